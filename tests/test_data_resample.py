"""CPU: the data path around the resampler (tt2.data): read_wav, LJSpeech at another rate, collate
with a resampler, resample_corpus and the corpus tool's arguments.  No GPU: the resampler is a stub
built on the float64 numpy reference (tests/_resample_refs.py) and the extractor a stub that records
what it is given."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import _resample_refs as R
from tt2 import data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StubResampler:
    """The Resampler signature on the host: the numpy reference with the float64 bank."""

    def __init__(self, sr_in, sr_out=22050, gain=1.0):
        self.sr_in, self.sr_out, self.gain = sr_in, sr_out, gain
        self.up, self.down, self.half, self.taps = R.design(sr_in, sr_out)
        self.calls = []

    def params(self):
        return {"sr_in": self.sr_in, "sr_out": self.sr_out, "up": self.up, "down": self.down, "half": self.half,
                "zeros": 24, "rolloff": 0.9, "beta": 10.0}

    def __call__(self, audio, lens=None):
        B, L = audio.shape
        lens = [L] * B if lens is None else [int(n) for n in lens]
        self.calls.append((B, L, list(lens)))
        y = torch.zeros(B, R.out_len(L, self.up, self.down), dtype=torch.float32)
        for b in range(B):
            yb = self.gain * R.resample(audio[b].numpy(), lens[b], self.taps, self.up, self.down, self.half)
            y[b, :len(yb)] = torch.from_numpy(yb.astype(np.float32))
        return y, torch.tensor([R.out_len(n, self.up, self.down) for n in lens], dtype=torch.int32)


class StubExtractor:
    def __init__(self):
        self.seen = None

    def __call__(self, audio, lens):
        self.seen = (audio.clone(), lens.clone())
        frames = 1 + lens // 256
        return torch.zeros(audio.shape[0], 1 + audio.shape[1] // 256, 80), frames.to(torch.int32)


def mini_corpus(root, sr, n=3, amp=0.3):
    os.makedirs(os.path.join(root, "wavs"))
    lines, sigs = [], []
    for i in range(n):
        uid = f"U{i:03d}"
        x = amp * np.sin(2 * np.pi * (220 + 60 * i) * np.arange(sr // 8 + 777 * i) / sr + 0.1 * i)
        pcm = np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16)
        wavfile.write(os.path.join(root, "wavs", uid + ".wav"), sr, pcm)
        sigs.append(pcm / 32768.0)
        lines.append(f"{uid}|Raw {i}.|Normalised text {i}.")
    with open(os.path.join(root, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return root, sigs


def test_read_wav_against_load_wav(tmp_path):
    rng = np.random.default_rng(0)
    x = rng.uniform(-0.9, 0.9, size=(500, 2))
    files = {"pcm16": (x[:, 0] * 32767).astype(np.int16), "pcm32": (x[:, 0] * 2147483647).astype(np.int32),
             "float": x[:, 0].astype(np.float32), "float_stereo": x.astype(np.float32)}
    for name, arr in files.items():
        for sr in (22050, 48000):
            path = str(tmp_path / f"{name}_{sr}.wav")
            wavfile.write(path, sr, arr)
            y, rate = data.read_wav(path)
            assert rate == sr and isinstance(rate, int) and y.dtype == np.float32 and y.shape == (500,)
            assert np.array_equal(y, data.load_wav(path, sr))
            want = x.mean(axis=1) if arr.ndim == 2 else x[:, 0]
            assert np.abs(y - want).max() < 1e-4
    with pytest.raises(ValueError, match="48000 Hz, expected 22050"):
        data.load_wav(str(tmp_path / "pcm16_48000.wav"))
    with pytest.raises(ValueError, match="resample"):
        data.load_wav(str(tmp_path / "float_22050.wav"), 16000)
    assert np.array_equal(data.read_wav(str(tmp_path / "pcm16_48000.wav"))[0], files["pcm16"] / np.float32(32768))


def test_ljspeech_at_another_rate(tmp_path):
    root, sigs = mini_corpus(str(tmp_path / "c48"), 48000)
    ds = data.LJSpeech(root, sr=48000)
    assert ds.sr == 48000 and len(ds) == 3
    w = ds.wav(1)
    assert w.dtype == np.float32 and len(w) == 6000 + 777 and np.array_equal(w, sigs[1].astype(np.float32))
    assert data.LJSpeech(root).sr == 22050
    with pytest.raises(ValueError, match="48000 Hz"):
        data.LJSpeech(root).wav(0)                    # the default still refuses it


def test_collate_runs_the_resampler_between_upload_and_extractor(tmp_path):
    root, sigs = mini_corpus(str(tmp_path / "c48"), 48000)
    ds = data.LJSpeech(root, sr=48000)
    rs, ex = StubResampler(48000), StubExtractor()
    text, text_len, mel, mel_len = data.collate(ds, [2, 0], ex, device="cpu", resampler=rs)
    n2, n0 = 6000 + 2 * 777, 6000
    assert rs.calls == [(2, n2, [n2, n0])]
    audio, lens = ex.seen
    o2, o0 = R.out_len(n2, 147, 320), R.out_len(n0, 147, 320)
    assert lens.tolist() == [o2, o0] and lens.dtype == torch.int32 and audio.shape == (2, o2)
    want0 = R.resample(sigs[0].astype(np.float32), n0, rs.taps, 147, 320, rs.half).astype(np.float32)
    assert np.array_equal(audio[1, :o0].numpy(), want0) and not audio[1, o0:].any()
    assert mel_len.tolist() == [1 + o2 // 256, 1 + o0 // 256] and mel_len.dtype == torch.long
    assert mel.shape[0] == 2 and text.shape[0] == 2 and text_len.tolist() == [len(ds.ids(2)), len(ds.ids(0))]
    # without the argument nothing changes: the extractor sees the corpus' own samples and lengths
    ex2 = StubExtractor()
    data.collate(ds, [2, 0], ex2, device="cpu")
    assert ex2.seen[1].tolist() == [n2, n0] and ex2.seen[0].shape == (2, n2)
    # a resampler for another input rate is refused, before anything is loaded
    with pytest.raises(ValueError, match="44100"):
        data.collate(ds, [0], ex, device="cpu", resampler=StubResampler(44100))
    with pytest.raises(ValueError, match="22050"):
        data.collate(data.LJSpeech(root), [0], ex, device="cpu", resampler=rs)


def test_resample_corpus_files_rounding_clipping_and_manifest(tmp_path):
    root, sigs = mini_corpus(str(tmp_path / "c48"), 48000, n=3, amp=0.9)
    ds = data.LJSpeech(root, sr=48000)
    rs = StubResampler(48000, gain=1.25)               # 0.9 * 1.25 exceeds the PCM16 range
    out = str(tmp_path / "c22")
    man = data.resample_corpus(ds, out, rs, batch_size=2)
    assert [c[0] for c in rs.calls] == [2, 1]           # batches of two in corpus order
    assert man == json.load(open(os.path.join(out, "resample.json")))
    assert man["resampler"] == rs.params() and sorted(man["utterances"]) == ["U000", "U001", "U002"]
    assert open(os.path.join(out, "metadata.csv")).read() == open(os.path.join(root, "metadata.csv")).read()
    assert sorted(os.listdir(os.path.join(out, "wavs"))) == ["U000.wav", "U001.wav", "U002.wav"]
    for i, uid in enumerate(("U000", "U001", "U002")):
        n_in = 6000 + 777 * i
        rate, pcm = wavfile.read(os.path.join(out, "wavs", uid + ".wav"))
        assert rate == 22050 and pcm.dtype == np.int16 and pcm.ndim == 1
        y = (1.25 * R.resample(sigs[i].astype(np.float32), n_in, rs.taps, 147, 320, rs.half)).astype(np.float32)
        q = np.rint(y.astype(np.float64) * 32768.0)
        clipped = int(((q > 32767) | (q < -32768)).sum())
        assert clipped > 0 and pcm.max() == 32767 and pcm.min() == -32768
        assert np.array_equal(pcm, np.clip(q, -32768, 32767).astype(np.int16))
        assert man["utterances"][uid] == {"samples_in": n_in, "samples_out": R.out_len(n_in, 147, 320),
                                          "clipped": clipped}
    # the written corpus is one the default data path reads
    ds2 = data.LJSpeech(out)
    assert len(ds2) == 3 and len(ds2.wav(2)) == R.out_len(6000 + 2 * 777, 147, 320) and ds2.ids(1) == ds.ids(1)
    with pytest.raises(ValueError, match="44100"):
        data.resample_corpus(ds, str(tmp_path / "x"), StubResampler(44100))
    with pytest.raises(ValueError, match="itself"):
        data.resample_corpus(ds, root, rs)


def test_rint_is_round_half_to_even_and_no_clip_below_full_scale(tmp_path):
    """rint(x * 32768): 0.5 quanta go to the even code, -1.0 is representable, +1.0 clips."""
    root = str(tmp_path / "c")
    os.makedirs(os.path.join(root, "wavs"))
    wavfile.write(os.path.join(root, "wavs", "A.wav"), 22050, np.zeros(6, dtype=np.float32))
    open(os.path.join(root, "metadata.csv"), "w").write("A|a|a\n")

    class Fixed:
        sr_in, sr_out = 22050, 22050

        def params(self):
            return {}

        def __call__(self, audio, lens):
            y = torch.tensor([[0.5 / 32768, 1.5 / 32768, -0.5 / 32768, -1.0, 1.0, 32767.4 / 32768]])
            return y, torch.tensor([6], dtype=torch.int32)

    man = data.resample_corpus(data.LJSpeech(root), str(tmp_path / "o"), Fixed())
    _, pcm = wavfile.read(str(tmp_path / "o" / "wavs" / "A.wav"))
    assert pcm.tolist() == [0, 2, 0, -32768, 32767, 32767] and man["utterances"]["A"]["clipped"] == 1


def test_tool_arguments():
    spec = importlib.util.spec_from_file_location("resample_corpus_tool", os.path.join(ROOT, "tools",
                                                                                      "resample_corpus.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(["--in", "A", "--out", "B", "--sr-in", "48000"])
    assert (a.src, a.out, a.sr_in, a.sr, a.zeros, a.rolloff, a.beta, a.batch) == ("A", "B", 48000, 22050, 24, 0.9,
                                                                                  10.0, 16)
    a = tool.parse_args(["--in", "A", "--out", "B", "--sr-in", "44100", "--sr", "16000", "--zeros", "16",
                         "--rolloff", "0.95", "--beta", "8", "--batch", "4"])
    assert (a.sr_in, a.sr, a.zeros, a.rolloff, a.beta, a.batch) == (44100, 16000, 16, 0.95, 8.0, 4)
    for argv in (["--out", "B", "--sr-in", "48000"], ["--in", "A", "--sr-in", "48000"], ["--in", "A", "--out", "B"]):
        with pytest.raises(SystemExit):
            tool.parse_args(argv)
