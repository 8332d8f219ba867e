"""CPU: tt2.data.trim_corpus and the corpus tool's arguments.  No GPU: the trimmer is a stand-in built
on the float64 numpy reference (tests/_trim_refs.py)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import _trim_refs as R
from tt2 import data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StubTrimmer:
    """SilenceTrimmer's trim() on the host, by the numpy reference."""

    def __init__(self, sr=22050, hop=64, r=2, keep=0, top_db=40.0, gain=1.0, sr_in=None):
        self.sr_in, self.sr_out = sr if sr_in is None else sr_in, sr
        self.hop, self.r, self.keep, self.gain = hop, r, keep, gain
        self.ratio = np.float32(10.0 ** (-top_db / 10.0))
        self.calls = []

    def params(self):
        return {"hop": self.hop, "r": self.r, "keep": self.keep, "ratio": float(self.ratio), "sr": self.sr_out}

    def trim(self, audio, lens=None, want_energy=False):
        B, L = audio.shape
        lens = [L] * B if lens is None else [int(n) for n in lens]
        self.calls.append((B, L, list(lens)))
        y, outs, starts, en = R.reference(audio.numpy(), lens, self.hop, self.r, self.keep, self.ratio, L)
        return (torch.from_numpy((self.gain * y).astype(np.float32)), torch.tensor(outs, dtype=torch.int32),
                torch.tensor(starts, dtype=torch.int32), None)


def padded_corpus(root, sr=22050, n=4):
    """Tones between stretches of exact silence; utterance 2 is silence only."""
    os.makedirs(os.path.join(root, "wavs"))
    lines, sigs = [], []
    for i in range(n):
        uid = f"U{i:03d}"
        lead, body, tail = 700 + 130 * i, 3000 + 500 * i, 400 + 90 * i
        tone = 0.3 * np.sin(2 * np.pi * (220 + 60 * i) * np.arange(body) / sr + 0.1 * i)
        x = np.concatenate([np.zeros(lead), tone if i != 2 else np.zeros(body), np.zeros(tail)])
        pcm = np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16)
        wavfile.write(os.path.join(root, "wavs", uid + ".wav"), sr, pcm)
        sigs.append((pcm / 32768.0).astype(np.float32))
        lines.append(f"{uid}|Raw {i}.|Normalised text {i}.")
    with open(os.path.join(root, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return root, sigs


def test_trim_corpus_files_and_manifest(tmp_path):
    root, sigs = padded_corpus(str(tmp_path / "c"))
    ds = data.LJSpeech(root)
    tr = StubTrimmer(keep=10)
    out = str(tmp_path / "trimmed")
    man = data.trim_corpus(ds, out, tr, batch_size=3)
    assert [c[0] for c in tr.calls] == [3, 1] and tr.calls[0][1] == max(len(s) for s in sigs[:3])
    assert tr.calls[0][2] == [len(s) for s in sigs[:3]]
    assert man == json.load(open(os.path.join(out, "trim.json")))
    assert set(man) == {"trimmer", "utterances", "removed_seconds", "empty"}
    assert man["trimmer"] == tr.params() and man["empty"] == ["U002"]
    removed = 0.0
    for i, s in enumerate(sigs):
        uid = f"U{i:03d}"
        u = man["utterances"][uid]
        assert set(u) == {"samples_in", "start", "samples_out", "clipped"}
        _, outs, starts, _ = R.reference(s[None, :], None, tr.hop, tr.r, tr.keep, tr.ratio, len(s))
        assert (u["samples_in"], u["start"], u["samples_out"], u["clipped"]) == (len(s), starts[0], outs[0], 0)
        removed += (len(s) - outs[0]) / 22050
        path = os.path.join(out, "wavs", uid + ".wav")
        if i == 2:
            assert outs[0] == 0 and not os.path.exists(path)
            continue
        lead = 700 + 130 * i
        assert 0 < lead - starts[0] <= 10 + 2 * tr.hop and outs[0] < len(s) - 300
        rate, pcm = wavfile.read(path)
        assert rate == 22050 and pcm.dtype == np.int16 and pcm.ndim == 1 and len(pcm) == outs[0]
        # PCM16 in, PCM16 out: the samples themselves
        assert np.array_equal(pcm, np.rint(s[starts[0]:starts[0] + outs[0]] * 32768).astype(np.int16))
    assert man["removed_seconds"] == pytest.approx(removed, rel=1e-12)
    # metadata.csv without the empty utterance's line, the others as they were
    src = open(os.path.join(root, "metadata.csv")).read().splitlines()
    assert open(os.path.join(out, "metadata.csv")).read().splitlines() == [ln for ln in src if not ln.startswith("U002|")]
    again = data.LJSpeech(out)
    assert [u for u, _ in again.items] == ["U000", "U001", "U003"] and len(again.wav(2)) == man["utterances"]["U003"]["samples_out"]
    assert sorted(os.listdir(os.path.join(out, "wavs"))) == ["U000.wav", "U001.wav", "U003.wav"]


def test_trim_corpus_without_empties_copies_metadata_and_clips(tmp_path):
    root, sigs = padded_corpus(str(tmp_path / "c"), n=2)
    out = str(tmp_path / "t")
    man = data.trim_corpus(data.LJSpeech(root), out, StubTrimmer(gain=4.0), batch_size=16)
    assert man["empty"] == []
    assert open(os.path.join(out, "metadata.csv"), "rb").read() == open(os.path.join(root, "metadata.csv"), "rb").read()
    for i in range(2):
        u = man["utterances"][f"U{i:03d}"]
        _, pcm = wavfile.read(os.path.join(out, "wavs", f"U{i:03d}.wav"))
        q = np.rint(4.0 * sigs[i][u["start"]:u["start"] + u["samples_out"]].astype(np.float64) * 32768.0)
        assert u["clipped"] == int(((q < -32768) | (q > 32767)).sum()) > 0
        assert np.array_equal(pcm, np.clip(q, -32768, 32767).astype(np.int16)) and pcm.max() == 32767


def test_trim_corpus_with_a_rate_change_counts_seconds_at_both_rates(tmp_path):
    root, sigs = padded_corpus(str(tmp_path / "c"), sr=44100, n=2)
    tr = StubTrimmer(sr=22050, sr_in=44100)          # (a stand-in: it trims and relabels the rate)
    man = data.trim_corpus(data.LJSpeech(root, sr=44100), str(tmp_path / "t"), tr)
    want = sum(len(s) / 44100 - man["utterances"][f"U{i:03d}"]["samples_out"] / 22050 for i, s in enumerate(sigs))
    assert man["removed_seconds"] == pytest.approx(want, rel=1e-12)
    assert wavfile.read(str(tmp_path / "t" / "wavs" / "U000.wav"))[0] == 22050


def test_trim_corpus_refusals(tmp_path):
    root, _ = padded_corpus(str(tmp_path / "c"))
    ds = data.LJSpeech(root)
    with pytest.raises(ValueError, match="48000 Hz"):
        data.trim_corpus(ds, str(tmp_path / "o"), StubTrimmer(sr_in=48000))
    with pytest.raises(ValueError, match="batch_size"):
        data.trim_corpus(ds, str(tmp_path / "o"), StubTrimmer(), batch_size=0)
    with pytest.raises(ValueError, match="corpus itself"):
        data.trim_corpus(ds, os.path.join(root, "."), StubTrimmer())
    assert not os.path.exists(str(tmp_path / "o"))


def _tool():
    spec = importlib.util.spec_from_file_location("trim_corpus_tool", os.path.join(ROOT, "tools", "trim_corpus.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_arguments():
    tool = _tool()
    a = tool.parse_args(["--in", "A", "--out", "B"])
    assert (a.src, a.out, a.sr_in, a.top_db, a.frame, a.hop, a.keep, a.batch) == ("A", "B", 22050, 60.0, 2048, 512, 0, 16)
    a = tool.parse_args(["--in", "A", "--out", "B", "--sr-in", "48000", "--top-db", "35.5", "--frame", "1024",
                         "--hop", "256", "--keep", "220", "--batch", "4"])
    assert (a.sr_in, a.top_db, a.frame, a.hop, a.keep, a.batch) == (48000, 35.5, 1024, 256, 220, 4)
    with pytest.raises(SystemExit):
        tool.parse_args(["--in", "A"])


def test_tool_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "trim_corpus.py"), "--help"], capture_output=True,
                       text=True)
    assert r.returncode == 0
    for word in ("--in", "--out", "--sr-in", "--top-db", "--frame", "--hop", "--keep", "--batch", "trim.json", "librosa"):
        assert word in r.stdout, word
