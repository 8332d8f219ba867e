"""CPU: tt2.data.normalize_corpus and the corpus tool's arguments.  No GPU: the normaliser is a
stand-in built on the float64 numpy reference (tests/_loudness_refs.py)."""
import importlib.util
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import _loudness_refs as R
from tt2 import data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StubNormalizer:
    """LoudnessNormalizer's normalize() on the host, by the numpy reference."""

    def __init__(self, sr=22050, target=-23.0, peak_db=-1.0, sr_in=None, cut=None):
        self.sr_in, self.sr_out = sr if sr_in is None else sr_in, sr
        self.p = R.default_params(sr, target, peak_db)
        self.cut = cut or {}          # batch row -> samples kept (a trimmer in front)
        self.calls = []

    def params(self):
        return {"sr": self.sr_out, "step": self.p["step"], "target_ms": self.p["target_ms"], "ceiling": self.p["ceiling"]}

    def normalize(self, audio, lens=None):
        B, L = audio.shape
        lens = [L] * B if lens is None else [int(n) for n in lens]
        lens = [self.cut.get(b, n) for b, n in enumerate(lens)]
        self.calls.append((B, L, list(lens)))
        r = R.reference(audio.numpy(), lens, n_out=L, **self.p)
        return (torch.from_numpy(r["y"]), torch.tensor(lens, dtype=torch.int32), torch.from_numpy(r["loud"]),
                torch.from_numpy(r["gain"]), torch.from_numpy(r["peak"]), torch.tensor(r["limited"], dtype=torch.int32))


def level_corpus(root, sr=22050, n=5):
    """Noise at levels 12 dB apart; utterance 2 is 0.3 s long (below four steps: unmeasured),
    utterance 3 is quiet but for one loud sample (the peak ceiling sets its gain)."""
    os.makedirs(os.path.join(root, "wavs"))
    rng = np.random.default_rng(4)
    lines, sigs = [], []
    for i in range(n):
        uid = f"U{i:03d}"
        length = int(sr * (0.3 if i == 2 else 0.7 + 0.1 * i))
        x = 0.2 * 10.0 ** (-12.0 * i / 20.0) * rng.normal(size=length)
        if i == 3:
            x[2000] = 0.95
        pcm = np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16)
        wavfile.write(os.path.join(root, "wavs", uid + ".wav"), sr, pcm)
        sigs.append((pcm / 32768.0).astype(np.float32))
        lines.append(f"{uid}|Raw {i}.|Normalised text {i}.")
    with open(os.path.join(root, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return root, sigs


def test_normalize_corpus_files_and_manifest(tmp_path):
    root, sigs = level_corpus(str(tmp_path / "c"))
    ds = data.LJSpeech(root)
    nz = StubNormalizer()
    out = str(tmp_path / "norm")
    man = data.normalize_corpus(ds, out, nz, batch_size=3)
    assert [c[0] for c in nz.calls] == [3, 2] and nz.calls[0][1] == max(len(s) for s in sigs[:3])
    assert nz.calls[0][2] == [len(s) for s in sigs[:3]]
    assert man == json.load(open(os.path.join(out, "loudness.json")))
    assert set(man) == {"normalizer", "utterances", "unmeasured", "empty", "stats"}
    assert man["normalizer"] == nz.params() and man["unmeasured"] == ["U002"] and man["empty"] == []
    louds = []
    for i, s in enumerate(sigs):
        uid = f"U{i:03d}"
        u = man["utterances"][uid]
        assert set(u) == {"samples", "loudness_in", "gain_db", "peak_in", "limited", "clipped"}
        r = R.reference(s[None, :], None, n_out=len(s), **nz.p)
        g = float(r["gain"][0])
        assert u["samples"] == len(s) and u["peak_in"] == float(r["peak"][0]) and u["clipped"] == 0
        assert u["limited"] is bool(r["limited"][0]) and u["gain_db"] == pytest.approx(20 * math.log10(g), abs=1e-12)
        rate, pcm = wavfile.read(os.path.join(out, "wavs", uid + ".wav"))
        assert rate == 22050 and pcm.dtype == np.int16 and len(pcm) == len(s)
        assert np.array_equal(pcm, np.rint(r["y"][0].astype(np.float64) * 32768).astype(np.int16))
        if i == 2:
            assert u["loudness_in"] is None and u["gain_db"] == 0.0 and not u["limited"]
            assert np.array_equal(pcm, np.rint(s * 32768).astype(np.int16))       # copied at gain 1
            continue
        assert u["loudness_in"] == float(r["loud"][0])
        louds.append(u["loudness_in"])
        if i != 3:
            assert abs(u["loudness_in"] + u["gain_db"] + 23.0) < 1e-4 and not u["limited"]
    u3 = man["utterances"]["U003"]
    assert u3["limited"] and u3["loudness_in"] + u3["gain_db"] < -23.5
    assert abs(10 ** (u3["gain_db"] / 20) * u3["peak_in"] - 10 ** (-1 / 20)) < 1e-6
    assert louds[0] - louds[1] == pytest.approx(12.0, abs=0.3)
    st = man["stats"]
    assert set(st) == {"measured", "limited", "mean_loudness_in", "min_loudness_in", "max_loudness_in"}
    assert (st["measured"], st["limited"]) == (4, 1)
    assert st["mean_loudness_in"] == pytest.approx(sum(louds) / 4, rel=1e-12)
    assert (st["min_loudness_in"], st["max_loudness_in"]) == (min(louds), max(louds))
    assert open(os.path.join(out, "metadata.csv"), "rb").read() == open(os.path.join(root, "metadata.csv"), "rb").read()
    again = data.LJSpeech(out)
    assert [u for u, _ in again.items] == [f"U{i:03d}" for i in range(5)]
    # a second pass over the normalised corpus finds it at the target (PCM16 rounding apart)
    man2 = data.normalize_corpus(again, str(tmp_path / "norm2"), StubNormalizer(), batch_size=8)
    for i in (0, 1, 4):
        assert abs(man2["utterances"][f"U{i:03d}"]["loudness_in"] + 23.0) < 0.02


def test_an_utterance_left_empty_by_a_trimmer_in_front_is_not_written(tmp_path):
    root, sigs = level_corpus(str(tmp_path / "c"), n=3)
    out = str(tmp_path / "o")
    man = data.normalize_corpus(data.LJSpeech(root), out, StubNormalizer(cut={1: 0}), batch_size=16)
    assert man["empty"] == ["U001"] and man["unmeasured"] == ["U001", "U002"]
    assert man["utterances"]["U001"]["samples"] == 0 and man["stats"]["measured"] == 1
    assert sorted(os.listdir(os.path.join(out, "wavs"))) == ["U000.wav", "U002.wav"]
    src = open(os.path.join(root, "metadata.csv")).read().splitlines()
    assert open(os.path.join(out, "metadata.csv")).read().splitlines() == [ln for ln in src if not ln.startswith("U001|")]


def test_a_corpus_with_nothing_measured_has_null_statistics(tmp_path):
    root = str(tmp_path / "c")
    os.makedirs(os.path.join(root, "wavs"))
    wavfile.write(os.path.join(root, "wavs", "A.wav"), 22050, np.zeros(30000, dtype=np.int16))
    open(os.path.join(root, "metadata.csv"), "w").write("A|x|x\n")
    man = data.normalize_corpus(data.LJSpeech(root), str(tmp_path / "o"), StubNormalizer())
    assert man["unmeasured"] == ["A"] and man["stats"]["measured"] == 0 and man["stats"]["mean_loudness_in"] is None
    assert json.load(open(str(tmp_path / "o" / "loudness.json"))) == man          # strict JSON: no -Infinity
    assert "Infinity" not in open(str(tmp_path / "o" / "loudness.json")).read()


def test_normalize_corpus_refusals(tmp_path):
    root, _ = level_corpus(str(tmp_path / "c"), n=2)
    ds = data.LJSpeech(root)
    with pytest.raises(ValueError, match="48000 Hz"):
        data.normalize_corpus(ds, str(tmp_path / "o"), StubNormalizer(sr_in=48000))
    with pytest.raises(ValueError, match="batch_size"):
        data.normalize_corpus(ds, str(tmp_path / "o"), StubNormalizer(), batch_size=0)
    with pytest.raises(ValueError, match="corpus itself"):
        data.normalize_corpus(ds, os.path.join(root, "."), StubNormalizer())
    assert not os.path.exists(str(tmp_path / "o"))


def _tool():
    spec = importlib.util.spec_from_file_location("normalize_corpus_tool", os.path.join(ROOT, "tools", "normalize_corpus.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_arguments():
    tool = _tool()
    a = tool.parse_args(["--in", "A", "--out", "B"])
    assert (a.src, a.out, a.sr_in, a.target, a.peak_db, a.trim, a.top_db, a.batch) == ("A", "B", 22050, -23.0, -1.0, False, 60.0, 16)
    a = tool.parse_args(["--in", "A", "--out", "B", "--sr-in", "48000", "--target", "-18.5", "--peak-db", "-3", "--trim",
                         "--top-db", "35.5", "--frame", "1024", "--hop", "256", "--keep", "220", "--batch", "4"])
    assert (a.sr_in, a.target, a.peak_db, a.trim, a.top_db, a.frame, a.hop, a.keep, a.batch) == \
        (48000, -18.5, -3.0, True, 35.5, 1024, 256, 220, 4)
    with pytest.raises(SystemExit):
        tool.parse_args(["--in", "A"])


def test_tool_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "normalize_corpus.py"), "--help"], capture_output=True,
                       text=True)
    assert r.returncode == 0
    for word in ("--in", "--out", "--sr-in", "--target", "--peak-db", "--trim", "--top-db", "--batch", "loudness.json",
                 "BS.1770", "R128"):
        assert word in r.stdout, word
