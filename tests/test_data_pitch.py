"""CPU: tt2.audio.phoneme_average against a Python loop, and tt2.data.extract_pitch with a stub
extractor (the files and manifest it writes, the corpus statistics, the refusal on a duration
mismatch) plus the argument parsing of tools/extract_pitch.py."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tt2.audio import Pitch, phoneme_average
from tt2.data import extract_pitch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def average_loop(values, durations, mask=None):
    B, T = values.shape
    out = np.zeros(durations.shape, np.float64)
    for b in range(B):
        pos = 0
        for p, d in enumerate(durations[b]):
            fr = [t for t in range(pos, min(pos + max(int(d), 0), T)) if mask is None or mask[b, t]]
            pos += max(int(d), 0)
            out[b, p] = sum(float(values[b, t]) for t in fr) / len(fr) if fr else 0.0
    return out


def test_phoneme_average_against_a_loop():
    rng = np.random.default_rng(1)
    B, T, Tx = 4, 23, 7
    v = rng.uniform(50, 400, (B, T)).astype(np.float32)
    mask = rng.random((B, T)) < 0.6
    dur = np.array([[3, 0, 5, 1, 0, 10, 4],      # zero durations, sums to T
                    [2, 2, 2, 2, 2, 2, 2],       # sums short: frames 14.. belong to no phoneme
                    [0, 0, 23, 0, 0, 0, 0],      # one phoneme owns everything
                    [4, 4, 4, 4, 4, 4, 4]])      # sums long: clipped at T
    mask[0, 3:8] = False                         # phoneme 2 of utterance 0: unvoiced only
    mask[3, 20:] = True
    for m in (None, mask):
        got = phoneme_average(torch.from_numpy(v), torch.from_numpy(dur), None if m is None else torch.from_numpy(m))
        want = average_loop(v, dur, m)
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, Tx)
        assert np.allclose(got.numpy(), want, rtol=1e-6, atol=0), (got, want)
    got = phoneme_average(torch.from_numpy(v), torch.from_numpy(dur), torch.from_numpy(mask)).numpy()
    assert got[0, 2] == 0 and got[0, 1] == 0 and got[0, 4] == 0 and got[1, 0] != 0
    assert got[3, 6] == 0 and got[3, 5] == pytest.approx(v[3, 20:23].astype(np.float64).mean(), rel=1e-6)   # 20..22; 6 starts at 24
    # int32 durations and a float64 track
    g64 = phoneme_average(torch.from_numpy(v).double(), torch.from_numpy(dur).int())
    assert g64.dtype == torch.float64 and np.allclose(g64.numpy(), average_loop(v, dur), rtol=1e-12)
    with pytest.raises(ValueError):
        phoneme_average(torch.zeros(2, 5), torch.zeros(3, 4, dtype=torch.long))


class StubPitch:
    """Frame tracks made from the audio itself: f0 = 100 + the frame's first sample where that is
    positive, else unvoiced; energy = |first sample|."""

    def params(self):
        return {"fmin": 65.0, "fmax": 600.0, "threshold": 0.1, "stub": True}

    def __call__(self, audio, lens):
        B, L = audio.shape
        T = 1 + L // 256
        first = torch.zeros(B, T)
        first[:, :L // 256 + (1 if L % 256 else 0)] = audio[:, ::256][:, :T]
        frames = (1 + lens // 256).to(torch.int32)
        live = torch.arange(T)[None, :] < frames[:, None]
        f0 = torch.where((first > 0) & live, 100.0 + first, torch.zeros(()))
        return Pitch(f0, f0 > 0, torch.where(f0 > 0, 0.05, 1.0), torch.where(live, first.abs(), torch.zeros(())), frames)


def corpus():
    rng = np.random.default_rng(4)
    a1 = rng.uniform(-50, 50, (2, 256 * 6 + 10)).astype(np.float32)
    a2 = rng.uniform(-50, 50, (1, 256 * 3)).astype(np.float32)
    a1[0, 0], a1[0, 256] = 20.0, 30.0           # voiced frames for the phoneme averages
    return [(["u1", "u2"], torch.from_numpy(a1), torch.tensor([256 * 6 + 10, 256 * 4 + 5], dtype=torch.int32)),
            (["u3"], torch.from_numpy(a2), torch.tensor([256 * 3], dtype=torch.int32))]


def test_extract_pitch_files_manifest_and_statistics(tmp_path):
    out, dur_dir = str(tmp_path / "pitch"), str(tmp_path / "dur")
    os.makedirs(dur_dir)
    np.save(os.path.join(dur_dir, "u1.npy"), np.array([2, 0, 4, 1], np.int32))     # sums to 7 frames
    np.save(os.path.join(dur_dir, "u3.npy"), np.array([1, 3], np.int32))           # 4 frames; u2 has none
    batches = corpus()
    stub = StubPitch()
    man = extract_pitch(iter(batches), out, stub, durations_dir=dur_dir)
    assert man == json.load(open(os.path.join(out, "pitch.json")))
    assert man["extractor"] == stub.params()
    assert {k: v["frames"] for k, v in man["utterances"].items()} == {"u1": 7, "u2": 5, "u3": 4}
    files = sorted(os.listdir(out))
    assert files == sorted(["pitch.json", "u1.f0.npy", "u1.energy.npy", "u1.f0_ph.npy", "u1.energy_ph.npy",
                            "u2.f0.npy", "u2.energy.npy", "u3.f0.npy", "u3.energy.npy", "u3.f0_ph.npy",
                            "u3.energy_ph.npy"])
    all_f0, all_en = [], []
    for ids, audio, lens in batches:
        p = stub(audio, lens)
        for b, uid in enumerate(ids):
            n = int(p.frames[b])
            f0, en = np.load(os.path.join(out, f"{uid}.f0.npy")), np.load(os.path.join(out, f"{uid}.energy.npy"))
            assert f0.dtype == np.float32 and en.dtype == np.float32 and f0.shape == (n,) and en.shape == (n,)
            assert np.array_equal(f0, p.f0[b, :n].numpy()) and np.array_equal(en, p.energy[b, :n].numpy())
            assert man["utterances"][uid]["voiced"] == pytest.approx(float((f0 > 0).mean()))
            all_f0.append(f0[f0 > 0].astype(np.float64))
            all_en.append(en.astype(np.float64))
            dpath = os.path.join(dur_dir, f"{uid}.npy")
            if os.path.exists(dpath):
                d = np.load(dpath)
                f_ph, e_ph = np.load(os.path.join(out, f"{uid}.f0_ph.npy")), np.load(os.path.join(out, f"{uid}.energy_ph.npy"))
                assert f_ph.dtype == np.float32 and f_ph.shape == d.shape and e_ph.shape == d.shape
                assert np.allclose(f_ph, average_loop(f0[None], d[None], (f0 > 0)[None])[0], rtol=1e-6)
                assert np.allclose(e_ph, average_loop(en[None], d[None])[0], rtol=1e-6)
    assert np.load(os.path.join(out, "u1.f0_ph.npy"))[0] == 125.0 and np.load(os.path.join(out, "u1.f0_ph.npy"))[1] == 0
    lf, en = np.log(np.concatenate(all_f0)), np.concatenate(all_en)
    assert man["log_f0"]["frames"] == lf.size and man["energy"]["frames"] == en.size == 16
    assert man["log_f0"]["mean"] == pytest.approx(lf.mean(), rel=1e-9) and man["log_f0"]["std"] == pytest.approx(lf.std(), rel=1e-6)
    assert man["energy"]["mean"] == pytest.approx(en.mean(), rel=1e-9) and man["energy"]["std"] == pytest.approx(en.std(), rel=1e-6)
    # without a durations directory: no phoneme files
    out2 = str(tmp_path / "plain")
    extract_pitch(batches, out2, stub)
    assert not [f for f in os.listdir(out2) if f.endswith("_ph.npy")] and len(os.listdir(out2)) == 7


def test_extract_pitch_refuses_a_duration_mismatch(tmp_path):
    dur_dir = str(tmp_path / "dur")
    os.makedirs(dur_dir)
    np.save(os.path.join(dur_dir, "u2.npy"), np.array([2, 2], np.int32))   # 4, but u2 has 5 frames
    with pytest.raises(ValueError, match="u2"):
        extract_pitch(corpus(), str(tmp_path / "out"), StubPitch(), durations_dir=dur_dir)


def test_an_empty_corpus_writes_an_empty_manifest(tmp_path):
    man = extract_pitch([], str(tmp_path / "o"), StubPitch())
    assert man["utterances"] == {} and man["log_f0"] == {"mean": 0.0, "std": 0.0, "frames": 0}
    assert not math.isnan(man["energy"]["std"])


def test_tool_arguments():
    spec = importlib.util.spec_from_file_location("extract_pitch_tool", os.path.join(ROOT, "tools", "extract_pitch.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(["--data", "/d", "--out", "o"])
    assert (a.data, a.out, a.durations, a.batch, a.fmin, a.fmax, a.threshold, a.limit) == \
        ("/d", "o", None, 16, 65.0, 600.0, 0.1, 0)
    a = tool.parse_args(["--data", "/d", "--out", "o", "--durations", "dd", "--batch", "4", "--fmin", "80",
                         "--fmax", "400.5", "--threshold", "0.15", "--limit", "10"])
    assert (a.durations, a.batch, a.fmin, a.fmax, a.threshold, a.limit) == ("dd", 4, 80.0, 400.5, 0.15, 10)
    for bad in (["--out", "o"], ["--data", "/d"], ["--data", "/d", "--out", "o", "--batch", "x"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
