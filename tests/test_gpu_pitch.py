"""tt2.audio.PitchExtractor and the F0 scoring of tt2.evaluate (GPU).

PitchExtractor: the padded buffer it leaves equals numpy's reflect padding, its outputs equal a
direct tt2_yin launch on that buffer bit for bit, and that launch obeys the comparison rules of
tests/test_gpu_yin_kernels.py against the float64 reference of tests/_yin_refs.py (d' within
1600 * 2^-24 relative; the reference's selection on the kernel's own d' reproduces lag, voicing
and aper).  A pitch call between two mel extractions leaves the second bit-identical.

f0_metrics against a numpy loop on hand-made tracks and paths, the NaN cases included.  f0_dtw of
a signal with itself is 0 / 0 / 0; of a tone against the same tone 50 cents sharp, rmse_cents is
within 2 cents of 50.  The tones' harmonic mix changes over the utterance, so the DTW path is held
near the diagonal by the timbre while the pitch offset is the same everywhere; the first and last
frames, where the reflect padding breaks the period, are off by up to 12 cents in the float64
reference too.  The float64 reference tracks scored by the numpy loop along the kernel's own path
give 50.02 and 50.07 cents (the kernel: 50.02 and 50.07; on the diagonal path, on the CPU alone,
50.00 and 50.03), so the bar of 2 cents stands; the reference's value is asserted as well."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _yin_refs as R  # noqa: E402
from tt2 import audio, evaluate, ops  # noqa: E402

U, check_selection = R.U, R.check_selection


@pytest.fixture(scope="module")
def mx():
    return audio.MelExtractor()


def voiced_batch():
    """[3, 4000] f32: tones with a second harmonic plus a little noise, then a noisy stretch."""
    rng = np.random.default_rng(5)
    L = 4000
    t = np.arange(L) / R.SR
    x = np.zeros((3, L), np.float32)
    for b, f in enumerate((110.0, 207.3, 311.0)):
        y = 0.4 * np.sin(2 * np.pi * f * t + b) + 0.15 * np.sin(4 * np.pi * f * t) + 0.004 * rng.normal(size=L)
        y[2600:3300] = 0.2 * rng.normal(size=700)
        x[b] = y
    return x, [4000, 2500, 1300]


def test_extractor_against_the_reference(mx):
    x, lens = voiced_batch()
    px = audio.PitchExtractor(mx)
    xd, ld = torch.from_numpy(x).cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")
    p = px(xd, ld)
    _, mel_frames = mx(xd, ld)
    B, T = 3, 1 + 4000 // 256
    assert tuple(p.f0.shape) == (B, T) and p.voiced.dtype == torch.bool and p.frames.dtype == torch.int32
    assert torch.equal(p.frames, mel_frames) and p.frames.tolist() == [1 + n // 256 for n in lens]
    assert torch.equal(p.voiced, p.f0 > 0)
    # the same launch by hand on numpy's padding, with d'
    P = mx.plan(B, 4000)
    pad = np.zeros((B, P.Lp), np.float32)
    for b, n in enumerate(lens):
        pad[b, :n + 1024] = R.reflect_pad(x[b], n)
    padded = torch.from_numpy(pad).cuda()
    px(xd, ld)
    assert torch.equal(P.padded.view(B, P.Lp), padded)
    f0 = torch.empty(B, T, device="cuda")
    lag = torch.empty(B, T, dtype=torch.int32, device="cuda")
    aper, en = torch.empty_like(f0), torch.empty_like(f0)
    cm = torch.full((B, T, px.tau_max + 1), float("nan"), device="cuda")
    ops.yin(padded.view(-1), P.Lp, f0, lag, aper, en, 256, px.tau_min, px.tau_max, R.SR, px.threshold,
            frames=p.frames, cmnd=cm)
    for got, want in ((p.f0, f0), (p.aperiodicity, aper), (p.energy, en)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    out = {"f0": f0.cpu().numpy(), "lag": lag.cpu().numpy(), "aper": aper.cpu().numpy(), "energy": en.cpu().numpy(),
           "cmnd": cm.cpu().numpy()}
    voiced = 0
    for b in range(B):
        nv = 1 + lens[b] // 256
        for f in range(T):
            if f >= nv:
                assert (out["f0"][b, f], out["lag"][b, f], out["aper"][b, f], out["energy"][b, f]) == (0, -1, 1, 0)
                continue
            y = pad[b, f * 256:f * 256 + 1024]
            ref, _, _ = R.cmnd_of(y, np.float64)
            got = out["cmnd"][b, f].astype(np.float64)
            assert (np.abs(got - ref[:px.tau_max + 1]) <= 1600 * U * ref[:px.tau_max + 1]).all(), (b, f)
            r = check_selection(out, b, f, out["cmnd"][b, f], px.tau_min, px.tau_max, px.threshold)
            voiced += r["voiced"]
            e64 = float(R.energy_of(y, np.float64))
            assert abs(float(out["energy"][b, f]) - e64) <= 600 * U * e64
    # the tones are found: utterance 0's frames before the noisy stretch, away from the padded ends
    mid = out["f0"][0, 2:9]
    assert (np.abs(1200 * np.log2(mid / 110.0)) < 5).all(), mid
    assert voiced >= 12 and not p.voiced[0, 11].item()   # frame 11 lies inside the noise


def test_mel_is_untouched_by_a_pitch_call_in_between(mx):
    x, lens = voiced_batch()
    xd, ld = torch.from_numpy(x).cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")
    px = audio.PitchExtractor(mx, fmin=80.0, fmax=500.0, threshold=0.15)
    mel1, fr1 = mx(xd, ld)
    p = px(xd, ld)
    mel2, fr2 = mx(xd, ld)
    assert torch.equal(mel1.view(torch.int32), mel2.view(torch.int32)) and torch.equal(fr1, fr2)
    assert torch.equal(p.frames, fr1)
    p2 = px(xd, None)   # no lengths: every frame valid
    assert p2.frames.tolist() == [16, 16, 16] and p2.f0.data_ptr() != p.f0.data_ptr()
    assert bool((p.energy[2, 6:] == 0).all()) and bool((p2.energy[2, 6:] > 0).any())


def metrics_loop(fh, fr, ph, pr, length):
    out = []
    for b in range(len(length)):
        sq, n, gross, vuv = 0.0, 0, 0, 0
        for k in range(int(length[b])):
            h, r = float(fh[b, ph[b, k]]), float(fr[b, pr[b, k]])
            if h > 0 and r > 0:
                n += 1
                sq += (1200 * math.log2(h / r)) ** 2
                gross += abs(h / r - 1) > 0.2
            vuv += (h > 0) != (r > 0)
        L = int(length[b])
        out.append((math.sqrt(sq / n) if n else math.nan, vuv / L if L else math.nan, gross / n if n else math.nan, n))
    return out


def test_f0_metrics_against_a_numpy_loop():
    rng = np.random.default_rng(9)
    B, Th, Tr = 5, 12, 10
    fh = rng.uniform(80, 400, (B, Th)).astype(np.float32)
    fr = rng.uniform(80, 400, (B, Tr)).astype(np.float32)
    fh[rng.random((B, Th)) < 0.3] = 0
    fr[rng.random((B, Tr)) < 0.3] = 0
    fr[0, :8] = fh[0, :8] * np.float32(1.1)      # a row with small errors
    fh[2], fr[2, ::2] = 0, 0                      # no doubly voiced cell: rmse and gpe are NaN
    P = Th + Tr - 1
    ph, pr = np.full((B, P), -1, np.int32), np.full((B, P), -1, np.int32)
    length = np.zeros(B, np.int32)
    for b in range(B):
        if b == 3:
            continue                              # an empty path: everything NaN, 0 pairs
        i = j = 0
        cells = [(0, 0)]
        while (i, j) != (Th - 1, Tr - 1):
            move = rng.integers(0, 3)
            i2, j2 = min(i + (move != 2), Th - 1), min(j + (move != 1), Tr - 1)
            if (i2, j2) != (i, j):
                i, j = i2, j2
                cells.append((i, j))
        length[b] = len(cells)
        ph[b, :len(cells)], pr[b, :len(cells)] = [c[0] for c in cells], [c[1] for c in cells]
    length[4] = 4                                 # a path cut short: only its first cells count
    s = evaluate.f0_metrics(*(torch.from_numpy(a).cuda() for a in (fh, fr, ph, pr, length)))
    assert s.rmse_cents.dtype == torch.float32 and s.voiced_pairs.dtype == torch.int32
    want = metrics_loop(fh, fr, ph, pr, length)
    got = list(zip(s.rmse_cents.tolist(), s.vuv_error.tolist(), s.gpe.tolist(), s.voiced_pairs.tolist()))
    for b, (g, w) in enumerate(zip(got, want)):
        for name, x, y in zip(("rmse", "vuv", "gpe", "pairs"), g, w):
            if isinstance(y, float) and math.isnan(y):
                assert math.isnan(x), (b, name, x)
            else:
                assert abs(x - y) <= 1e-6 * max(1.0, abs(y)), (b, name, x, y)
    assert math.isnan(got[2][0]) and math.isnan(got[2][2]) and not math.isnan(got[2][1]) and got[2][3] == 0
    assert all(math.isnan(v) for v in got[3][:3]) and got[3][3] == 0
    assert got[0][3] > 0


def evolving_tone(f, n):
    """A tone whose second and third harmonics swell and fade over the utterance."""
    t = np.arange(n) / R.SR
    u = np.arange(n) / n
    return (0.4 * (0.4 + 0.6 * u) * np.sin(2 * np.pi * f * t) + 0.3 * (1 - u) * np.sin(4 * np.pi * f * t + 0.7) +
            0.2 * np.sin(np.pi * u) * np.sin(6 * np.pi * f * t)).astype(np.float32)


def test_f0_dtw_of_a_signal_with_itself(mx):
    x, lens = voiced_batch()
    xd, ld = torch.from_numpy(x).cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")
    s, m = evaluate.f0_dtw(xd, ld, xd.clone(), ld, pitch=audio.PitchExtractor(mx))
    assert s.rmse_cents.tolist() == [0, 0, 0] and s.vuv_error.tolist() == [0, 0, 0] and s.gpe.tolist() == [0, 0, 0]
    assert m.length.tolist() == [1 + n // 256 for n in lens] and m.total.tolist() == [0, 0, 0]
    assert (s.voiced_pairs > 0).all()


def test_f0_dtw_fifty_cents_sharp(mx):
    n = 8192
    T = 1 + n // 256
    tones = [(200.0, 200.0 * 2 ** (50 / 1200)), (140.0 * 2 ** (50 / 1200), 140.0)]   # hyp flat, then hyp sharp
    hyp = np.stack([evolving_tone(h, n) for h, _ in tones])
    ref = np.stack([evolving_tone(r, n) for _, r in tones])
    px = audio.PitchExtractor(mx)
    s, m = evaluate.f0_dtw(torch.from_numpy(hyp).cuda(), None, torch.from_numpy(ref).cuda(), None, pitch=px)
    # the float64 reference tracks scored along the same path
    def track(x):
        p = R.reflect_pad(x, n)
        return np.array([float(R.yin_frame(p[f * 256:f * 256 + 1024], px.tau_min, px.tau_max, px.threshold)["f0"])
                         for f in range(T)])
    th, tr = np.stack([track(x) for x in hyp]), np.stack([track(x) for x in ref])
    want = metrics_loop(th, tr, m.path_hyp.cpu().numpy(), m.path_ref.cpu().numpy(), m.length.cpu().numpy())
    print("kernel rmse_cents", s.rmse_cents.tolist(), "reference", [w[0] for w in want], "pairs", s.voiced_pairs.tolist(),
          "path cells", m.length.tolist(), "vuv", s.vuv_error.tolist())
    for b in range(2):
        assert abs(want[b][0] - 50) < 2, want[b]                     # the reference reaches the bar
        assert abs(float(s.rmse_cents[b]) - 50) < 2, s.rmse_cents
        assert int(s.voiced_pairs[b]) >= T - 6 and float(s.gpe[b]) == 0
        assert float(s.vuv_error[b]) <= 4 / T
