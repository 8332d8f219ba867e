"""YIN pitch kernel (tt2_yin) against the numpy references of tests/_yin_refs.py (GPU), by direct
C-ABI calls on hand-built buffers.

Exact problem (_yin_refs.exact_signal): samples are integers in -3..3, so d, S and d * tau are
integers below 2^24 (tests/test_yin_refs.py asserts it) and exact in f32 in any summation order;
lag, aper, energy, every d' written to cmnd and the unrefined f0 must then equal the f32 twin bit
for bit.  The refined f0 is held to 1e-6 relative of the float64 formula evaluated on the kernel's
own (a, b, c): its f32 evaluation makes 7 roundings (three differences, a sum, a product that is
exact, two quotients and a sum), each amplified at most once by a well-conditioned step (off is at
most 1/2 against a lag of at least 2), about 8 * 2^-24 = 4.8e-7.  Everything the kernel must not
read is NaN (samples past an utterance's valid frames), the outputs sit between NaN guard bands,
and the cmnd rows are pre-filled with NaN so that the tail past tau_max and the rows of invalid
frames must still hold it.

Random real-valued problem: d' against the float64 reference within 1600 * 2^-24 relative.  With
u = 2^-24: a term (y[j] - y[j + tau])^2 carries 2u from the rounded difference and the sum of 512
non-negative terms adds at most 512u in any order (the fma rounds once per add), so d is within
514u; S adds up to 511 such values with at most 510 more roundings, within 1024u; the numerator
d * tau adds one rounding and the correctly rounded divide one more: 514 + 1 + 1024 + 1 = 1540u to
first order, 1600u with the second-order terms.  The reference's selection is then run on the
kernel's own d': it must reproduce lag and voicing exactly and aper bit for bit, so a near-tie in
d' can neither make the test flaky nor hide a selection bug.  The energy is within 600u: 1024
roundings in the sum of squares, halved by the square root, plus the root's own and the scaling.

Measured (MI355X): worst relative error of d' 6.9e-7 .. 7.4e-7 over the three random problems, against
the bound 9.5e-5; 3, 3 and 5 of their 11 frames voiced."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _yin_refs as R  # noqa: E402
from tt2 import _lib  # noqa: E402

GUARD = 64
U, SR = R.U, R.SR
bits, check_selection = R.bits, R.check_selection
NAN = float("nan")


def guarded(n):
    """n f32 / int32 slots inside a NaN-filled f32 buffer, the interior NaN too: (whole, interior)."""
    whole = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, n):
    return bool(torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[GUARD + n:]).all())


def launch(x, stride, B, t, hop, tmin, tmax, thr, frames=None, cmnd_ld=None, sr=SR):
    """One tt2_yin call -> dict of numpy arrays f0, lag, aper, energy [B, t] and cmnd [B, t, ld]."""
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32).reshape(-1)).cuda() if isinstance(x, np.ndarray) else x
    outs = {k: guarded(B * t) for k in ("f0", "lag", "aper", "energy")}
    ld = (tmax + 5) if cmnd_ld is None else cmnd_ld
    wc, cm = guarded(B * t * ld) if ld else (None, None)
    fr = torch.tensor(frames, dtype=torch.int32, device="cuda") if frames is not None else None
    a = _lib.YinArgs()
    a.x, a.frames = xd.data_ptr(), _lib.ptr(fr)
    a.f0, a.lag, a.aper, a.energy = (outs[k][1].data_ptr() for k in ("f0", "lag", "aper", "energy"))
    a.cmnd, a.cmnd_ld, a.utt_stride = (cm.data_ptr() if ld else None), ld, stride
    a.batch, a.t, a.hop, a.tau_min, a.tau_max, a.sr, a.threshold = B, t, hop, tmin, tmax, sr, thr
    _lib.check(_lib.lib().tt2_yin(ctypes.byref(a), _lib.stream_ptr()), "tt2_yin")
    torch.cuda.synchronize()
    for k, (whole, _) in outs.items():
        assert guards_intact(whole, B * t), f"{k} guard bands"
    res = {k: outs[k][1].cpu().numpy().copy().reshape(B, t) for k in ("f0", "aper", "energy")}
    res["lag"] = outs["lag"][1].view(torch.int32).cpu().numpy().copy().reshape(B, t)
    if ld:
        assert guards_intact(wc, B * t * ld), "cmnd guard bands"
        res["cmnd"] = cm.cpu().numpy().copy().reshape(B, t, ld)
    return res


def check_exact(x, stride, B, t, hop, tmin, tmax, thr, frames, **kw):
    """Every output of one launch on integer samples against the f32 twin, bit for bit."""
    out = launch(x, stride, B, t, hop, tmin, tmax, thr, frames=frames, **kw)
    clean = np.nan_to_num(np.asarray(x, dtype=np.float32).reshape(B, stride), nan=1e30)
    for b in range(B):
        nv = t if frames is None else min(max(frames[b], 0), t)
        for f in range(t):
            if f >= nv:
                got = (out["f0"][b, f], out["lag"][b, f], out["aper"][b, f], out["energy"][b, f])
                assert got == (0, -1, 1, 0), (b, f, got)
                if "cmnd" in out:
                    assert np.isnan(out["cmnd"][b, f]).all(), (b, f, "cmnd row of an invalid frame written")
                continue
            y = clean[b, f * hop:f * hop + R.FRAME]
            assert np.abs(y).max() <= 3, "the test's own frame reads poison"
            cm, _, _ = R.cmnd_of(y, np.float32)
            if "cmnd" in out:
                row = out["cmnd"][b, f]
                assert np.array_equal(bits(row[:tmax + 1]), bits(cm[:tmax + 1])), (b, f, "cmnd")
                assert np.isnan(row[tmax + 1:]).all(), (b, f, "cmnd tail written")
            check_selection(out, b, f, cm, tmin, tmax, thr)
            assert bits(out["energy"][b, f]) == bits(R.energy_of(y, np.float32)), (b, f, "energy")
    return out


@pytest.mark.parametrize("tmin,tmax,thr", R.EXACT_PARAMS, ids=[f"{a}-{b}-thr{c}" for a, b, c in R.EXACT_PARAMS])
def test_exact_integer_problem(tmin, tmax, thr):
    x = R.exact_signal(poison=True)
    out = check_exact(x, R.EXACT_STRIDE, R.EXACT_B, R.EXACT_T, R.HOP, tmin, tmax, thr, list(R.EXACT_FRAMES))
    if (tmin, tmax, thr) == (36, 340, 0.1):   # what the designed frames are there for
        assert out["lag"][0, 0] == 50 and out["lag"][0, 4] == 340 and out["lag"][0, 8] == 36
        assert out["aper"][0, 8] == 0 and out["f0"][1, 0] == 0 and out["aper"][1, 0] == 1
    again = launch(x, R.EXACT_STRIDE, R.EXACT_B, R.EXACT_T, R.HOP, tmin, tmax, thr, frames=list(R.EXACT_FRAMES))
    for k in out:
        assert np.array_equal(out[k].view(np.int32), again[k].view(np.int32)), k   # NaN poison included


EDGES = {
    "frames-null": dict(frames=None),
    "frames-clamped": dict(frames=[100, -3, 9]),
    "t1": dict(t=1, frames=[1, 1, 0]),
    "B1": dict(B=1, frames=[9]),
    "t10-last-group-of-two": dict(t=10, hop=200, frames=[10, 5, 9]),
    "hop1": dict(hop=1, frames=[9, 4, 0]),
    "hop300": dict(hop=300, t=7, frames=[7, 3, 7]),
    "no-cmnd": dict(frames=[9, 4, 0], cmnd_ld=0),
    "cmnd-ld-exact": dict(frames=[9, 4, 0], cmnd_ld="tight"),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_parameter_edges(name):
    e = dict(EDGES[name])
    x = R.exact_signal(poison=False)
    B, t, hop = e.get("B", R.EXACT_B), e.get("t", R.EXACT_T), e.get("hop", R.HOP)
    assert (t - 1) * hop + R.FRAME <= R.EXACT_STRIDE
    kw = {}
    for tmin, tmax, thr in ((36, 340, 0.1), (1, 511, 0.1)):
        if "cmnd_ld" in e:
            kw["cmnd_ld"] = tmax + 1 if e["cmnd_ld"] == "tight" else e["cmnd_ld"]
        check_exact(x[:B], R.EXACT_STRIDE, B, t, hop, tmin, tmax, thr, e["frames"], **kw)


def test_byte_offsets_past_2_31():
    """Utterance 1 starts more than 2^31 bytes into x, and its cmnd row more than 2^31 bytes into cmnd."""
    stride = (1 << 29) + 24
    x = torch.empty(stride + 2 * R.FRAME, dtype=torch.float32, device="cuda")
    sig = R.exact_signal(poison=False)
    x[:R.FRAME] = torch.from_numpy(sig[0, :R.FRAME]).cuda()
    x[stride:stride + R.FRAME] = torch.from_numpy(sig[0, R.FRAME:2 * R.FRAME]).cuda()
    out = launch(x, stride, 2, 1, R.HOP, 36, 340, 0.1, cmnd_ld=0)
    for b in range(2):
        y = sig[0, b * R.FRAME:(b + 1) * R.FRAME]
        cm, _, _ = R.cmnd_of(y, np.float32)
        check_selection(out, b, 0, cm, 36, 340, 0.1)
        assert bits(out["energy"][b, 0]) == bits(R.energy_of(y, np.float32))
    del x
    torch.cuda.empty_cache()


def random_signal(seed, snrs):
    """[2, 6 * 256 + 1024 - 256] samples: per utterance, segments of a two-harmonic tone plus white
    noise at the given SNRs (dB; None: noise alone), each 768 samples with a pitch of its own."""
    rng = np.random.default_rng(seed)
    n = 5 * R.HOP + R.FRAME
    x = np.zeros((2, n))
    for b in range(2):
        pos = 0
        for k, snr in enumerate(snrs[b]):
            m = min(768, n - pos)
            f = rng.uniform(80, 400)
            tt = np.arange(m) / SR
            tone = np.sin(2 * np.pi * f * tt + k) + 0.4 * np.sin(4 * np.pi * f * tt + 0.3)
            noise = rng.normal(size=m)
            x[b, pos:pos + m] = noise if snr is None else tone + noise * 10 ** (-snr / 20) * np.sqrt(0.58)
            pos += m
    return (0.3 * x).astype(np.float32)


RANDOM = [(1, (36, 340, 0.1)), (2, (1, 511, 0.15)), (3, (20, 400, 0.3))]


@pytest.mark.parametrize("seed,params", RANDOM, ids=[f"seed{s}-{p[0]}-{p[1]}" for s, p in RANDOM])
def test_random_real_valued_problem(seed, params):
    tmin, tmax, thr = params
    B, t = 2, 6
    x = random_signal(seed, ([40, 20, 5], [10, None, 30]))
    stride = x.shape[1]
    out = launch(x, stride, B, t, R.HOP, tmin, tmax, thr, frames=[6, 5])
    worst, voiced = 0.0, 0
    for b, nv in enumerate((6, 5)):
        for f in range(nv):
            y = x[b, f * R.HOP:f * R.HOP + R.FRAME]
            ref, _, _ = R.cmnd_of(y, np.float64)
            got = out["cmnd"][b, f, :tmax + 1].astype(np.float64)
            err = np.abs(got - ref[:tmax + 1]) / ref[:tmax + 1]
            worst = max(worst, float(err.max()))
            assert err.max() <= 1600 * U, (b, f, float(err.max()))
            assert np.isnan(out["cmnd"][b, f, tmax + 1:]).all()
            r = check_selection(out, b, f, out["cmnd"][b, f], tmin, tmax, thr)
            voiced += r["voiced"]
            e64 = float(R.energy_of(y, np.float64))
            assert abs(float(out["energy"][b, f]) - e64) <= 600 * U * e64, (b, f)
    assert out["lag"][1, 5] == -1 and np.isnan(out["cmnd"][1, 5]).all()
    print(f"worst relative error of d' {worst:.3e} (bound {1600 * U:.3e}); {voiced} of 11 frames voiced")
    assert 0 < voiced < 11   # the problem exercises both outcomes
    again = launch(x, stride, B, t, R.HOP, tmin, tmax, thr, frames=[6, 5])
    for k in out:
        assert np.array_equal(out[k].view(np.int32), again[k].view(np.int32)), k
