"""Loudness kernels (tt2_loudness) against the float64 reference of tests/_loudness_refs.py (GPU), by
direct C-ABI calls on hand-built buffers.

x, y and energy are NaN-filled and sit between NaN guard bands; loud, gain, peak and limited are
NaN- or sentinel-filled between guard bands; x is NaN at and past each utterance's length and in its
pad columns, so a sample read where none may be read turns the peak, an energy or a state into NaN.
The pad widths of x, y and energy differ (5 or 6, 11 or 12, 3), x's and y's leading dimensions are
odd, so that rows start at every alignment a float can have, and x's base is shifted besides.  After
a launch the guards, the pad columns and every output that was not asked for must be untouched.

Exact problems (_loudness_refs.exact_problems): every intermediate is an integer (asserted before
each launch), so energy, peak, limited, loud, gain and y are compared bit for bit.  The random
problem runs the default 22.05 kHz coefficients: energy, loud and gain within 2 f32 ulp of the float64
reference (the float64 scheme itself is within 1e-9: the bar is the output rounding with one ulp of
slack), the gate decisions re-derived from the kernel's own energies identical, peak and limited
exact, y bit-equal to f32(gain * x) with the kernel's own gain.

Measured (MI355X): the worst errors are 0.497 (energy), 0.446 (loud) and 0.449 (gain) f32 ulp."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _loudness_refs as R  # noqa: E402
from tt2 import _lib  # noqa: E402

GUARD = 64
EPAD = 3
NAN = float("nan")
SENT = -77
bits = R.bits
ALL = ("y", "loud", "gain", "peak", "limited", "energy")


def guarded(n, dtype=torch.float32):
    fill = NAN if dtype == torch.float32 else SENT
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def untouched(t):
    return bool(torch.isnan(t).all()) if t.dtype == torch.float32 else bool((t == SENT).all())


def guards_intact(whole, n):
    return untouched(whole[:GUARD]) and untouched(whole[GUARD + n:])


def pads(n_in, n_out):
    """Pad widths that make x_ld and y_ld odd."""
    return (5 if n_in % 2 == 0 else 6), (11 if n_out % 2 == 0 else 12)


def launch(p, want=ALL, expect=0, shift=0, x_null=False):
    """One tt2_loudness call on problem p (a dict as _loudness_refs makes them).  want: the outputs
    given (the others are null); shift moves x's base by that many floats.  Returns a dict of numpy
    arrays (None where not asked for) and the alignments of x's rows."""
    x = np.asarray(p["x"], dtype=np.float32)
    lens, step, n_out = p["lens"], p["step"], p["n_out"]
    B, n_in = x.shape
    ne = n_in // step + 1
    xpad, ypad = pads(n_in, n_out)
    x_ld, y_ld, e_ld = n_in + xpad, n_out + ypad, ne + EPAD
    xh = np.full((B, x_ld), np.nan, dtype=np.float32)
    for b in range(B):
        L = R.clamp_len(None if lens is None else lens[b], n_in)
        xh[b, :L] = x[b, :L]
    wx, xd = guarded(B * x_ld + shift)
    xd = xd[shift:]
    xd.copy_(torch.from_numpy(xh.reshape(-1)))
    wy, yd = guarded(B * y_ld)
    we, ed = guarded(B * e_ld)
    vec = {k: guarded(B, torch.int32 if k == "limited" else torch.float32) for k in ("loud", "gain", "peak", "limited")}
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda") if lens is not None else None
    L_ = _lib.lib()
    need = L_.tt2_loudness_workspace_size(B, n_in, step)
    wws, ws = guarded((need + 3) // 4 + 4)
    off = (-ws.data_ptr() // 4) % 4                     # the workspace 16-byte aligned
    a = _lib.LoudnessArgs()
    a.x, a.lens = (None if x_null else xd.data_ptr()), _lib.ptr(ld)
    a.y = wy.data_ptr() + 4 * GUARD if "y" in want else None
    a.energy = ed.data_ptr() if "energy" in want else None
    for k in vec:
        setattr(a, k, vec[k][1].data_ptr() if k in want else None)
    a.workspace, a.workspace_bytes = ws.data_ptr() + 4 * off, need
    a.x_ld, a.y_ld, a.energy_ld = x_ld, y_ld, e_ld
    a.batch, a.n_in, a.n_out, a.step = B, n_in, n_out, step
    a.coef = (ctypes.c_double * 10)(*p["coef"])
    a.abs_sum, a.rel_ratio, a.target_ms, a.ceiling = p["abs_sum"], p["rel_ratio"], p["target_ms"], p["ceiling"]
    rc = L_.tt2_loudness(ctypes.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, L_.tt2_last_error())
    for whole, n in [(wx, B * x_ld + shift), (wy, B * y_ld), (we, B * e_ld), (wws, (need + 3) // 4 + 4)] + [
            (vec[k][0], B) for k in vec]:
        assert guards_intact(whole, n), "guard bands"
    yh = yd.cpu().numpy().copy().reshape(B, y_ld)
    eh = ed.cpu().numpy().copy().reshape(B, e_ld)
    assert np.isnan(yh[:, n_out:]).all(), "y written at or past n_out"
    assert np.isnan(eh[:, ne:]).all(), "energy written past n_in / step"
    assert np.array_equal(bits(xd.cpu().numpy()), bits(xh.reshape(-1))), "x written"
    for k, t in [("y", yd), ("energy", ed)] + [(k, vec[k][1]) for k in vec]:
        assert k in want or untouched(t), f"{k} was not asked for and was written"
    got = {k: (vec[k][1].cpu().numpy().copy() if k in want else None) for k in vec}
    got["y"] = yh[:, :n_out] if "y" in want else None
    got["energy"] = eh[:, :ne] if "energy" in want else None
    align = [((xd.data_ptr() // 4) + b * x_ld) % 4 for b in range(B)]
    return got, align


def run_ref(p):
    return R.reference(**{k: v for k, v in p.items() if k != "name"})


def check(got, ref, what):
    keys = tuple(k for k in ALL if got[k] is not None)
    full = dict(ref)
    full.update({k: got[k] for k in keys})
    assert R.same(full, ref, keys) == [], what


PROBLEMS = R.exact_problems()
DROPS = [ALL] + [tuple(k for k in ALL if k != d) for d in ALL]


@pytest.mark.parametrize("step", R.STEPS)
def test_exact_integer_problems(step):
    """Ragged B = 5, lengths around 4 step, every chunk and segment seam, 0, negative and above n_in;
    n_out either side of the lengths; each output absent in turn (y among them: measuring only)."""
    seen_align, turn = set(), 0
    for p in [q for q in PROBLEMS if q["step"] == step]:
        assert R.exact(p), p["name"]
        ref = run_ref(p)
        for shift in ((0, 1, 2, 3) if p["x"].shape[1] < 200 else (turn % 4,)):
            turn += 1
            got, align = launch(p, want=DROPS[turn % len(DROPS)], shift=shift)
            seen_align |= set(align)
            check(got, ref, (p["name"], shift))
    assert seen_align == {0, 1, 2, 3}
    # lens null: every utterance is n_in long
    q = [q for q in PROBLEMS if q["step"] == step and len(q["lens"]) == 5][-1]
    n_in = q["x"].shape[1]
    b = int(np.argmax([R.clamp_len(v, n_in) for v in q["lens"]]))
    L = R.clamp_len(q["lens"][b], n_in)
    p = dict(q, x=q["x"][b:b + 1, :L].copy(), lens=None, n_out=L + 2)
    assert R.exact(dict(p, lens=[L]))
    check(launch(p)[0], run_ref(p), "lens null")


def test_a_long_utterance_takes_every_loop_round_again():
    """300 003 samples: 293 segments, so the segment scan runs five rounds and the sub-block and peak
    loops of the last launch go round again; at step 5 a block sum needs 60 000 sequential adds."""
    n_in = 300_003
    rng = np.random.default_rng(5)
    sections = R.FILTERS["p4-p6"]
    x = np.stack([R.exact_utterance(rng, n_in, sections, (4, 1, 0, 4, 1)),
                  R.exact_utterance(rng, n_in, sections, (1, 0, 4))]).astype(np.float32)
    for step in (2205, 5):
        p = dict(name="long", x=x, lens=[n_in, 299_500], step=step, coef=R.coef10(sections), abs_sum=8.0 * step,
                 rel_ratio=0.125, target_ms=0.5, ceiling=2.0 ** -3, n_out=n_in + 1)
        ref = R.reference(**{k: v for k, v in p.items() if k != "name"})
        sub = np.concatenate(ref["sub"])
        assert sub.max() < 2 ** 24 and np.all(sub == np.rint(sub)) and np.abs(x).max() < 2 ** 10
        got, _ = launch(p)
        check(got, ref, ("long", step))
        assert all(m is not None for m in ref["ms"])


def test_batch_position_independence_and_repeatability():
    """The same utterance at b = 0 of one batch and b = 3 of another, among other neighbours, lengths,
    n_in, n_out and leading dimensions: the same bits (default coefficients on noise, so every
    rounding matters); and the same call twice."""
    rng = np.random.default_rng(11)
    n = 7001
    u = (0.1 * rng.normal(size=n)).astype(np.float32)
    a = (0.3 * rng.normal(size=(2, n))).astype(np.float32)
    a[0] = u
    b = (0.3 * rng.normal(size=(5, n + 1234))).astype(np.float32)
    b[3, :n] = u
    d = R.default_params()
    d["step"], d["abs_sum"] = 441, d["abs_sum"] / 5
    pa = dict(d, x=a, lens=[n, n - 5], n_out=n)
    pb = dict(d, x=b, lens=[n + 1234, 17, 0, n, 4000], n_out=n + 2000)
    ga, _ = launch(pa)
    gb, _ = launch(pb)
    S = n // 441
    assert np.isfinite(ga["loud"][0]) and S > 10
    for k in ("loud", "gain", "peak"):
        assert bits(ga[k][0:1])[0] == bits(gb[k][3:4])[0], k
    assert ga["limited"][0] == gb["limited"][3]
    assert np.array_equal(bits(ga["energy"][0, :S]), bits(gb["energy"][3, :S]))
    assert np.array_equal(bits(ga["y"][0, :n]), bits(gb["y"][3, :n])) and not gb["y"][3, n:].any()
    again, _ = launch(pb)
    assert R.same(again, gb) == []


def test_zero_sizes():
    p = dict(PROBLEMS[2])
    # batch = 0: success, nothing written
    q = dict(p, x=p["x"][:0], lens=[])
    got, _ = launch(q)
    assert got["y"].shape == (0, p["n_out"])
    # n_out = 0 with y given: the measures are written, no sample is
    q = dict(p, n_out=0)
    check(launch(q)[0], run_ref(q), "n_out 0")
    # n_in = 0: unmeasured, zero-fill; x may be null
    for x_null in (False, True):
        q = dict(p, x=np.zeros((3, 0), dtype=np.float32), lens=None, n_out=700)
        got, _ = launch(q, x_null=x_null)
        assert np.array_equal(bits(got["y"]), bits(np.zeros((3, 700))))
        assert np.isneginf(got["loud"]).all() and (got["gain"] == 1).all() and not got["peak"].any()
        assert not got["limited"].any() and np.array_equal(bits(got["energy"]), bits(np.zeros((3, 1))))


def test_refusals_leave_the_buffers_untouched():
    p = PROBLEMS[2]
    x = p["x"][:2]
    n_in = x.shape[1]
    n_out, ne = 50, n_in // p["step"] + 1
    E = _lib.E_INVALID
    wy, yd = guarded(2 * (n_out + 11))
    we, ed = guarded(2 * (ne + EPAD))
    xd = torch.from_numpy(np.nan_to_num(x)).cuda()
    vec = {k: guarded(2, torch.int32 if k == "limited" else torch.float32)[1] for k in ("loud", "gain", "peak", "limited")}
    L = _lib.lib()
    need = L.tt2_loudness_workspace_size(2, n_in, p["step"])
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    none = dict(y=None, loud=None, gain=None, peak=None, limited=None, energy=None)
    for kw in (dict(step=0), dict(step=-4), dict(step=2 ** 29), dict(batch=-1), dict(n_in=-1), dict(n_out=-1),
               dict(x_ld=n_in - 1), dict(y_ld=n_out - 1), dict(energy_ld=ne - 1), dict(coef=(3, NAN)),
               dict(coef=(9, float("inf"))), dict(abs_sum=-1.0), dict(abs_sum=NAN), dict(rel_ratio=-0.1),
               dict(rel_ratio=1.5), dict(rel_ratio=NAN), dict(target_ms=0.0), dict(target_ms=NAN), dict(ceiling=0.0),
               dict(ceiling=float("inf")), dict(x=None), none, dict(workspace=None), dict(workspace_bytes=need - 1)):
        a = _lib.LoudnessArgs()
        a.x, a.y, a.energy = xd.data_ptr(), yd.data_ptr(), ed.data_ptr()
        for k in vec:
            setattr(a, k, vec[k].data_ptr())
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        a.x_ld, a.y_ld, a.energy_ld = n_in, n_out + 11, ne + EPAD
        a.batch, a.n_in, a.n_out, a.step = 2, n_in, n_out, p["step"]
        a.coef = (ctypes.c_double * 10)(*p["coef"])
        a.abs_sum, a.rel_ratio, a.target_ms, a.ceiling = 8.0, 0.125, 0.5, 0.25
        for k, v in kw.items():
            if k == "coef":
                a.coef[v[0]] = v[1]
            else:
                setattr(a, k, v)
        assert L.tt2_loudness(ctypes.byref(a), _lib.stream_ptr()) == E, kw
        assert b"tt2_loudness" in L.tt2_last_error()
    torch.cuda.synchronize()
    assert untouched(wy) and untouched(we) and all(untouched(t) for t in vec.values()) and bool((ws == 0x5A).all())


def ulps(got, want64):
    """|got - want| in units of the f32 ulp of want."""
    w = np.asarray(want64, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - w) / np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)


def test_the_random_problem_at_the_default_coefficients():
    x, lens = R.random_problem()
    d = R.default_params()
    p = dict(d, x=x, lens=lens, n_out=x.shape[1] - 2000)
    got, _ = launch(p)
    ref = run_ref(p)
    worst = dict(energy=0.0, loud=0.0, gain=0.0)
    for b in range(4):
        S = len(ref["sub"][b])
        worst["energy"] = max(worst["energy"], float(ulps(got["energy"][b, :S], ref["sub"][b]).max()))
        assert not got["energy"][b, S:].any()
        ms = ref["ms"][b]
        worst["loud"] = max(worst["loud"], float(ulps(got["loud"][b], -0.691 + 10 * np.log10(ms))))
        gd = min(np.sqrt(d["target_ms"] / ms), d["ceiling"] / float(ref["peak"][b]))
        worst["gain"] = max(worst["gain"], float(ulps(got["gain"][b], gd)))
        # the gate decisions from the kernel's own (f32) energies are the reference's
        _, _, pa, both, _ = R.gate(got["energy"][b, :S].astype(np.float64), d["step"], d["abs_sum"], d["rel_ratio"])
        assert np.array_equal(pa, ref["gates"][b][1]) and np.array_equal(both, ref["gates"][b][2])
    print("worst f32 ulps:", {k: round(v, 3) for k, v in worst.items()})
    assert worst["energy"] <= 2 and worst["loud"] <= 2 and worst["gain"] <= 2, worst
    assert np.array_equal(bits(got["peak"]), bits(ref["peak"])) and got["limited"].tolist() == ref["limited"].tolist()
    assert got["limited"].tolist() == [0, 0, 0, 1]
    own = np.zeros_like(got["y"])
    for b in range(4):
        m = min(lens[b], p["n_out"])
        own[b, :m] = got["gain"][b] * x[b, :m]
    assert np.array_equal(bits(got["y"]), bits(own))
