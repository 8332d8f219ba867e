"""Silence-trimming kernels (tt2_trim) against the float64 reference of tests/_trim_refs.py (GPU), by
direct C-ABI calls on hand-built buffers.

x, y and energy are NaN-filled and sit between NaN guard bands, out_lens and start are sentinel-filled
between guard bands; x is NaN at and past each utterance's length and in its pad columns, so a sample
read where none may be read turns an energy into NaN and with it the decision.  The pad widths of x,
y and energy differ (5 or 6, 11 or 12, 3), and x's and y's leading dimensions are odd, so that rows
start at every alignment a float can have.  After a launch the guards and the pad columns of y and
energy must still be NaN.

Exact problems (_trim_refs.exact_problems): integers in [-3, 3] and ratios 1/8, 1/4, 1/2, so every
square, partial sum and threshold is an exact f32 (asserted before each launch) and y, out_lens, start
and energy are compared bit for bit.  The random problem: Gaussian noise under a 40 dB stepped
envelope at top_db = 30; each energy within E[f] = frame 2^-24 sum x^2 of float64 (the sequential-sum
bound, which covers any order; _trim_refs' docstring), the reference decision re-run on the kernel's
own energies bit for bit, and the float64 decision for every utterance
(tests/test_trim_refs.py shows that no frame is within the bound of the threshold).

Measured (MI355X): the worst energy error is 0.0009 (hop 512, r 2) and 0.0057 (hop 64, r 3) of E[f]."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _trim_refs as R  # noqa: E402
from tt2 import _lib  # noqa: E402

GUARD = 64
EPAD = 3
NAN = float("nan")
SENT = -77
bits = R.bits


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


def launch(x, lens, hop, r, keep, ratio, n_out, want=(True, True, True), expect=0, x_null=False, shift=0):
    """One tt2_trim call.  x [B, n_in] numpy; lens a list (as passed, unclamped) or None;
    want = (out_lens, start, energy) given or null; shift moves x's base by that many floats.
    Returns (y [B, n_out], out_lens, start, energy [B, nf]) as numpy (None where not asked for) and
    the float addresses' alignments of x's rows."""
    x = np.asarray(x, dtype=np.float32)
    B, n_in = x.shape
    nf = n_in // hop + 1
    xpad, ypad = pads(n_in, n_out)
    x_ld, y_ld, e_ld = n_in + xpad, n_out + ypad, nf + EPAD
    xh = np.full((B, x_ld), np.nan, dtype=np.float32)
    for b in range(B):
        L = R.clamp_len(None if lens is None else lens[b], n_in)
        xh[b, :L] = x[b, :L]
    wx, xd = guarded(B * x_ld + shift)
    xd = xd[shift:]
    xd.copy_(torch.from_numpy(xh.reshape(-1)))
    wy, yd = guarded(B * y_ld)
    we, ed = guarded(B * e_ld)
    wo, od = guarded(B, torch.int32)
    wst, sd = guarded(B, torch.int32)
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda") if lens is not None else None
    L_ = _lib.lib()
    need = L_.tt2_trim_workspace_size(B, n_in, hop)
    wws, ws = guarded((need + 3) // 4 + 4)
    off = (-ws.data_ptr() // 4) % 4                     # the workspace 16-byte aligned
    a = _lib.TrimArgs()
    # (an empty view has a null data_ptr, and a null y is refused also when there is nothing to write)
    a.x, a.lens, a.y = (None if x_null else xd.data_ptr()), _lib.ptr(ld), wy.data_ptr() + 4 * GUARD
    a.out_lens = od.data_ptr() if want[0] else None
    a.start = sd.data_ptr() if want[1] else None
    a.energy = ed.data_ptr() if want[2] else None
    a.workspace, a.workspace_bytes = ws.data_ptr() + 4 * off, need
    a.x_ld, a.y_ld, a.energy_ld = x_ld, y_ld, e_ld
    a.batch, a.n_in, a.n_out, a.hop, a.r, a.keep, a.ratio = B, n_in, n_out, hop, r, keep, ratio
    rc = L_.tt2_trim(ctypes.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, L_.tt2_last_error())
    for whole, n in ((wx, B * x_ld + shift), (wy, B * y_ld), (we, B * e_ld), (wo, B), (wst, B),
                     (wws, (need + 3) // 4 + 4)):
        assert guards_intact(whole, n), "guard bands"
    yh = yd.cpu().numpy().copy().reshape(B, y_ld)
    eh = ed.cpu().numpy().copy().reshape(B, e_ld)
    assert np.isnan(yh[:, n_out:]).all(), "y written at or past n_out"
    assert np.isnan(eh[:, nf:]).all(), "energy written at or past n_in / hop + 1"
    assert np.array_equal(bits(xd.cpu().numpy()), bits(xh.reshape(-1))), "x written"
    for asked, t in zip(want, (od, sd, ed)):
        assert asked or untouched(t), "an output that was not asked for was written"
    align = [((xd.data_ptr() // 4) + b * x_ld) % 4 for b in range(B)]
    return (yh[:, :n_out], od.cpu().numpy().copy() if want[0] else None, sd.cpu().numpy().copy() if want[1] else None,
            eh[:, :nf] if want[2] else None), align


def check(got, ref, what):
    y, ol, st, en = got
    ry, rol, rst, ren = ref
    assert np.array_equal(bits(y), bits(ry)), ("y", what)
    assert ol is None or ol.tolist() == rol, ("out_lens", what, ol.tolist(), rol)
    assert st is None or st.tolist() == rst, ("start", what, st.tolist(), rst)
    assert en is None or np.array_equal(bits(en), bits(ren)), ("energy", what)


PROBLEMS = R.exact_problems()


@pytest.mark.parametrize("hop,r", R.GEOMETRIES, ids=[f"{h}-{r}" for h, r in R.GEOMETRIES])
def test_exact_integer_problems(hop, r):
    flip = 0
    seen_align = set()
    for p in [q for q in PROBLEMS if (q["hop"], q["r"]) == (hop, r)]:
        x, lens = p["x"], p["lens"]
        assert R.exact(x, hop, r, p["ratio"], lens)
        ref = R.reference(x, lens, hop, r, p["keep"], p["ratio"], p["n_out"])
        flip += 1
        want = (bool(flip % 3), bool(flip % 4), bool(flip % 2))      # every output both given and null
        got, align = launch(x, lens, hop, r, p["keep"], p["ratio"], p["n_out"], want=want)
        seen_align |= {al for al, v in zip(align, lens) if v > 0}
        what = (p["keep"], p["ratio"], p["n_out"])
        check(got, ref, what)
        assert R.judge((got[0], ref[1] if got[1] is None else got[1], ref[2] if got[2] is None else got[2], got[3]),
                       ref) == []
    assert seen_align == {0, 1, 2, 3}           # among them a row 4 bytes off 16-byte alignment
    # lens null: every utterance is n_in long; every shift of x's base
    p = PROBLEMS[[(q["hop"], q["r"]) for q in PROBLEMS].index((hop, r))]
    for shift in range(4):
        got, _ = launch(p["x"], None, hop, r, 1, 0.125, p["x"].shape[1] + 2, shift=shift)
        assert R.exact(p["x"], hop, r, 0.125)
        check(got, R.reference(p["x"], None, hop, r, 1, 0.125, p["x"].shape[1] + 2), ("lens null", shift))


def test_a_long_utterance_takes_every_loop_round_again():
    """About 300 000 samples: at hop 4 the 75 000 blocks are more than the energy pass's 4096 per trip
    and the frames more than the decision's 256 per trip, and the copy's columns more than its 262 144
    per trip; at hop 512 the blocks are the usual size."""
    n_in = 300_003
    rng = np.random.default_rng(5)
    x = np.zeros((2, n_in), dtype=np.float32)
    x[0, 70_001:290_000] = rng.integers(-3, 4, size=219_999)
    x[0, :70_001] = rng.integers(-1, 2, size=70_001) * (rng.random(70_001) < 0.02)
    x[1, 1000:299_000] = rng.integers(-2, 3, size=298_000)
    lens = [n_in, 299_500]
    for hop, r, keep in ((4, 3, 0), (512, 2, 100)):
        assert R.exact(x, hop, r, 2.0 ** -4, lens)
        got, _ = launch(x, lens, hop, r, keep, 2.0 ** -4, n_in + 1)
        ref = R.reference(x, lens, hop, r, keep, 2.0 ** -4, n_in + 1)
        check(got, ref, (hop, r))
        assert ref[1][1] > 262_144 + 4096 and ref[2][0] > 60_000


def test_a_row_beyond_two_to_the_31_bytes():
    """Row 1 of x and of y starts 2^31 + 32 bytes into its buffer; a few thousand samples are valid."""
    ld = (1 << 29) + 8
    n_in, n_out, hop, r = 5000, 5003, 256, 2
    rng = np.random.default_rng(8)
    xh = np.zeros((2, n_in), dtype=np.float32)
    xh[0, 1300:3000] = rng.integers(-3, 4, size=1700)
    xh[1, 2100:4100] = rng.integers(-3, 4, size=2000)
    lens = [4700, n_in]
    assert R.exact(xh, hop, r, 0.125, lens)
    x = torch.empty(ld + n_in, dtype=torch.float32, device="cuda")
    y = torch.empty(ld + n_out, dtype=torch.float32, device="cuda")
    for b in range(2):
        x[b * ld:b * ld + n_in] = torch.from_numpy(xh[b]).cuda()
        x[b * ld + lens[b]:b * ld + n_in + (8 if b == 0 else 0)] = NAN
        y[b * ld:b * ld + n_out] = NAN
    od = torch.full((2,), SENT, dtype=torch.int32, device="cuda")
    sd = torch.full((2,), SENT, dtype=torch.int32, device="cuda")
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    need = L.tt2_trim_workspace_size(2, n_in, hop)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    a = _lib.TrimArgs()
    a.x, a.lens, a.y, a.out_lens, a.start = x.data_ptr(), lens_d.data_ptr(), y.data_ptr(), od.data_ptr(), sd.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    a.x_ld, a.y_ld = ld, ld
    a.batch, a.n_in, a.n_out, a.hop, a.r, a.keep, a.ratio = 2, n_in, n_out, hop, r, 7, 0.125
    _lib.check(L.tt2_trim(ctypes.byref(a), _lib.stream_ptr()), "tt2_trim")
    torch.cuda.synchronize()
    ref = R.reference(xh, lens, hop, r, 7, 0.125, n_out)
    got = np.stack([y[b * ld:b * ld + n_out].cpu().numpy() for b in range(2)])
    assert od.tolist() == ref[1] and sd.tolist() == ref[2] and min(ref[1]) > 1000
    assert np.array_equal(bits(got), bits(ref[0]))
    del x, y
    torch.cuda.empty_cache()


def test_batch_position_independence_and_repeatability():
    """The same utterance at b = 0 of one batch and b = 3 of another, among different neighbours,
    other lengths, n_in, n_out and leading dimensions: the same bits (random data, so the order of
    the sums matters); and the same call twice."""
    rng = np.random.default_rng(11)
    hop, r, n = 256, 2, 7001
    env = np.repeat(rng.choice([0.001, 0.5], size=n // 100 + 1), 100)[:n]
    env[:2000] = env[-1500:] = 0.001                      # something to trim at either end
    u = (rng.normal(size=n) * env).astype(np.float32)
    a = (0.3 * rng.normal(size=(2, n))).astype(np.float32)
    a[0] = u
    b = (0.3 * rng.normal(size=(5, n + 1234))).astype(np.float32)
    b[3, :n] = u
    ratio = np.float32(1e-3)
    ga, _ = launch(a, [n, n - 5], hop, r, 3, ratio, n)
    gb, _ = launch(b, [n + 1234, 17, 0, n, 4000], hop, r, 3, ratio, n + 2000)
    assert ga[1][0] == gb[1][3] and ga[2][0] == gb[2][3] and 0 < ga[1][0] < n
    out = int(ga[1][0])
    F = R.n_frames(n, hop)
    assert np.array_equal(bits(ga[0][0, :out]), bits(gb[0][3, :out])) and not gb[0][3, out:].any()
    assert np.array_equal(bits(ga[3][0, :F]), bits(gb[3][3, :F]))
    again, _ = launch(b, [n + 1234, 17, 0, n, 4000], hop, r, 3, ratio, n + 2000)
    for g, h in zip(gb, again):
        assert np.array_equal(bits(g) if g.dtype == np.float32 else g, bits(h) if h.dtype == np.float32 else h)


def test_zero_sizes():
    x = R.exact_batch(4, 1)[0][:3]
    # batch = 0 and n_out = 0: success, nothing written (launch() checks the poison of what was not asked for;
    # here nothing may be written at all)
    for B, n_out in ((0, 10), (3, 0)):
        got, _ = launch(x[:B], None, 4, 1, 0, 0.125, n_out)
        assert got[0].shape == (B, n_out)
        if B:
            assert (got[1] == SENT).all() and (got[2] == SENT).all() and np.isnan(got[3]).all()
    # n_in = 0 with n_out > 0: zero-fills, out_lens = start = 0, the one energy column 0; x may be null
    for x_null in (False, True):
        got, _ = launch(np.zeros((3, 0), dtype=np.float32), None, 4, 1, 2, 0.125, 700, x_null=x_null)
        assert np.array_equal(bits(got[0]), bits(np.zeros((3, 700))))
        assert got[1].tolist() == [0, 0, 0] and got[2].tolist() == [0, 0, 0]
        assert np.array_equal(bits(got[3]), bits(np.zeros((3, 1))))


def test_refusals_leave_the_buffers_untouched():
    x = R.exact_batch(4, 1)[0][:2]
    n_in = x.shape[1]
    n_out, nf = 50, n_in // 4 + 1
    E = _lib.E_INVALID
    wy, yd = guarded(2 * (n_out + 11))
    we, ed = guarded(2 * (nf + EPAD))
    xd = torch.from_numpy(x).cuda()
    od = torch.full((2,), SENT, dtype=torch.int32, device="cuda")
    sd = torch.full((2,), SENT, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    need = L.tt2_trim_workspace_size(2, n_in, 4)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    for kw in (dict(hop=0), dict(hop=-4), dict(r=0), dict(r=17), dict(hop=2 ** 30, r=2), dict(keep=-1),
               dict(ratio=NAN), dict(ratio=float("inf")), dict(ratio=-0.5), dict(ratio=1.5),
               dict(batch=-1), dict(n_in=-1), dict(n_out=-1), dict(x_ld=n_in - 1), dict(y_ld=n_out - 1),
               dict(energy_ld=nf - 1), dict(y=None), dict(x=None), dict(workspace=None),
               dict(workspace_bytes=need - 1)):
        a = _lib.TrimArgs()
        a.x, a.y, a.out_lens, a.start, a.energy = xd.data_ptr(), yd.data_ptr(), od.data_ptr(), sd.data_ptr(), ed.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        a.x_ld, a.y_ld, a.energy_ld = n_in, n_out + 11, nf + EPAD
        a.batch, a.n_in, a.n_out, a.hop, a.r, a.keep, a.ratio = 2, n_in, n_out, 4, 1, 0, 0.125
        for k, v in kw.items():
            setattr(a, k, v)
        assert L.tt2_trim(ctypes.byref(a), _lib.stream_ptr()) == E, kw
        assert b"tt2_trim" in L.tt2_last_error()
    torch.cuda.synchronize()
    assert untouched(wy) and untouched(we) and untouched(od) and untouched(sd) and bool((ws == 0x5A).all())


RANDOM = [(512, 2, 12 * 2048 + 300, 3), (64, 3, 12 * 384 + 77, 4)]


@pytest.mark.parametrize("hop,r,n_in,seed", RANDOM, ids=["512-2", "64-3"])
def test_a_random_problem(hop, r, n_in, seed):
    """Energies within E[f]; the decision on the kernel's own energies bit for bit; the float64
    decision for every utterance.  The module docstring has the measured worst ratios."""
    x, lens = R.random_problem(hop, r, n_in, seed)
    ratio = np.float32(10.0 ** -3.0)
    n_out = 12 * r * hop                   # six frames: utterance 2 is shorter, the others are cut
    (y, ol, st, en), _ = launch(x, lens, hop, r, 0, ratio, n_out)
    ref = R.reference(x, lens, hop, r, 0, ratio, n_out)
    worst = 0.0
    for b in range(4):
        F = R.n_frames(lens[b], hop)
        E = R.energy_bound(x[b], lens[b], hop, r)
        err = np.abs(en[b, :F].astype(np.float64) - ref[3][b, :F])
        worst = max(worst, float((err / E).max()))
        assert (err <= E).all(), (b, float((err / E).max()))
        assert not en[b, F:].any()
    print(f"hop {hop} r {r}: worst energy error {worst:.4f} of the bound E[f]")
    own = R.reference(x, lens, hop, r, 0, ratio, n_out, energies=en)
    assert ol.tolist() == own[1] and st.tolist() == own[2] and np.array_equal(bits(y), bits(own[0]))
    assert ol.tolist() == ref[1] and st.tolist() == ref[2] and np.array_equal(bits(y), bits(ref[0]))
    assert any(o == n_out for o in ol.tolist()) and any(0 < o < n_out for o in ol.tolist())
