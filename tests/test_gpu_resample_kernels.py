"""Polyphase resampling kernel (tt2_resample) against the float64 reference of
tests/_resample_refs.py (GPU), by direct C-ABI calls on hand-built buffers.

Every buffer is NaN-filled and sits between NaN guard bands; x is NaN at and past each utterance's
length and in its pad columns, so a sample read where none may be read turns an output into NaN;
the pad columns of x, y and the bank have different widths (5, 11, 3), so a leading dimension taken
from the wrong buffer shows.  After a launch the guards and y's pad columns must still be NaN.

Exact problems: banks of integers in [-8, 8] (one of them a selector, a single 1 per row at a
row-dependent tap) and samples in [-64, 64]: every product and partial sum is an integer below
2^24 (tests/test_resample_refs.py asserts it), so the f32 result is defined bit for bit in any
order.  Random problems with the default banks: each output within E[n] = (K + 2) 2^-24
sum_k |bank x| of the float64 reference fed the same f32 bank (_resample_refs' docstring derives
the bound).

Measured (MI355X): the worst error over each random problem's outputs is 0.054 (48000), 0.072
(44100), 0.102 (24000), 0.102 (16000), 0.087 (22050 -> 16000) and 0.032 (96000) of E[n]."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _resample_refs as R  # noqa: E402
from tt2 import _lib  # noqa: E402

GUARD = 64
XPAD, YPAD, BPAD = 5, 11, 3
NAN = float("nan")
bits = R.bits


def guarded(n):
    whole = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, n):
    return bool(torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[GUARD + n:]).all())


def eff_lens(lens, B, n_in):
    return [n_in] * B if lens is None else [min(max(int(v), 0), n_in) for v in lens]


def launch(x, lens, bank, up, down, half, n_out, want_out_lens=True, expect=0, x_null=False):
    """One tt2_resample call.  x [B, n_in] and bank [up, K] numpy; lens a list (as passed to the
    kernel, unclamped) or None.  Returns (y [B, n_out] numpy, out_lens list or None, the out_lens
    buffer as the f32 it was poisoned as)."""
    x = np.asarray(x, dtype=np.float32)
    B, n_in = x.shape
    K = 2 * half + 1
    x_ld, y_ld, b_ld = n_in + XPAD, n_out + YPAD, K + BPAD
    el = eff_lens(lens, B, n_in)
    xh = np.full((B, x_ld), np.nan, dtype=np.float32)
    for b in range(B):
        xh[b, :el[b]] = x[b, :el[b]]
    bh = np.full((up, b_ld), np.nan, dtype=np.float32)
    bh[:, :K] = np.asarray(bank, dtype=np.float32)[:, :K]
    wx, xd = guarded(B * x_ld)
    xd.copy_(torch.from_numpy(xh.reshape(-1)))
    wb, bd = guarded(up * b_ld)
    bd.copy_(torch.from_numpy(bh.reshape(-1)))
    wy, yd = guarded(B * y_ld)
    wo, od = guarded(B)
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda") if lens is not None else None
    a = _lib.ResampleArgs()
    a.x, a.lens, a.bank, a.y = (None if x_null else xd.data_ptr()), _lib.ptr(ld), bd.data_ptr(), yd.data_ptr()
    a.out_lens = od.data_ptr() if want_out_lens else None
    a.x_ld, a.y_ld, a.bank_ld = x_ld, y_ld, b_ld
    a.batch, a.n_in, a.n_out, a.up, a.down, a.half = B, n_in, n_out, up, down, half
    rc = _lib.lib().tt2_resample(ctypes.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.lib().tt2_last_error())
    assert guards_intact(wy, B * y_ld) and guards_intact(wo, B) and guards_intact(wx, B * x_ld), "guard bands"
    yh = yd.cpu().numpy().copy().reshape(B, y_ld)
    assert np.isnan(yh[:, n_out:]).all(), "y written at or past n_out"
    ol = od.view(torch.int32).cpu().numpy().copy()
    return yh[:, :n_out], ([int(v) for v in ol] if want_out_lens else None), od.cpu().numpy().copy()


def reference_rows(x, lens, bank, up, down, half, n_out):
    """(y [B, n_out] float64, out_lens) of the definition, zeros past each out_b."""
    B, n_in = x.shape
    el = eff_lens(lens, B, n_in)
    y = np.zeros((B, n_out))
    outs = []
    for b in range(B):
        ob = min(R.out_len(el[b], up, down), n_out)
        outs.append(ob)
        if ob:
            y[b, :ob] = R.resample(x[b], el[b], bank, up, down, half, np.arange(ob))
    return y, outs


@pytest.mark.parametrize("up,down,half", R.EXACT_TRIPLES, ids=[f"{a}-{b}-{c}" for a, b, c in R.EXACT_TRIPLES])
def test_exact_integer_problems(up, down, half):
    B, flip = 5, 0
    for n_in in R.exact_n_ins(half):
        full = R.out_len(n_in, up, down)
        rag = R.ragged_lens(B, n_in, seed=n_in)
        lens = [n_in + 7, -2, rag[2], rag[3], n_in]          # clamped to n_in and 0, ragged, exact
        x = R.int_signal(B, n_in, seed=3 + n_in)
        for n_out in sorted({max(full - 3, 1), full, full + 37}):
            for selector in (False, True):
                bank = R.int_bank(up, half, seed=up + half, selector=selector)
                assert R.is_exact(bank, x)
                flip += 1
                want_ol = bool(flip % 3)                       # both given and null, across both banks
                y, ol, raw = launch(x, lens, bank, up, down, half, n_out, want_out_lens=want_ol)
                ref, outs = reference_rows(x, lens, bank, up, down, half, n_out)
                assert np.array_equal(bits(y), bits(ref)), (n_in, n_out, selector)
                if want_ol:
                    assert ol == outs, (n_in, n_out)
                else:
                    assert np.isnan(raw).all()
                assert outs[1] == 0 and not y[1].any()
    # lens null: every utterance is n_in long
    x = R.int_signal(2, 1000, seed=11)
    bank = R.int_bank(up, half, seed=5)
    n_out = R.out_len(1000, up, down) + 2
    y, ol, _ = launch(x, None, bank, up, down, half, n_out)
    ref, outs = reference_rows(x, None, bank, up, down, half, n_out)
    assert np.array_equal(bits(y), bits(ref)) and ol == outs == [n_out - 2] * 2


@pytest.mark.parametrize("up,down,half", [(3, 5, 4), (5, 7, 2), (1, 3, 40)], ids=["3-5-4", "5-7-2", "1-3-40"])
def test_exact_problems_with_an_odd_period_stride(up, down, half):
    """Triples beyond the nine above: an odd `down` stored as one contiguous span with an odd number
    of period groups per tile leaves a thread's windows at alternating parities, the one case in
    which the kernel reads its samples singly instead of in aligned pairs."""
    for n_in in (2 * half + 1, 1000, 5003):
        x = R.int_signal(3, n_in, seed=n_in)
        lens = [n_in, 0, n_in // 2 + 1]
        for selector in (False, True):
            bank = R.int_bank(up, half, seed=7, selector=selector)
            n_out = R.out_len(n_in, up, down) + 5
            y, ol, _ = launch(x, lens, bank, up, down, half, n_out)
            ref, outs = reference_rows(x, lens, bank, up, down, half, n_out)
            assert np.array_equal(bits(y), bits(ref)) and ol == outs, (n_in, selector)


def test_zero_input_length_zero_fills():
    """n_in = 0 with n_out > 0 launches, writes zeros and out_lens 0; x may be null."""
    bank = R.int_bank(3, 4, seed=1)
    for x_null in (False, True):
        y, ol, _ = launch(np.zeros((3, 0), dtype=np.float32), None, bank, 3, 2, 4, 700, x_null=x_null)
        assert ol == [0, 0, 0] and np.array_equal(bits(y), bits(np.zeros((3, 700))))


def test_64_bit_indexing():
    """(1024, 1023, 1) on 2^21 + 4096 samples: n * down crosses 2^31 near n = 2 099 203, and row 1
    of x and of y starts more than 2^31 bytes into its buffer."""
    up, down, half = 1024, 1023, 1
    n_in = (1 << 21) + 4096
    n_out = R.out_len(n_in, up, down)
    ld = (1 << 29) + 24
    lens = [n_in, n_in - 1234]          # both rows reach past the crossing
    rng = np.random.default_rng(9)
    xh = rng.integers(-64, 65, size=(2, n_in)).astype(np.float32)
    bank = R.int_bank(up, half, seed=2)
    x = torch.empty(ld + n_in, dtype=torch.float32, device="cuda")
    y = torch.empty(ld + n_out, dtype=torch.float32, device="cuda")
    for b in range(2):
        x[b * ld:b * ld + n_in] = torch.from_numpy(xh[b]).cuda()
        x[b * ld + lens[b]:b * ld + n_in] = NAN
    y[:n_out] = NAN
    y[ld:ld + n_out] = NAN
    bd = torch.from_numpy(bank).cuda()
    od = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    a = _lib.ResampleArgs()
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    a.x, a.lens, a.bank, a.y, a.out_lens = x.data_ptr(), lens_d.data_ptr(), bd.data_ptr(), y.data_ptr(), od.data_ptr()
    a.x_ld, a.y_ld, a.bank_ld = ld, ld, 3
    a.batch, a.n_in, a.n_out, a.up, a.down, a.half = 2, n_in, n_out, up, down, half
    _lib.check(_lib.lib().tt2_resample(ctypes.byref(a), _lib.stream_ptr()), "tt2_resample")
    torch.cuda.synchronize()
    outs = [R.out_len(n, up, down) for n in lens]
    assert od.tolist() == outs and outs[0] == n_out
    cross = (1 << 31) // down
    assert (cross - 1) * down < (1 << 31) < (cross + 2) * down and cross + 2048 < min(outs)
    for b in range(2):
        got = y[b * ld:b * ld + n_out].cpu().numpy()
        for lo in (0, cross - 2048, outs[b] - 4096):
            idx = np.arange(lo, lo + 4096)
            ref = R.resample(xh[b], lens[b], bank, up, down, half, idx)
            assert np.array_equal(bits(got[idx]), bits(ref)), (b, lo)
        assert not got[outs[b]:].any() and not np.isnan(got).any()
    del x, y
    torch.cuda.empty_cache()


def random_problem(pair, seed):
    up, down, half, taps = R.design(*pair)
    bank = taps.astype(np.float32)
    n_in = 3001
    x = (0.3 * np.random.default_rng(seed).normal(size=(3, n_in))).astype(np.float32)
    return up, down, half, bank, x, [n_in, 1777, 2 * half]


@pytest.mark.parametrize("pair", R.PAIRS, ids=[f"{a}-{b}" for a, b in R.PAIRS])
def test_random_problems_with_the_default_banks(pair):
    """Every output within E[n]; the module docstring has the measured worst ratios."""
    up, down, half, bank, x, lens = random_problem(pair, seed=pair[0] % 97)
    n_out = R.out_len(x.shape[1], up, down) + 9
    y, ol, _ = launch(x, lens, bank, up, down, half, n_out)
    ref, outs = reference_rows(x, lens, bank, up, down, half, n_out)
    assert ol == outs
    worst = 0.0
    for b in range(3):
        E = R.bound(x[b], lens[b], bank, up, down, half, np.arange(outs[b]))
        err = np.abs(y[b, :outs[b]].astype(np.float64) - ref[b, :outs[b]])
        worst = max(worst, float((err / np.maximum(E, 1e-300)).max()))
        assert (err <= E).all(), (b, float((err / np.maximum(E, 1e-300)).max()))
        assert not y[b, outs[b]:].any()
    print(f"{pair}: worst error {worst:.3f} of the bound E[n]")
    again, ol2, _ = launch(x, lens, bank, up, down, half, n_out)
    assert np.array_equal(bits(y), bits(again)) and ol2 == ol          # run to run


@pytest.mark.parametrize("pair", [(48000, 22050), (44100, 22050), (16000, 22050)], ids=["48k", "44k1", "16k"])
def test_an_utterance_alone_and_inside_a_batch(pair):
    """The same utterance as a batch of one, and as row 3 of a batch of five with a longer n_in,
    a larger n_out and other leading dimensions: identical bits."""
    up, down, half, bank, x, _ = random_problem(pair, seed=5)
    n = 2500
    alone, ol, _ = launch(x[:1, :n], None, bank, up, down, half, R.out_len(n, up, down))
    big = (0.3 * np.random.default_rng(6).normal(size=(5, 3001))).astype(np.float32)
    big[3, :n] = x[0, :n]
    n_out = R.out_len(3001, up, down) + 500
    batch, ol5, _ = launch(big, [3001, 100, 0, n, 2999], bank, up, down, half, n_out)
    assert ol5[3] == ol[0] == R.out_len(n, up, down)
    assert np.array_equal(bits(batch[3, :ol[0]]), bits(alone[0])) and not batch[3, ol[0]:].any()


def test_refusals_leave_the_buffers_untouched():
    bank = R.int_bank(3, 4, seed=1)
    x = R.int_signal(2, 100, seed=2)
    E = _lib.E_INVALID
    n_out = 150
    K = 9
    wy, yd = guarded(2 * (n_out + YPAD))
    xd = torch.from_numpy(x).cuda()
    bd = torch.from_numpy(bank).cuda()
    od = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    for kw in (dict(up=0), dict(down=0), dict(up=1025), dict(half=-1), dict(half=128), dict(batch=-1), dict(n_in=-1),
               dict(n_out=-1), dict(x_ld=99), dict(y_ld=n_out - 1), dict(bank_ld=K - 1), dict(bank=None), dict(y=None),
               dict(x=None)):
        a = _lib.ResampleArgs()
        a.x, a.bank, a.y, a.out_lens = xd.data_ptr(), bd.data_ptr(), yd.data_ptr(), od.data_ptr()
        a.x_ld, a.y_ld, a.bank_ld = 100, n_out + YPAD, K
        a.batch, a.n_in, a.n_out, a.up, a.down, a.half = 2, 100, n_out, 3, 2, 4
        for k, v in kw.items():
            setattr(a, k, v)
        assert _lib.lib().tt2_resample(ctypes.byref(a), _lib.stream_ptr()) == E, kw
        assert b"tt2_resample" in _lib.lib().tt2_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(wy).all()) and od.tolist() == [-7, -7]
