"""Viterbi pitch tracking kernel (tt2_pitch_track) against the numpy references of
tests/_pitch_track_refs.py (GPU), by direct C-ABI calls on hand-built buffers.

Exact problem (_pitch_track_refs.exact_cmnd): d' in eighths, integer positions and parameters in
quarters, so every value of the recurrence is a multiple of 2^-3 below 2^21
(tests/test_pitch_track_refs.py asserts it) and exact in f32 in any order, with or without an fma:
lag, cost and the unrefined f0 must equal the f32 twin bit for bit.  The refined f0 is held to 1e-6
relative of the float64 formula on (a, b, c), as tests/test_gpu_yin_kernels.py derives it.
Everything the kernel must not read is NaN (columns outside the lag range, rows past an
utterance's frames), and every output sits between NaN guard bands.

Planted track and glide: the f32 twin and the float64 reference agree on every lag on the CPU
(asserted in test_pitch_track_refs.py), so a near-tie cannot be what decides, and the kernel's
lags must equal theirs.

Random real-valued problem: with C* the float64 optimum and C(pi) the float64 cost of the
kernel's own path, C(pi) <= C* + E and |cost - C(pi)| <= E for E = 6 N 2^-24 M,
M = N (max(c, C) + max(J (p_max - p_min), W)): no value of the recurrence exceeds M, a frame makes
at most three roundings (the product and two adds; the fma saves one) of relative size 2^-24,
and two paths are compared.

Measured (MI355X): C(pi) - C* was 0 in all nine random utterances (the kernel's path is the float64
optimum); |cost - C(pi)| was 2.2e-7 .. 1.4e-6 at N = 57 and 90 against E = 4.3e-3 .. 1.7e-2, and 0 at
N = 1 against E = 1.3e-6 .. 2.0e-6."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _pitch_track_refs as R  # noqa: E402
from tt2 import _lib  # noqa: E402

GUARD = 64
NAN = float("nan")


def guarded(n):
    whole = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, n):
    return bool(torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[GUARD + n:]).all())


def launch(c, frames, lo, hi, pos, J, W, C, sr=R.SR, rc=False):
    """One tt2_pitch_track call on c [B, t, ld] -> dict of numpy arrays f0, lag [B, t], cost [B]."""
    c = np.ascontiguousarray(c, dtype=np.float32)
    B, t, ld = c.shape
    cd = torch.from_numpy(c).cuda()
    pd = torch.from_numpy(np.ascontiguousarray(pos[:hi + 1], dtype=np.float32)).cuda()
    outs = {"f0": guarded(B * t), "lag": guarded(B * t), "cost": guarded(B)}
    fr = torch.tensor(frames, dtype=torch.int32, device="cuda") if frames is not None else None
    L = _lib.lib()
    need = L.tt2_pitch_track_workspace_size(B, t, lo, hi)
    ww, ws = guarded((need + 3) // 4)
    a = _lib.PitchTrackArgs()
    a.cmnd, a.frames, a.pos = cd.data_ptr(), _lib.ptr(fr), pd.data_ptr()
    a.f0, a.lag, a.cost = (outs[k][0].data_ptr() + 4 * GUARD for k in ("f0", "lag", "cost"))   # (an empty view has none)
    a.workspace, a.workspace_bytes = ww.data_ptr() + 4 * GUARD, need
    a.cmnd_ld, a.batch, a.t, a.tau_min, a.tau_max = ld, B, t, lo, hi
    a.sr, a.jump, a.switch_cost, a.unvoiced = sr, J, W, C
    code = L.tt2_pitch_track(ctypes.byref(a), _lib.stream_ptr())
    if rc:
        return code
    _lib.check(code, "tt2_pitch_track")
    torch.cuda.synchronize()
    for k, (whole, inner) in outs.items():
        assert guards_intact(whole, inner.numel()), f"{k} guard bands"
    assert guards_intact(ww, (need + 3) // 4), "workspace guard bands"
    return {"f0": outs["f0"][1].cpu().numpy().copy().reshape(B, t),
            "lag": outs["lag"][1].view(torch.int32).cpu().numpy().copy().reshape(B, t),
            "cost": outs["cost"][1].cpu().numpy().copy()}


def same_bits(x, y):
    return all(np.array_equal(x[k].view(np.int32), y[k].view(np.int32)) for k in ("f0", "lag", "cost"))


@pytest.mark.parametrize("lo,hi", R.EXACT_RANGES, ids=[f"{a}-{b}" for a, b in R.EXACT_RANGES])
def test_exact_problem(lo, hi):
    pos = R.exact_pos()
    c, clean = R.exact_cmnd(lo, hi), R.exact_cmnd(lo, hi, poison=False)
    assert c.shape[2] > hi + 1
    for J, W, C in R.EXACT_PARAMS:
        out = launch(c, list(R.EXACT_FRAMES), lo, hi, pos, J, W, C)
        for b, n in enumerate(R.EXACT_FRAMES):
            r = R.track(clean[b, :n], lo, hi, pos, J, W, C, dtype=np.float32)
            R.check_outputs(out, b, r, R.EXACT_T)
        assert out["cost"][3] == 0
    again = launch(c, list(R.EXACT_FRAMES), lo, hi, pos, J, W, C)
    assert same_bits(out, again)


def test_frames_above_t_negative_and_null():
    """frames[b] is clamped into [0, t]; a null frames pointer means t everywhere."""
    lo, hi = 36, 340
    pos, clean = R.exact_pos(), R.exact_cmnd(36, 340, poison=False)
    J, W, C = R.EXACT_PARAMS[0]
    out = launch(clean, [R.EXACT_T + 5, -3, 2 ** 31 - 1, -2 ** 31], lo, hi, pos, J, W, C)
    full = launch(clean, None, lo, hi, pos, J, W, C)
    for b, n in enumerate((R.EXACT_T, 0, R.EXACT_T, 0)):
        r = R.track(clean[b, :n], lo, hi, pos, J, W, C, dtype=np.float32)
        R.check_outputs(out, b, r, R.EXACT_T)
        R.check_outputs(full, b, R.track(clean[b], lo, hi, pos, J, W, C, dtype=np.float32), R.EXACT_T)


def test_one_frame_and_no_frame():
    """t = 1: the end rule alone.  t = 0 with a batch: success, cost written as 0."""
    pos = R.exact_pos()
    for lo, hi in R.EXACT_RANGES:
        clean = R.exact_cmnd(lo, hi, poison=False)[:, :1]
        for J, W, C in ((0.25, 0.5, 0.25), (0.25, 0.5, 0.0), (0.0, 0.0, 0.125)):
            out = launch(clean, [1, 1, 0, 1], lo, hi, pos, J, W, C)
            for b, n in enumerate((1, 1, 0, 1)):
                R.check_outputs(out, b, R.track(clean[b, :n], lo, hi, pos, J, W, C, dtype=np.float32), 1)
    out = launch(np.zeros((3, 0, 400), np.float32), [0, 0, 0], 36, 340, pos, 1.0, 0.1, 0.2)
    assert np.array_equal(out["cost"].view(np.int32), np.zeros(3, np.int32))


def test_nan_in_one_utterance_leaves_the_others():
    lo, hi = 36, 340
    pos, clean = R.exact_pos(), R.exact_cmnd(36, 340, poison=False)
    J, W, C = R.EXACT_PARAMS[0]
    ref = launch(clean, list(R.EXACT_FRAMES), lo, hi, pos, J, W, C)
    bad = clean.copy()
    bad[0, 2, lo:hi + 1:3] = np.nan
    bad[0, 5, lo:hi + 1] = np.nan
    bad[0, 7, 200] = np.inf
    out = launch(bad, list(R.EXACT_FRAMES), lo, hi, pos, J, W, C)
    for k in ("f0", "lag"):
        assert np.array_equal(out[k][1:].view(np.int32), ref[k][1:].view(np.int32)), k
    assert np.array_equal(out["cost"][1:].view(np.int32), ref["cost"][1:].view(np.int32))
    lag = out["lag"][0]
    assert np.all((lag == 0) | ((lag >= lo) & (lag <= hi))), lag


def test_planted_track():
    c, lag = R.planted()
    lo, hi = R.PLANT_RANGE
    pos = R.log2_pos()
    r = R.track(c, lo, hi, pos, *R.DEFAULTS, dtype=np.float32)
    out = launch(np.stack([c, c[::-1]]), [R.PLANT_T, R.PLANT_T], lo, hi, pos, *R.DEFAULTS)
    assert np.array_equal(out["lag"][0], r["lag"]) and np.array_equal(out["lag"][0], lag)
    assert np.array_equal(out["lag"][1], lag[::-1])
    E = R.random_bound(R.PLANT_T, 1.5, pos, lo, hi, *R.DEFAULTS)
    assert abs(float(out["cost"][0]) - float(r["cost"])) <= E
    voiced = lag > 0
    assert np.all(out["f0"][0][~voiced] == 0) and np.all(out["f0"][0][voiced] > 0)


@pytest.mark.parametrize("lo,hi,J,W,C", [(37, 339, 1.0, 0.1, 0.2), (1, 511, 0.3, 0.05, 0.45), (100, 227, 4.0, 1.0, 0.3)])
def test_random_problem_within_the_bound(lo, hi, J, W, C):
    frames = [90, 57, 1]
    c, fr = R.random_problem(1000 + lo, 3, 90, frames)
    pos = R.log2_pos()
    out = launch(c, frames, lo, hi, pos, J, W, C)
    again = launch(c, frames, lo, hi, pos, J, W, C)
    assert same_bits(out, again)
    J32, W32, C32 = (float(np.float32(v)) for v in (J, W, C))
    for b, n in enumerate(frames):
        lag = out["lag"][b, :n]
        assert np.all((lag == 0) | ((lag >= lo) & (lag <= hi))) and np.all(out["lag"][b, n:] == -1)
        best = float(R.track(c[b, :n], lo, hi, pos, J, W, C, dtype=np.float64)["cost"])
        own = float(R.path_cost(R.states_of(lag, lo), c[b, :n], lo, hi, pos, J, W, C))
        E = R.random_bound(n, float(c[b, :n, lo:hi + 1].max()), pos, lo, hi, J32, W32, C32)
        print(f"random {lo}-{hi} b={b}: C(pi) - C* = {own - best:.3e}, |cost - C(pi)| = "
              f"{abs(float(out['cost'][b]) - own):.3e}, E = {E:.3e}")
        assert own <= best + E, (b, own, best, E)
        assert abs(float(out["cost"][b]) - own) <= E, (b, out["cost"][b], own, E)


def test_glide_from_the_cpu_cmnd():
    c, truth = R.glide_cmnd()
    lo, hi = R.GLIDE_RANGE
    out = launch(c[None], [R.GLIDE_T], lo, hi, R.log2_pos(), *R.DEFAULTS)
    assert R.glide_tracked_ok(out["lag"][0], truth) == [], out["lag"][0]
    assert np.array_equal(out["lag"][0], R.track(c, lo, hi, R.log2_pos(), *R.DEFAULTS, dtype=np.float32)["lag"])
    assert R.glide_octave_errors(R.select_lags(c, lo, hi), truth) >= 5


def test_ops_wrapper_checks_before_launching():
    from tt2 import ops
    B, T, lo, hi = 2, 5, 37, 339
    c = torch.rand(B, T, hi + 1, device="cuda")
    f0 = torch.empty(B, T, device="cuda")
    lag = torch.empty(B, T, dtype=torch.int32, device="cuda")
    cost = torch.empty(B, device="cuda")
    pos = torch.from_numpy(R.log2_pos()[:hi + 1]).cuda()
    fr = torch.tensor([5, 3], dtype=torch.int32, device="cuda")
    ops.pitch_track(c, fr, f0, lag, cost, lo, hi, R.SR, pos, 1.0, 0.1, 0.2)
    wide = torch.rand(B, T, 512, device="cuda")
    wide[:, :, :hi + 1] = c
    f1, l1, c1 = ops.pitch_track(wide[:, :, :hi + 1], fr, torch.empty_like(f0), torch.empty_like(lag),
                                 torch.empty_like(cost), lo, hi, R.SR, pos, 1.0, 0.1, 0.2)
    torch.cuda.synchronize()
    assert torch.equal(l1, lag) and torch.equal(f1, f0) and torch.equal(c1, cost)
    assert lag[1, 3:].tolist() == [-1, -1]
    bad = [dict(cmnd=c.double()), dict(cmnd=c[:, :, :hi]), dict(cmnd=c.transpose(1, 2)), dict(f0=f0[:1]),
           dict(lag=lag.float()), dict(cost=cost[:1]), dict(pos=pos[:hi]), dict(pos=pos.double()),
           dict(frames=fr[:1]), dict(frames=fr.long()), dict(f0=f0.cpu()), dict(tau_min=0), dict(tau_max=512),
           dict(f0=torch.empty(B, 2 * T, device="cuda")[:, ::2])]
    for kw in bad:
        args = dict(cmnd=c, frames=fr, f0=f0, lag=lag, cost=cost, tau_min=lo, tau_max=hi, sr=R.SR, pos=pos, jump=1.0,
                    switch=0.1, unvoiced=0.2)
        args.update(kw)
        with pytest.raises(_lib.TT2Error):
            ops.pitch_track(**args)
    with pytest.raises(_lib.TT2Error):
        ops.pitch_track(torch.rand(1, _lib.PITCH_TRACK_MAX_FRAMES + 1, 3, device="cuda"), None,
                        torch.empty(1, 4097, device="cuda"), torch.empty(1, 4097, dtype=torch.int32, device="cuda"),
                        cost[:1], 1, 2, R.SR, pos, 1.0, 0.1, 0.2)
