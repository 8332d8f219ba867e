"""Dynamic time warping kernel (tt2_dtw) against the numpy references of tests/_dtw_refs.py (GPU).

Exact problem: a and b are small integers that differ in one column of [c0, c1) only (a: x_i, b:
y_j, both in {0, 1, 2}); every cost is the integer |x_i - y_j| and every total stays far below
2^24, so total, length and both path arrays must equal the int64 reference bit for bit (such costs
are full of ties, so the tie rule is covered).  Everything the kernel must not read (columns
outside [c0, c1), rows past the lengths, the row padding) is NaN, and the outputs sit between NaN
guard bands.

Random problems: |total - total64| <= 2 gamma total64 with gamma = (Na + Nb + C / 2 + 3) 2^-24:
each f32 cost carries a relative error <= (C / 2 + 3) 2^-24 (C squared differences summed, one
square root), each cell adds one rounding, costs are non-negative and min is monotone, so the
bound follows by induction over the cells; the factor 2 covers the second-order terms.  The path
returned must be a warping path of `length` cells whose float64 cost is <= total64 (1 + 2 gamma).
Length and path are not compared with the reference there (near-ties may flip under rounding).

Measured (MI355X): relative errors of the totals 0 .. 7.9e-7 against bounds of 3.1e-5 .. 1.4e-4.

Shapes: the kernel tiles by 64 columns x 32 rows up to 1024 columns of b and by 128 columns x 16
rows above, and packs move codes 16 rows to a word."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _dtw_refs import check_path, cost_ref, dtw_ref_fast  # noqa: E402
from tt2 import _lib, ops  # noqa: E402

GUARD = 64
U = 2.0 ** -24
# (c0, c1, ld): 13 features (the 16-feature kernel, row padding) and 20 (the 32-feature kernel)
COLS = [(0, 20, 24), (1, 14, 16)]
COL_IDS = ["c0=0", "c0=1"]
SHAPES = [(1, 1), (1, 70), (65, 1), (63, 64), (64, 65), (129, 127), (130, 257),
          (17, 15), (16, 16), (31, 33), (32, 17), (33, 70),          # move-word and row-block edges
          (21, 1024), (20, 1025),                                     # one / two columns per lane
          (2048, 33), (33, 2048), (2048, 2048)]
BATCH = ([40, 0, 70, 5, 64], [66, 30, 0, 130, 64])                    # one launch, ta = 70, tb = 130


def guarded(n, dtype):
    """A [n] tensor of `dtype` (4 bytes) inside a NaN-filled f32 buffer: (whole, interior)."""
    whole = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(dtype)


def guards_intact(whole, n):
    return bool(torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[GUARD + n:]).all())


def pack(seqs, T, ld, c0, c1):
    """[B, T, ld] f32 on the GPU: utterance b's rows < len(seqs[b]) hold seqs[b] in columns [c0, c1);
    everything else is NaN."""
    x = np.full((len(seqs), T, ld), np.nan, np.float32)
    for i, s in enumerate(seqs):
        x[i, :len(s), c0:c1] = s
    return torch.from_numpy(x).cuda()


def launch(a, b, la, lb, c0, c1, want_path=True, lens=True):
    """One tt2_dtw launch with guarded outputs -> (total [B] f32, length [B], path_a, path_b) numpy."""
    B, ta, tb = a.shape[0], a.shape[1], b.shape[1]
    npth = max(0, ta + tb - 1)
    wt, total = guarded(B, torch.float32)
    wl, length = guarded(B, torch.int32)
    wa, pa = guarded(B * npth, torch.int32)
    wb, pb = guarded(B * npth, torch.int32)
    al = torch.tensor(la, dtype=torch.int32, device="cuda") if lens else None
    bl = torch.tensor(lb, dtype=torch.int32, device="cuda") if lens else None
    ops.dtw(a, b, total, length, a_len=al, b_len=bl, cols=(c0, c1),
            path_a=pa.view(B, npth) if want_path else None, path_b=pb.view(B, npth) if want_path else None)
    torch.cuda.synchronize()
    assert guards_intact(wt, B) and guards_intact(wl, B), "total / length guard bands"
    assert guards_intact(wa, B * npth) and guards_intact(wb, B * npth), "path guard bands"
    if not want_path:   # untouched
        assert bool(torch.isnan(wa).all() and torch.isnan(wb).all())
    return (total.cpu().numpy().copy(), length.cpu().numpy().copy(),
            pa.view(B, npth).cpu().numpy().copy(), pb.view(B, npth).cpu().numpy().copy())


def integer_feats(x, c0, c1):
    """Rows whose column c0 + min(2, width - 1) holds x_i; the other columns are the same small
    integers in every row of a and b."""
    w = c1 - c0
    f = np.tile((np.arange(w) % 3).astype(np.float32), (len(x), 1))
    f[:, min(2, w - 1)] = x
    return f


def check_exact(la, lb, ta, tb, c0, c1, ld, seed, lens=True):
    rng = np.random.default_rng(seed)
    xs = [rng.integers(0, 3, n) for n in la]
    ys = [rng.integers(0, 3, n) for n in lb]
    a = pack([integer_feats(x, c0, c1) for x in xs], ta, ld, c0, c1)
    b = pack([integer_feats(y, c0, c1) for y in ys], tb, ld + 4, c0, c1)
    total, length, pa, pb = launch(a, b, la, lb, c0, c1, lens=lens)
    for i, (x, y) in enumerate(zip(xs, ys)):
        if len(x) == 0 or len(y) == 0:
            assert total[i] == 0 and length[i] == 0 and (pa[i] == -1).all() and (pb[i] == -1).all(), i
            continue
        rt, rl, ra, rb = dtw_ref_fast(np.abs(x[:, None] - y[None, :]).astype(np.int64))
        assert rt < 2 ** 24
        assert total[i] == np.float32(rt), (i, total[i], rt)
        assert length[i] == rl, (i, length[i], rl)
        assert np.array_equal(pa[i, :rl], ra) and np.array_equal(pb[i, :rl], rb), i
        assert (pa[i, rl:] == -1).all() and (pb[i, rl:] == -1).all(), i
    return a, b, (total, length, pa, pb)


@pytest.mark.parametrize("c0,c1,ld", COLS, ids=COL_IDS)
@pytest.mark.parametrize("na,nb", SHAPES, ids=[f"{n}x{m}" for n, m in SHAPES])
def test_exact_single(na, nb, c0, c1, ld):
    # rows past the lengths exist (and are NaN) except at the frame limit; odd cases pass no length vectors
    full = max(na, nb) == _lib.DTW_MAX_FRAMES or (na + nb) % 2 == 1
    ta, tb = (na, nb) if full else (na + 3, nb + 2)
    check_exact([na], [nb], ta, tb, c0, c1, ld, seed=na * 7 + nb, lens=not full)


@pytest.mark.parametrize("c0,c1,ld", COLS, ids=COL_IDS)
def test_exact_batch_no_path_and_repeat(c0, c1, ld):
    la, lb = BATCH
    a, b, first = check_exact(la, lb, 70, 130, c0, c1, ld, seed=5)
    # clamping: lengths beyond ta / tb and below 0 behave as ta / tb and 0
    la2, lb2 = list(la), list(lb)
    la2[2], lb2[3], la2[1] = 1000, 131, -4
    again = launch(a, b, la2, lb2, c0, c1)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)          # and a second launch repeats the first bit for bit
    nop = launch(a, b, la, lb, c0, c1, want_path=False)   # no workspace, no move bits
    assert np.array_equal(nop[0].view(np.int32), first[0].view(np.int32)) and np.array_equal(nop[1], first[1])


def test_zero_frames_is_a_written_no_op():
    a = torch.full((2, 0, 16), float("nan"), device="cuda")
    b = torch.full((2, 9, 16), float("nan"), device="cuda")
    total, length, pa, pb = launch(a, b, [0, 0], [9, 4], 1, 14)
    assert (total == 0).all() and (length == 0).all() and (pa == -1).all() and (pb == -1).all()
    total, length, _, _ = launch(b, a, [9, 4], [0, 0], 1, 14, want_path=False)
    assert (total == 0).all() and (length == 0).all()
    e = torch.empty(0, 5, 16, device="cuda")
    ops.dtw(e, e, torch.empty(0, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda"), cols=(1, 14))


def test_identity_and_repeated_frames():
    rng = np.random.default_rng(11)
    n = 130
    x = rng.normal(size=(n, 13)).astype(np.float32)
    a = pack([x], n, 16, 1, 14)
    total, length, pa, pb = launch(a, a.clone(), [n], [n], 1, 14)
    assert total[0] == 0 and length[0] == n
    assert np.array_equal(pa[0, :n], np.arange(n)) and np.array_equal(pb[0, :n], np.arange(n))
    idx = np.repeat(np.arange(n), np.where(np.arange(n) % 3 == 2, 2, 1))   # every third frame twice
    b = pack([x[idx]], len(idx), 16, 1, 14)
    total, length, pa, pb = launch(a, b, [n], [len(idx)], 1, 14)
    assert total[0] == 0 and length[0] == len(idx)
    assert np.array_equal(pa[0, :len(idx)], idx) and np.array_equal(pb[0, :len(idx)], np.arange(len(idx)))


def test_perfect_squares_are_exact():
    """3-4-5 and 5-12-13 triangles: an IEEE square root returns the integer."""
    a = np.zeros((3, 2), np.float32)
    b = np.array([[3, 4], [5, 12], [8, 15]], np.float32)
    total, length, pa, pb = launch(pack([a], 3, 4, 0, 2), pack([b], 3, 4, 0, 2), [3], [3], 0, 2)
    assert total[0] == 5 + 13 + 17 and length[0] == 3


RANDOM = [("gauss", 63, 64, 13), ("gauss", 129, 127, 32), ("gauss", 130, 257, 13), ("gauss", 40, 1100, 32),
          ("warp", 200, 257, 13), ("warp", 150, 90, 32), ("warp", 100, 1100, 13)]


@pytest.mark.parametrize("kind,na,nb,C", RANDOM, ids=[f"{k}-{n}x{m}-C{c}" for k, n, m, c in RANDOM])
def test_random_within_the_f32_bound(kind, na, nb, C):
    rng = np.random.default_rng(na + nb + C)
    x = rng.normal(size=(na, C)).astype(np.float32)
    if kind == "gauss":
        y = rng.normal(size=(nb, C)).astype(np.float32)
    else:   # b: a time-warped noisy copy of a, so the path wanders
        t = np.sort(rng.uniform(0, na - 1, nb))
        y = (x[np.rint(t).astype(int)] + 0.05 * rng.normal(size=(nb, C))).astype(np.float32)
    c0 = 1 if C < 32 else 0
    a, b = pack([x], na + 1, c0 + C + 3, c0, c0 + C), pack([y], nb + 2, c0 + C, c0, c0 + C)
    total, length, pa, pb = launch(a, b, [na], [nb], c0, c0 + C)
    c64 = cost_ref(x, y, 0, C).astype(np.float64)
    t64 = float(dtw_ref_fast(c64)[0])
    gamma = (na + nb + C / 2 + 3) * U
    L = int(length[0])
    print(f"total {total[0]:.6f} ref {t64:.6f} rel err {abs(total[0] - t64) / t64:.3e} bound {2 * gamma:.3e}")
    assert abs(float(total[0]) - t64) <= 2 * gamma * t64
    assert check_path(pa[0, :L], pb[0, :L], na, nb, L) is None, check_path(pa[0, :L], pb[0, :L], na, nb, L)
    assert (pa[0, L:] == -1).all() and (pb[0, L:] == -1).all()
    assert c64[pa[0, :L], pb[0, :L]].sum() <= t64 * (1 + 2 * gamma)
    nop = launch(a, b, [na], [nb], c0, c0 + C, want_path=False)
    assert nop[0].view(np.int32)[0] == total.view(np.int32)[0] and nop[1][0] == L


def test_ops_dtw_refuses_bad_tensors():
    f = torch.zeros(2, 8, 16, device="cuda")
    t, l = torch.zeros(2, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.TT2Error):
        ops.dtw(f.half(), f, t, l)
    with pytest.raises(_lib.TT2Error):
        ops.dtw(f.transpose(1, 2), f, t, l)
    with pytest.raises(_lib.TT2Error):
        ops.dtw(f, f, t[:1], l)
    with pytest.raises(_lib.TT2Error):
        ops.dtw(f, f, t, l.float())
    with pytest.raises(_lib.TT2Error):
        ops.dtw(f, f, t, l, path_a=torch.zeros(2, 15, dtype=torch.int32, device="cuda"))
    with pytest.raises(_lib.TT2Error):
        ops.dtw(f, f, t.cpu(), l)
    with pytest.raises(_lib.TT2Error):
        ops.dtw(f, f, t, l, cols=(0, 17))
    with pytest.raises(_lib.TT2Error):
        ops.dtw(f, torch.zeros(2, _lib.DTW_MAX_FRAMES + 1, 16, device="cuda"), t, l)
