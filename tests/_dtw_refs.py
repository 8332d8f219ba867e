"""numpy references for dynamic time warping (tt2_dtw) and MCD-DTW (tt2.evaluate).

The definition (include/tt2_capi.h): D[0][0] = c[0][0]; otherwise D[i][j] = c[i][j] + the least D
among the existing predecessors (i-1, j-1), (i-1, j), (i, j-1), a tie going to the diagonal, then
up, then left; the path follows the chosen predecessors back from the end cell.  Integer costs are
summed in int64 (exact), anything else in float64.
"""
import math

import numpy as np

DIAG, UP, LEFT = 0, 1, 2


def _acc_dtype(c):
    return np.int64 if np.issubdtype(np.asarray(c).dtype, np.integer) else np.float64


def _big(dt):
    return np.iinfo(np.int64).max // 4 if dt == np.int64 else np.inf


def _walk(move, n, m, free_end_at=None):
    i, j = (n - 1, m - 1) if free_end_at is None else free_end_at
    pa, pb = [i], [j]
    while i or j:
        mv = move[i, j]
        if mv != LEFT:
            i -= 1
        if mv != UP:
            j -= 1
        pa.append(i)
        pb.append(j)
    return np.array(pa[::-1], np.int64), np.array(pb[::-1], np.int64)


def dtw_ref(c, order=(DIAG, UP, LEFT), allow_left=True, free_end=False, zero_start=False):
    """The definition as a plain double loop -> (total, length, path_a, path_b).  The keywords make
    the mutants below; the defaults are the definition."""
    c = np.asarray(c)
    dt = _acc_dtype(c)
    n, m = c.shape
    D = np.zeros((n, m), dt)
    move = np.zeros((n, m), np.int8)
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                D[0, 0] = 0 if zero_start else c[0, 0]
                continue
            cand = {}
            if i and j:
                cand[DIAG] = D[i - 1, j - 1]
            if i:
                cand[UP] = D[i - 1, j]
            if j and (allow_left or not i):
                cand[LEFT] = D[i, j - 1]
            best = min(cand.values())
            mv = next(o for o in order if o in cand and cand[o] == best)
            move[i, j] = mv
            D[i, j] = c[i, j] + best
    end = None
    if free_end:   # ends on the cheapest cell of the last row
        end = (n - 1, int(np.argmin(D[n - 1])))
    pa, pb = _walk(move, n, m, end)
    return D[pa[-1], pb[-1]], len(pa), pa, pb


def dtw_ref_fast(c):
    """dtw_ref vectorised over anti-diagonals (cells with i + j = d depend only on d - 1, d - 2)."""
    c = np.asarray(c)
    dt = _acc_dtype(c)
    n, m = c.shape
    big = _big(dt)
    D = np.full((n + 1, m + 1), big, dt)   # D[i + 1][j + 1]; the border stands for "no predecessor"
    move = np.zeros((n, m), np.int8)
    D[1, 1] = c[0, 0]
    for d in range(1, n + m - 1):
        i = np.arange(max(0, d - m + 1), min(n - 1, d) + 1)
        j = d - i
        dg, up, lf = D[i, j], D[i, j + 1], D[i + 1, j]
        is_dg = (dg <= up) & (dg <= lf)
        is_up = ~is_dg & (up <= lf)
        best = np.where(is_dg, dg, np.where(is_up, up, lf))
        move[i, j] = np.where(is_dg, DIAG, np.where(is_up, UP, LEFT))
        D[i + 1, j + 1] = c[i, j] + best
    pa, pb = _walk(move, n, m)
    return D[n, m], len(pa), pa, pb


def check_path(pa, pb, n, m, length=None):
    """None if (pa, pb) is a warping path of an n x m problem, else what is wrong."""
    pa, pb = np.asarray(pa, np.int64), np.asarray(pb, np.int64)
    if len(pa) != len(pb) or len(pa) == 0:
        return f"path arrays of {len(pa)} and {len(pb)} entries"
    if length is not None and len(pa) != length:
        return f"path has {len(pa)} cells, length says {length}"
    if (pa[0], pb[0]) != (0, 0):
        return f"starts at {(pa[0], pb[0])}"
    if (pa[-1], pb[-1]) != (n - 1, m - 1):
        return f"ends at {(pa[-1], pb[-1])}, not {(n - 1, m - 1)}"
    da, db = np.diff(pa), np.diff(pb)
    bad = np.nonzero(~(((da == 1) & (db == 1)) | ((da == 1) & (db == 0)) | ((da == 0) & (db == 1))))[0]
    if len(bad):
        k = int(bad[0])
        return f"step {k}: {(pa[k], pb[k])} -> {(pa[k + 1], pb[k + 1])}"
    return None


def cost_ref(a, b, c0, c1):
    """c[i][j] = ||a[i, c0:c1] - b[j, c0:c1]|| in float64 (int64 when every cost is an integer)."""
    a, b = np.asarray(a, np.float64)[:, c0:c1], np.asarray(b, np.float64)[:, c0:c1]
    c = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
    r = np.rint(c)
    return r.astype(np.int64) if np.array_equal(r, c) else c


# ---- mutants: each must differ from dtw_ref on the integer problem set
def mutant_up_first(c):
    return dtw_ref(c, order=(UP, DIAG, LEFT))


def mutant_left_first(c):
    return dtw_ref(c, order=(LEFT, DIAG, UP))


def mutant_no_left(c):
    return dtw_ref(c, allow_left=False)


def mutant_free_end(c):
    return dtw_ref(c, free_end=True)


def mutant_zero_start(c):
    return dtw_ref(c, zero_start=True)


MUTANTS = {"up before diagonal": mutant_up_first, "left first": mutant_left_first, "no left move": mutant_no_left,
           "free end point": mutant_free_end, "D[0][0] = 0": mutant_zero_start}


def same(r, s):
    return r[0] == s[0] and r[1] == s[1] and np.array_equal(r[2], s[2]) and np.array_equal(r[3], s[3])


def integer_problems(sizes=((5, 7), (9, 4), (12, 12)), per_size=40, seed=0):
    """Costs |x_i - y_j| with x, y in {0, 1, 2}: full of ties."""
    rng = np.random.default_rng(seed)
    out = []
    for n, m in sizes:
        for _ in range(per_size):
            x, y = rng.integers(0, 3, n), rng.integers(0, 3, m)
            out.append(np.abs(x[:, None] - y[None, :]).astype(np.int64))
    return out


# ---- MCD
def dct_ref(n_mels=80, n_coef=13):
    """Rows 0..n_coef of the orthonormal DCT-II, float64."""
    k = np.arange(n_coef + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    w = np.cos(np.pi * (m + 0.5) * k / n_mels) * math.sqrt(2.0 / n_mels)
    w[0] = math.sqrt(1.0 / n_mels)
    return w


MCD_SCALE = 10.0 / math.log(10.0) * math.sqrt(2.0)


def mcd_ref(cep_hyp, cep_ref, n_coef=13):
    """(mcd dB, total, length) of two cepstral sequences [T, >= n_coef + 1] over columns 1..n_coef."""
    if len(cep_hyp) == 0 or len(cep_ref) == 0:
        return float("nan"), 0.0, 0
    total, length, _, _ = dtw_ref_fast(cost_ref(cep_hyp, cep_ref, 1, n_coef + 1).astype(np.float64))
    return MCD_SCALE * total / length, total, length
