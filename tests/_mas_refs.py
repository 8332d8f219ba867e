"""numpy references for the monotonic alignment search (tt2_align_monotonic), shared by the CPU
and GPU tests.

Definition (include/tt2_capi.h): for scores s [Ty, Tx] and Te = min(Tx, Ty), the path pi with
pi(0) = 0, pi(Ty - 1) = Te - 1 and steps in {0, 1} that maximises sum_n s[n, pi(n)], through
  V[0][0] = s[0][0], V[0][t > 0] = -inf, V[n][t] = s[n][t] + max(V[n-1][t], V[n-1][t-1]),
  move[n][t] = V[n-1][t-1] > V[n-1][t]  (strict: a tie stays), backtrack from (Ty - 1, Te - 1).
Integer scores run in int64 (exact), real ones in float64.  The mutants (a non-strict tie, a free
end point, steps of 2) exist so that the tests of this file can show they are told apart.
"""
import itertools

import numpy as np


def _neg(dtype):
    return -np.inf if np.issubdtype(dtype, np.floating) else -(2 ** 62)


def mas_path(s, Ty, Tx, strict=True, free_end=False, max_step=1):
    """The path [Ty] (int64) of the definition above; an empty array when Ty or Tx is 0."""
    s = np.asarray(s)
    assert s.dtype in (np.int64, np.float64), s.dtype
    Ty, Tx = int(Ty), int(Tx)
    if Ty <= 0 or Tx <= 0:
        return np.zeros(0, np.int64)
    Te = min(Tx, Ty)
    neg = _neg(s.dtype)
    V = np.full(Te, neg, s.dtype)
    V[0] = s[0, 0]
    step = np.zeros((Ty, Te), np.int64)
    for n in range(1, Ty):
        best, mv = V.copy(), np.zeros(Te, np.int64)
        for m in range(1, max_step + 1):
            prev = np.concatenate((np.full(min(m, Te), neg, s.dtype), V[:-m] if m < Te else V[:0]))
            take = prev > best if strict else prev >= best
            best = np.where(take, prev, best)
            mv = np.where(take, m, mv)
        V = s[n, :Te] + best
        V[max_step * n + 1:] = neg   # keys no path can have reached yet
        step[n] = mv
    t = int(np.argmax(V)) if free_end else Te - 1
    path = np.zeros(Ty, np.int64)
    for n in range(Ty - 1, -1, -1):
        path[n] = t
        t -= int(step[n, t])
    return path


def check_path(path, Ty, Tx):
    """None if `path` is a monotone alignment of Ty frames to Tx phonemes, else what is wrong."""
    path = np.asarray(path)
    Ty, Tx = int(Ty), int(Tx)
    if path.shape != (Ty,):
        return f"length {path.shape} for {Ty} frames"
    if Ty == 0:
        return None
    if Tx <= 0:
        return "frames but no phoneme"
    if path[0] != 0:
        return f"starts on {path[0]}"
    if path[-1] != min(Tx, Ty) - 1:
        return f"ends on {path[-1]}, not {min(Tx, Ty) - 1}"
    d = np.diff(path)
    if ((d < 0) | (d > 1)).any():
        return f"step {d[(d < 0) | (d > 1)][0]} at frame {int(np.argmax((d < 0) | (d > 1))) + 1}"
    return None


def durations_of(path, Tk):
    return np.bincount(np.asarray(path, np.int64), minlength=Tk).astype(np.int64)


def path_score(s, path):
    s = np.asarray(s)
    return s[np.arange(len(path)), path].sum()


def all_paths(Ty, Tx):
    """Every monotone path of the definition (small sizes only)."""
    Te = min(Tx, Ty)
    for steps in itertools.product((0, 1), repeat=Ty - 1):
        if sum(steps) == Te - 1:
            yield np.concatenate(([0], np.cumsum(steps))).astype(np.int64)


def brute_force(s, Ty, Tx):
    """The greatest-score path by enumeration.  Among equal scores the definition's backtrack
    prefers to stay at every step from the end, i.e. the greatest path read backwards."""
    best = None
    for p in all_paths(Ty, Tx):
        key = (path_score(s, p), tuple(p[::-1]))
        if best is None or key > best[0]:
            best = (key, p)
    return best[1]
