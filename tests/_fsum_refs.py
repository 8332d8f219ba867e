"""numpy references for the forward-sum alignment loss (tt2_forward_sum_fwd / _bwd / _path), the
problem sets of its GPU tests and the judge that holds an implementation to them; shared by the CPU
and GPU tests.

Definition (include/tt2_capi.h): for scores s [Ty, Tx], ls = log_softmax over the Tx phonemes, and
the monotone paths of tt2_align_monotonic (pi(0) = 0, pi(Ty - 1) = Te - 1, steps in {0, 1}),
  Z = sum_pi prod_n exp ls[n, pi(n)], loss = -ln Z, gamma[n, t] = P(pi(n) = t),
  dscores = grad_loss * (exp ls - gamma).
`forward_sum` is the one reference, parametrised by dtype and `renorm`: float64 is the truth,
float32 with the row maximum subtracted after every row (the offsets summed in float64) is the
yardstick whose own distance from the truth sets the bar, and float32 without renormalisation is
the plain log-space recurrence the bar is built to reject.  Its other parameters are the mutants.

The bar (`judge_soft`): per utterance, |loss - loss64| <= max(4 e_loss, 2 ulp32(loss64)), and for
every row of gamma and dscores max |x - x64| <= max(4 e, 2 ulp32(|grad_loss|)) (grad_loss = 1 for
gamma, whose entries are at most 1), where e is the float32 yardstick's greatest distance from
float64 over the whole utterance -- pooled, since a single row's float32 error can be 0 by luck.
The padding (n >= Ty or t >= Tx) must be +0 bit for bit.  Nothing is judged against the output of
the code under test.
"""
import math

import numpy as np

from _mas_refs import check_path, durations_of, mas_path, path_score

SHAPES = [(1, 1), (5, 5), (3, 5), (37, 7), (33, 64), (65, 65), (257, 129), (70, 512), (4096, 3), (1030, 130)]
LARGEST_RANDOM = (1030, 130)
MARGIN = 4.0


def clamp(v, hi):
    return max(0, min(int(v), hi))


def lengths(tq, tk):
    """q_len / key_len of the B = 4 utterances: above the size, inside it, 0 and negative."""
    inq, ink = max(1, (2 * tq + 2) // 3), max(1, (3 * tk + 3) // 4)
    return np.array([tq + 3, inq, 0, tq], np.int32), np.array([ink, tk + 2, tk, -1], np.int32)


def _shift(a, k, neg):
    return np.concatenate((np.full(min(k, len(a)), neg, a.dtype), a[:-k] if k < len(a) else a[:0]))


def forward_sum(s, Ty, Tx, dtype=np.float64, renorm=True, max_step=1, free_end=False, free_start=False,
                te_delta=0, semiring="sum", drop_offsets=False):
    """loss, gamma [Ty, Tx], P = exp ls, grad = P - gamma, lse [Ty] and ls of one utterance."""
    Ty, Tx = int(Ty), int(Tx)
    if Ty <= 0 or Tx <= 0:
        z = np.zeros((max(Ty, 0), max(Tx, 0)), dtype)
        return dict(loss=0.0, gamma=z, P=z.copy(), grad=z.copy(), lse=np.zeros(max(Ty, 0), dtype), ls=z.copy())
    s = np.asarray(s)[:Ty, :Tx].astype(dtype)
    m = s.max(1, keepdims=True)
    lse = m + np.log(np.exp(s - m).sum(1, keepdims=True, dtype=dtype))
    ls = (s - lse).astype(dtype)
    Te = min(max(min(Tx, Ty) + te_delta, 1), Tx)
    neg = dtype(-np.inf)
    add = np.logaddexp if semiring == "sum" else np.maximum
    alpha = np.full((Ty, Te), neg, dtype)
    beta = np.full((Ty, Te), neg, dtype)
    off = 0.0                               # float64, as the offsets are summed
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a = np.full(Te, neg, dtype)
        a[0] = ls[0, 0]
        if free_start:
            a[:] = ls[0, :Te]
        for n in range(Ty):
            if n:
                acc = a.copy()
                for k in range(1, max_step + 1):
                    acc = add(acc, _shift(a, k, neg))
                a = (ls[n, :Te] + acc).astype(dtype)
            if renorm:
                mx = a.max()
                a = (a - mx).astype(dtype)
                off += float(mx)
            alpha[n] = a
        end = alpha[Ty - 1, Te - 1]
        if free_end:
            end = np.logaddexp.reduce(alpha[Ty - 1].astype(np.float64)).astype(dtype)
        lnz = float(end) + (off if renorm and not drop_offsets else 0.0)
        b = np.full(Te, neg, dtype)
        b[Te - 1] = 0
        if free_end:
            b[:] = 0
        beta[Ty - 1] = b
        for n in range(Ty - 2, -1, -1):
            x = (ls[n + 1, :Te] + b).astype(dtype)
            acc = x.copy()
            for k in range(1, max_step + 1):
                acc = add(acc, _shift(x[::-1], k, neg)[::-1])
            b = acc.astype(dtype)
            if renorm:
                b = (b - b.max()).astype(dtype)
            beta[n] = b
        ab = (alpha + beta).astype(dtype)
        if renorm:
            e = np.exp(ab - ab.max(1, keepdims=True)).astype(dtype)
            g = (e / e.sum(1, keepdims=True, dtype=dtype)).astype(dtype)
        else:
            g = np.exp(ab - dtype(lnz)).astype(dtype)
    gamma = np.zeros((Ty, Tx), dtype)
    gamma[:, :Te] = np.nan_to_num(g, nan=0.0) if semiring != "sum" else g
    P = np.exp(ls).astype(dtype)
    loss = dtype(-lnz)
    return dict(loss=float(loss), gamma=gamma, P=P, grad=(P - gamma).astype(dtype), lse=lse[:, 0], ls=ls)


def hard(s, Ty, Tx, strict=True):
    """path [Ty] (float64 MAS over the raw scores), durations [Tx] and logp of one utterance."""
    Ty, Tx = int(Ty), int(Tx)
    if Ty <= 0 or Tx <= 0:
        return np.zeros(0, np.int64), np.zeros(max(Tx, 0), np.int64), 0.0
    s64 = np.asarray(s)[:Ty, :Tx].astype(np.float64)
    path = mas_path(s64, Ty, Tx, strict=strict)
    return path, durations_of(path, Tx), logp_of(s64, path)


def logp_of(s, path, dtype=np.float64):
    s = np.asarray(s).astype(dtype)
    m = s.max(1)
    lse = m + np.log(np.exp(s - m[:, None]).sum(1, dtype=dtype))
    return float((s[np.arange(len(path)), path] - lse).astype(dtype).sum(dtype=dtype) / dtype(len(path)))


def reduce_loss(loss, Tx, reduction):
    """The three reductions of forward_sum_loss over per-utterance losses and clamped Tx_b."""
    loss = np.asarray(loss, np.float64)
    if reduction == "none":
        return loss
    if reduction == "sum":
        return loss.sum()
    return (loss / np.maximum(np.asarray(Tx, np.float64), 1.0)).sum() / max(len(loss), 1)


def closed_form(Ty, Tx):
    """Constant scores, Ty >= Tx: gamma = C(n, t) C(Ty-1-n, Tx-1-t) / C(Ty-1, Tx-1) and
    loss = Ty ln Tx - ln C(Ty-1, Tx-1)."""
    c = math.comb(Ty - 1, Tx - 1)
    g = np.array([[math.comb(n, t) * math.comb(Ty - 1 - n, Tx - 1 - t) / c for t in range(Tx)] for n in range(Ty)])
    return Ty * math.log(Tx) - math.log(c), g


# ------------------------------------------------------------------------------------ problem sets
def planted_path(rng, Ty, Tx):
    Te = min(Tx, Ty)
    steps = np.zeros(Ty - 1, np.int64)
    steps[rng.choice(Ty - 1, Te - 1, replace=False)] = 1
    return np.concatenate(([0], np.cumsum(steps))).astype(np.int64)


def problem(kind, tq, tk, seed=0):
    """scores [4, tq, tk] f32 (finite everywhere; the GPU tests poison rows >= Ty and columns >= Tx),
    q_len, key_len, grad_loss [4] f32 and, for planted kinds, the planted paths."""
    rng = np.random.default_rng([seed, tq, tk, sum(map(ord, kind))])
    q_len, key_len = lengths(tq, tk)
    B = 4
    s = np.zeros((B, tq, tk), np.float32)
    paths = [None] * B
    for b in range(B):
        Ty, Tx = clamp(q_len[b], tq), clamp(key_len[b], tk)
        if kind == "const":
            Tx = 1 << (Tx.bit_length() - 1) if Tx else 0      # a power of two: ln Tx's softmax is exact-ish
            key_len[b] = Tx if key_len[b] > 0 else key_len[b]
        if Ty == 0 or Tx == 0:
            s[b] = rng.standard_normal((tq, tk))
            continue
        n, t = np.arange(tq)[:, None], np.arange(tk)[None, :]
        if kind == "exact":
            paths[b] = planted_path(rng, Ty, Tx)
            s[b] = -128.0
            s[b, np.arange(Ty), paths[b]] = 0.0
        elif kind == "const":
            s[b] = 0.75
        elif kind == "random":        # near-diagonal: a broad ridge under unit noise
            s[b] = rng.standard_normal((tq, tk)) - 8.0 * (t / Tx - n / Ty) ** 2
        elif kind == "sharp":         # a planted path 12 above unit noise: gamma is nearly one-hot
            paths[b] = planted_path(rng, Ty, Tx)
            s[b] = rng.standard_normal((tq, tk))
            s[b, np.arange(Ty), paths[b]] += 12.0
        elif kind == "integer":       # full of ties; every f32 path sum is exact
            s[b] = rng.integers(-2, 3, (tq, tk))
        else:
            raise ValueError(kind)
    grad = np.array([1.5, -0.75, 2.0, 0.5], np.float32)
    return dict(kind=kind, tq=tq, tk=tk, scores=s, q_len=q_len, key_len=key_len, grad_loss=grad, paths=paths)


def utterances(p):
    for b in range(len(p["q_len"])):
        yield b, clamp(p["q_len"][b], p["tq"]), clamp(p["key_len"][b], p["tk"])


def references(p):
    """Per utterance the float64 truth and the float32 renormalised yardstick, computed once."""
    if "_refs" not in p:
        p["_refs"] = {b: (forward_sum(p["scores"][b], Ty, Tx, np.float64), forward_sum(p["scores"][b], Ty, Tx, np.float32))
                      for b, Ty, Tx in utterances(p)}
    return p["_refs"]


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def plus_zero(x):
    x = np.ascontiguousarray(x, np.float32)
    return bool((x.view(np.uint32) == 0).all())


# ------------------------------------------------------------------------------------------- judges
def judge_soft(p, loss, gamma, dscores, grad_loss=None):
    """loss [B], gamma and dscores [B, tq, tk] of an implementation on problem p -> (failures,
    worst): the list of what misses the bar of this module's docstring, and the greatest
    error / bar ratio seen per quantity."""
    fails, worst = [], dict(loss=0.0, gamma=0.0, dscores=0.0)
    refs = references(p)
    gl = p["grad_loss"] if grad_loss is None else grad_loss
    for b, Ty, Tx in utterances(p):
        r64, r32 = refs[b]
        g = float(gl[b])
        if not plus_zero(gamma[b, Ty:]) or not plus_zero(gamma[b, :, Tx:]):
            fails.append(f"b {b}: gamma's padding is not +0")
        if not plus_zero(dscores[b, Ty:]) or not plus_zero(dscores[b, :, Tx:]):
            fails.append(f"b {b}: dscores' padding is not +0")
        if Ty == 0 or Tx == 0:
            if not plus_zero(np.float32(loss[b])):
                fails.append(f"b {b}: loss {loss[b]} of an empty utterance")
            continue
        bar = max(MARGIN * abs(r32["loss"] - r64["loss"]), 2 * ulp32(r64["loss"]))
        err = abs(float(loss[b]) - r64["loss"])
        worst["loss"] = max(worst["loss"], err / bar)
        if not err <= bar:
            fails.append(f"b {b}: loss {loss[b]} against {r64['loss']}: error {err:.3e}, bar {bar:.3e}")
        for name, got, want, yard, scale in (("gamma", gamma[b, :Ty, :Tx], r64["gamma"], r32["gamma"], 1.0),
                                             ("dscores", dscores[b, :Ty, :Tx], g * r64["grad"], g * r32["grad"].astype(np.float64), g)):
            e = float(np.abs(yard.astype(np.float64) - want).max())
            bar = max(MARGIN * e, 2 * ulp32(scale))
            rows = np.abs(got.astype(np.float64) - want).max(1)
            if np.isnan(rows).any():
                fails.append(f"b {b}: NaN in {name}")
                continue
            worst[name] = max(worst[name], float(rows.max()) / bar)
            bad = np.nonzero(~(rows <= bar))[0]
            if len(bad):
                fails.append(f"b {b}: {name} row {bad[0]} (of {len(bad)} rows): error {rows[bad[0]]:.3e}, bar {bar:.3e}")
    return fails, worst


def judge_path(p, path, durations, logp, exact=False):
    """path [B, tq], durations [B, tk] and logp [B] on problem p: a valid path whose float64 score is
    within 1.01 * 2 Ty u M of the optimum (u = 2^-24, M = sum_n max_t |s[n, t]|: one rounded add per
    row on sums no greater than M; the MAS test's bound with exact scores), -1 / 0 / 0 in the padding
    and for empty utterances, durations the path's histogram, and logp within max(4 x the float32
    evaluation's distance from float64, 2 ulp32 of the greatest |s| or |lse|) of the float64 value
    along the returned path.  exact: the path must equal the float64 reference's (integer or peaky
    scores)."""
    fails = []
    for b, Ty, Tx in utterances(p):
        live = Ty > 0 and Tx > 0
        n_path = Ty if live else 0
        if (path[b, n_path:] != -1).any():
            fails.append(f"b {b}: path past the utterance is not -1")
        got = path[b, :n_path].astype(np.int64)
        if not live:
            if (durations[b] != 0).any() or not plus_zero(np.float32(logp[b])):
                fails.append(f"b {b}: durations / logp of an empty utterance")
            continue
        why = check_path(got, Ty, Tx)
        if why:
            fails.append(f"b {b}: {why}")
            continue
        if not np.array_equal(durations[b], np.concatenate((durations_of(got, Tx), np.zeros(p["tk"] - Tx, np.int64)))):
            fails.append(f"b {b}: durations are not the path's histogram")
        s64 = p["scores"][b, :Ty, :Tx].astype(np.float64)
        best, _, _ = hard(s64, Ty, Tx)
        gap = path_score(s64, best) - path_score(s64, got)
        bound = 1.01 * 2 * Ty * 2.0 ** -24 * np.abs(s64).max(1).sum()
        if not -1e-9 <= gap <= bound:
            fails.append(f"b {b}: path score {gap:.3e} under the optimum, bound {bound:.3e}")
        if exact and not np.array_equal(got, best):
            fails.append(f"b {b}: path differs from the float64 path at frame {int(np.argmax(got != best))}")
        want, yard = logp_of(s64, got), logp_of(s64, got, np.float32)
        big = max(np.abs(s64).max(), abs(forward_sum(s64, Ty, Tx)["lse"]).max())
        bar = max(MARGIN * abs(yard - want), 2 * ulp32(big))
        if not abs(float(logp[b]) - want) <= bar:
            fails.append(f"b {b}: logp {logp[b]} against {want}: bar {bar:.3e}")
    return fails


def judge_reduced(p, reduction, value, per_tx=True):
    """forward_sum_loss's reduced value on problem p.  The bar is the per-utterance loss bars of
    judge_soft carried through the reduction's weights w_b (1, or 1 / (max(Tx_b, 1) B) for "mean")
    plus B ulp32 of sum_b |w_b loss_b| for the float32 reduction itself (B divisions, B - 1 adds and
    one division, each within half an ulp of a value no greater than that sum)."""
    refs = references(p)
    rows = list(utterances(p))
    B = len(rows)
    l64 = np.array([refs[b][0]["loss"] for b, _, _ in rows])
    l32 = np.array([refs[b][1]["loss"] for b, _, _ in rows])
    bars = np.array([max(MARGIN * abs(a - c), 2 * ulp32(c)) if c else 0.0 for a, c in zip(l32, l64)])
    tx = np.array([Tx for _, _, Tx in rows], np.float64)
    w = np.ones(B) if reduction != "mean" else 1.0 / (np.maximum(tx, 1.0) * B)
    want = reduce_loss(l64, tx, reduction)
    if reduction == "none":
        err, bar = np.abs(np.asarray(value, np.float64) - want), bars
        return [f"b {b}: loss error {err[b]:.3e}, bar {bar[b]:.3e}" for b in range(B) if not err[b] <= bar[b]]
    bar = float((w * bars).sum() + B * ulp32(float((w * np.abs(l64)).sum())))
    err = abs(float(value) - float(want))
    return [] if err <= bar else [f"{reduction}: {value} against {want}: error {err:.3e}, bar {bar:.3e}"]
