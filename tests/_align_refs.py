"""References, problems, numpy-float32 models and judges of what reads the cross-attention's
by-products: the guided instantiations of the attention kernels (tt2_attn_fwd_guided /
tt2_attn_bwd_guided), tt2_guided_attn_loss, tt2_attn_align and tt2_align_durations, written from the
contract in include/tt2_capi.h on top of tests/_attn_refs.py.  Everything runs on the CPU.
tests/test_align_refs.py validates this file against autograd and the plain twin and proves with
mutants that the judges bite; tests/test_gpu_guided_exact.py and tests/test_gpu_align_exact.py hold
the kernels to them.

guided_ref64   float64: W as the header states it, g = sum_t P W, the gradients of
               sum(o * do) + kappa * sum(g) by autograd, delta = rowsum(dO * O) + kappa g.
GuidedTwin     _attn_refs.Twin with the guided term, rounded where the kernels round: g from the
               unrounded p in f32 (divided by l once), dS = P (dP + kappa W - (delta + kappa g))
               rounded to bf16 for dQ / dK.  With kappa = 0 it is the plain twin bit for bit.
indicator      sigma = 2^-12 turns W into an exact indicator (0 on the diagonal t Ty == n Tx, 1
               elsewhere) whenever Ty_b is Tx_b times a power of two: assert_indicator() evaluates
               the kernels' own float32 formula in numpy and must be run before each launch.
models         numpy float32, from the header: loss term / coefficient, focus, pmax, amax,
               the durations histogram.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

import _attn_refs as R
from _attn_refs import D, F64, INF, LOG2E, Problem, Twin
from _misc_refs import ulp

F32 = torch.float32
INDICATOR_SIGMA = 2.0 ** -12
f32 = np.float32


@dataclass(frozen=True)
class Guide:
    q_len: object            # tuple of B ints, or None (tq)
    sigma: float
    heads: int               # heads h < heads are guided
    kappa: float


def lengths(p, gd):
    """(Tx [B], Ty [B]): the visible keys and the valid query rows of each utterance."""
    B, H, Tq, Tk = p.shape
    return R.key_limits(B, Tk, p.key_len), R.key_limits(B, Tq, None if gd.q_len is None else list(gd.q_len))


def guide_weight(p, gd, dtype=F64, wrong=None):
    """W[b, n, t] = 1 - exp(-(t / Tx_b - n / Ty_b)^2 / (2 sigma^2)) in `dtype`, [B, 1, Tq, Tk]
    (Tx_b, Ty_b taken as 1 for an utterance without a key or a row, which no head guides).
    wrong (mutants): 'n+1', 't+1', '4hi' (the 4 * hi of the second lane half's keys dropped),
    'full' (Tx, Ty taken as tk, tq)."""
    B, H, Tq, Tk = p.shape
    tx, ty = (x.to(dtype).clamp_min(1).view(B, 1, 1, 1) for x in lengths(p, gd))
    t = torch.arange(Tk, dtype=dtype).view(1, 1, 1, Tk)
    n = torch.arange(Tq, dtype=dtype).view(1, 1, Tq, 1)
    if wrong == "n+1":
        n = n + 1
    elif wrong == "t+1":
        t = t + 1
    elif wrong == "4hi":
        t = t - 4 * ((torch.arange(Tk) >> 2) & 1).to(dtype).view(1, 1, 1, Tk)
    elif wrong == "full":
        tx, ty = torch.full_like(tx, Tk), torch.full_like(ty, Tq)
    x = t / tx - n / ty
    return 1 - torch.exp(-(x * x) / torch.tensor(2 * gd.sigma * gd.sigma, dtype=dtype))


def guided_rows(p, gd):
    """bool [B, H, Tq, 1]: the rows the guide acts on (h < heads, n < Ty_b, Tx_b > 0)."""
    B, H, Tq, Tk = p.shape
    tx, ty = lengths(p, gd)
    rows = (torch.arange(Tq)[None, :] < ty[:, None]) & (tx[:, None] > 0)
    return (rows[:, None, :] & (torch.arange(H) < gd.heads)[None, :, None])[..., None]


# ------------------------------------------------------------------ float64 reference
def guided_ref64(p, gd):
    """{'o', 'lse', 'g', 'delta', 'dq', 'dk', 'dv'} in float64.  g is exactly 0 on heads >= heads,
    rows >= Ty_b and rows with no visible key; the gradients are those of sum(o * do) + kappa sum(g)
    by autograd; o and lse are _attn_refs.ref64's."""
    B, H, Tq, Tk = p.shape
    base = R.ref64(p)
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (p.q, p.k, p.v))
    vis = R.visible(B, Tq, Tk, p.key_len, p.causal)
    live = vis.any(-1, keepdim=True)
    x = ((q @ k.transpose(-1, -2)) * p.scale).masked_fill(~vis, -INF)
    prob = torch.softmax(torch.where(live, x, torch.zeros_like(x)), -1) * vis if Tk else x
    w = guide_weight(p, gd) * guided_rows(p, gd)
    g = (prob * w).sum(-1)
    o = prob @ v
    ((o * p.do).sum() + gd.kappa * g.sum()).backward()
    assert (o.detach() - base["o"]).abs().max().item() < 1e-12 if o.numel() else True
    g = g.detach()
    return {"o": base["o"], "lse": base["lse"], "g": g, "delta": (p.do * base["o"]).sum(-1) + gd.kappa * g,
            "dq": q.grad, "dk": k.grad, "dv": v.grad}


# ------------------------------------------------------------------ the guided twin
class GuidedTwin(Twin):
    """See the module docstring.  The steps a guided kernel could get wrong are methods, so that
    tests/test_align_refs.py can derive mutants."""

    def __init__(self, guide, dtype=F64, rnd=torch.bfloat16):
        super().__init__(dtype, rnd)
        self.guide = guide

    def weight(self, p):
        return guide_weight(p, self.guide, self.dtype)

    def rows(self, p):
        """The rows g is stored for (everything else stores 0)."""
        return guided_rows(p, self.guide)

    def kappa_rows(self, p):
        """The rows kappa acts on in the backward."""
        return guided_rows(p, self.guide)

    def g_probs(self, pf):
        return pf                                            # unrounded: p W is formed in f32

    def delta_term(self, kap, g):
        return kap * g

    def w_term(self, kap, w):
        return kap * w

    def __call__(self, p):
        dt = self.dtype
        q, k, v, do = (t.to(dt) for t in (p.q, p.k, p.v, p.do))
        scale = torch.tensor(p.scale, dtype=dt)
        c = scale * torch.tensor(LOG2E, dtype=dt)
        vis = self.visible(p)
        x = ((q @ k.transpose(-1, -2)) * c).masked_fill(~vis, -INF)
        m, l = self.stats(x)
        pf = torch.exp2(x - m)
        safe = torch.where(l > 0, l, torch.ones_like(l))
        o_acc = (self.r(pf) @ v) / safe
        w = self.weight(p)
        g = torch.where(self.rows(p) & (l > 0), (self.g_probs(pf) * w).sum(-1, keepdim=True) / safe, torch.zeros_like(l))
        o_delta, o, lse = self.saved(o_acc, self.r(o_acc), self.lse(m, l))
        pb = torch.exp2(x - lse)
        dp = do @ v.transpose(-1, -2)
        kap = self.kappa_rows(p).to(dt) * torch.tensor(self.guide.kappa, dtype=dt)
        delta = (do * o_delta).sum(-1, keepdim=True) + self.delta_term(kap, g)
        ds = self.round_ds(pb * (dp + self.w_term(kap, w) - delta))
        return {"o": o.to(F64), "lse": lse.squeeze(-1).to(F64), "g": g.squeeze(-1).to(F64),
                "delta": delta.squeeze(-1).to(F64),
                "dq": self.r((ds @ k) * scale).to(F64),
                "dk": self.r((ds.transpose(-1, -2) @ q) * scale).to(F64),
                "dv": self.r(self.r(pb).transpose(-1, -2) @ do).to(F64)}


def guided_float32_evaluations(p, gd, orders=8, twin=GuidedTwin):
    """_attn_refs.float32_evaluations with the guided term: the float32 CPU evaluation in `orders`
    accumulation orders of the head dimension (W is evaluated in float32 from the header's formula)."""
    outs = []
    for i in range(orders):
        perm = torch.arange(D) if i == 0 else torch.randperm(D, generator=torch.Generator().manual_seed(i))
        out = twin(gd, F32, None)(Problem(p.q[..., perm], p.k[..., perm], p.v[..., perm], p.do[..., perm],
                                          p.key_len, p.causal, p.scale))
        inv = torch.argsort(perm)
        outs.append({n: (x if x.dim() == 3 else x[..., inv]) for n, x in out.items()})
    return outs


# ------------------------------------------------------------------ the indicator guide
def kernel_gk(sigma):
    """log2(e) / (2 sigma^2) as to_args<true> forms it in float32."""
    return f32(f32(LOG2E) / (f32(2) * f32(sigma) * f32(sigma)))


def kernel_weight(tx, ty, sigma, fused=0):
    """(W, e) [ty, tx] of one utterance by the kernels' own float32 formula: tk = t * (1 / Tx),
    nq = n * (1 / Ty), x = tk - nq, e = -(x * x) * gk, W = 1 - exp2(e).  fused = 1 / 2: the
    subtraction contracted with the first / second product into one fma, as a compiler may."""
    rk, rq = f32(1) / f32(tx), f32(1) / f32(ty)
    t, n = np.arange(tx, dtype=f32), np.arange(ty, dtype=f32)
    tk, nq = (t * rk)[None, :], (n * rq)[:, None]
    if fused == 1:
        x = (t.astype(np.float64)[None, :] * np.float64(rk) - nq.astype(np.float64)).astype(f32)
    elif fused == 2:
        x = (tk.astype(np.float64) - n.astype(np.float64)[:, None] * np.float64(rq)).astype(f32)
    else:
        x = tk - nq
    e = -(x * x) * kernel_gk(sigma)
    with np.errstate(under="ignore"):
        return f32(1) - np.exp2(e), e


def assert_indicator(p, gd):
    """Every utterance's W is exactly 0 on the diagonal t Ty_b == n Tx_b and exactly 1 elsewhere in
    the kernels' float32 arithmetic: every off-diagonal exponent is <= -150, below the smallest
    float32 subnormal (2^-149), so the library exp2 and the hardware instruction both give 0;
    on the diagonal x is 0 (or, under an fma contraction, one rounding residual, whose exponent
    is above -2^-25 and exp2 rounds to 1).  Returns the smallest margin seen, -150 - max(e)."""
    margin = INF
    for tx, ty in zip(*(x.tolist() for x in lengths(p, gd))):
        if tx == 0 or ty == 0:
            continue
        diag = np.arange(tx)[None, :] * ty == np.arange(ty)[:, None] * tx
        for fused in (0, 1, 2):
            w, e = kernel_weight(tx, ty, gd.sigma, fused)
            assert np.isin(w, (0.0, 1.0)).all(), f"Tx {tx} Ty {ty}: W is not an indicator"
            assert ((w == 0) == diag).all(), f"Tx {tx} Ty {ty}: the zeros of W are not the diagonal"
            assert not np.signbit(w).any()
            if (~diag).any():
                assert e[~diag].max() <= -150, f"Tx {tx} Ty {ty}: exponent {e[~diag].max()} off the diagonal"
                margin = min(margin, -150 - float(e[~diag].max()))
    return margin


def guided_selector_problem(B, H, Tq, Tk, key_len, gd, pair_frac=0.5, share=0.9):
    """_attn_refs.selector_problem whose rows pick their on-diagonal key as t1 with probability
    `share` where they have one (selector_problem's `diag`).  With the indicator guide every P is
    1 or 1/2 twice and every W is 0 or 1, so g is 0, 1/2 or 1: 0 on a one-hot diagonal row, 1/2 on a
    pair row (its t2 is off the diagonal), 1 elsewhere.  With kappa a power of two, one-hot rows
    have dS = kappa (W - g) = 0 and pair rows dS = +-((dP1 - dP2) + kappa (W1 - W2)) / 4."""
    return R.selector_problem(B, H, Tq, Tk, key_len, False, pair_frac=pair_frac, diag=(gd.q_len, share))


def diagonal_share(p, gd, ref):
    """Share of the guided valid rows that put weight on their diagonal key (g < 1)."""
    rows = guided_rows(p, gd).squeeze(-1) & R.live_rows(p)[0]
    return ((ref["g"] < 1) & rows).sum().item() / max(rows.sum().item(), 1)


def assert_exact_guided(ref, p, gd, what=""):
    """assert_exact_problem extended to g and delta: O and the gradients are bf16 values, g is 0,
    1/2 or 1 and delta a float32 value; and the float64 twin with the kernels' roundings returns the
    reference bit for bit, so rounding dS to bf16 loses nothing either."""
    R.assert_exact_problem(ref, what)
    g32 = ref["g"].to(F32).to(F64)
    assert bool(((g32 == 0) | (g32 == 0.5) | (g32 == 1)).all()) and (ref["g"] - g32).abs().max().item() < 1e-100, what
    assert R.representable(ref["delta"], F32), what
    tw = GuidedTwin(gd)(p)
    for n in ("o", "g", "delta") + R.GRADS:
        assert torch.equal(tw[n].to(F32), ref[n].to(F32)), f"{what}: {n} of the rounded twin leaves the reference: thin the pair rows"


def random_diagonal_problem(B, H, Tq, Tk, key_len, gd, dtype, seed=1):
    """random_problem with 8 K[b, h, floor(n Tx_b / Ty_b)] added to Q on the valid rows: P is
    sharply diagonal and g small."""
    p = R.random_problem(B, H, Tq, Tk, key_len, False, dtype, seed=seed)
    tx, ty = lengths(p, gd)
    for b in range(B):
        if tx[b] > 0 and ty[b] > 0:
            n = torch.arange(int(ty[b]))
            p.q[b, :, :int(ty[b])] += 8 * p.k[b][:, (n * int(tx[b])) // int(ty[b])]
    p.q = p.q.to(dtype).to(F64)
    return p


# ------------------------------------------------------------------ judges of the guided kernels
def _positive_zero(x, mask):
    """x is +0 (not -0, not NaN) wherever mask holds."""
    x = x[mask]
    return bool(((x == 0) & ~torch.signbit(x)).all())


def zero_rows(p, gd):
    """bool [B, H, Tq]: where g must be exactly +0."""
    B, H, Tq, Tk = p.shape
    return ~(guided_rows(p, gd).squeeze(-1) & R.live_rows(p)[0].expand(B, H, Tq))


def judge_guided_selector(out, ref, p, gd, dtype):
    """judge_selector, plus: g and delta bit-equal to the float64 reference cast to float32; g
    exactly +0 on unguided heads, rows >= Ty_b and empty rows."""
    fails, figs = R.judge_selector(out, ref, p, dtype)
    for n in ("g", "delta"):
        want = ref[n].to(F32).to(F64)
        if not torch.equal(out[n], want):
            fails.append(f"{n} differs from the float64 reference: {R._first_diff(out[n], want)}")
    if not _positive_zero(out["g"], zero_rows(p, gd)):
        fails.append("g is not +0 on an unguided head, a row >= Ty or an empty row")
    return fails, figs


EXP2_ALLOWANCE = 64.0
"""Allowance for the hardware exp2 (v_exp_f32) behind the kernels' P and W (the v3 kernels call it
directly, the v1 kernels through exp2f, which compiles to the same instruction) and the float32
score arithmetic that feeds it, in units of 2^-24 * sum_t P |W| of the row, on top of max(4 x the
float32 CPU evaluations' error, 2 f32 ulp).  The next power of two at or above twice the worst
excess measured on an MI355X over the two problems that get this bar in
tests/test_gpu_guided_exact.py: 2.51 on the random problem (131x193, v1 bf16) and 28.67 on the
diagonal problem (33x64, heads 3, one row, the three v3 variants alike).  The random problem alone
would give 8, under which that row sits at 1.48 times its bar.  The excess there is not W's: the
kernels' float32 W formula evaluated in numpy on the float64 P sits at 0.39 of the bar.  It is the
off-diagonal keys' P: the scores of that problem are near 500, where an ulp is 6e-5, so the
exponents of the small p carry some 1e-5 of float32 accumulation noise of the 64-term dot product,
and on a sharply diagonal row they are most of g."""


def g_row_figures(g, ref, yard32, p, gd):
    """(ratio, excess): per row err = |g - ref|, first = max(4 x the worst float32 evaluation's error
    on that row, 2 f32 ulp of S = sum_t P |W|); ratio = max err / (first + EXP2_ALLOWANCE 2^-24 S)
    and excess = max (err - first) / (2^-24 S), the figure the allowance is set from (<= 0: none
    needed).  The v1 kernels call exp2f, which the compiler lowers to the same instruction: they
    measured an excess too and get the same allowance.
    A row whose reference is exactly 0 by construction must be +0."""
    zero = zero_rows(p, gd)
    if not _positive_zero(g, zero) or torch.isnan(g).any():
        return INF, INF
    s = ref["g"].abs()                                       # W >= 0: sum P |W| is g itself
    e32 = torch.stack([(y["g"] - ref["g"]).abs() for y in yard32]).amax(0)
    first = torch.maximum(4 * e32, 2 * ulp(torch.where(s > 0, s, torch.ones_like(s)), F32))
    unit = 2.0 ** -24 * s
    err = (g - ref["g"]).abs()
    live = ~zero & (s > 0)
    if not live.any():
        return 0.0, 0.0
    ratio = (err / (first + EXP2_ALLOWANCE * unit))[live].max().item()
    excess = ((err - first) / unit)[live].max().item()
    return ratio, excess


def delta_row_ratio(out, ref, yard32, p, gd):
    """delta per row against rowsum(dO * O) + kappa g formed in float64 from the O and g the
    kernel itself stored (the header's statement of what the backward leaves there), within
    max(4 x the worst float32 evaluation's error of delta on that row, 2 f32 ulp of
    sum |dO O| + |kappa| g)."""
    want = (p.do * out["o"]).sum(-1) + gd.kappa * guided_rows(p, gd).squeeze(-1) * out["g"]
    mag = (p.do * out["o"]).abs().sum(-1) + abs(gd.kappa) * out["g"].abs()
    e32 = torch.stack([(y["delta"] - ref["delta"]).abs() for y in yard32]).amax(0)
    allowed = torch.maximum(4 * e32, 2 * ulp(torch.where(mag > 0, mag, torch.ones_like(mag)), F32))
    err = (out["delta"] - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, INF))
    return (err / allowed).max().item() if err.numel() else 0.0


def guided_cancel_bound(p, gd):
    """cancel_bound extended by the kappa (W - g) term: on a row with a single visible key g = W
    identically and dS cancels; W and g are each within 8 f32 ulp of 1 plus the exp2 allowance, and
    the difference is multiplied by |kappa|, one K (or Q) row and scale."""
    big = max(p.k.abs().max().item() if p.k.numel() else 0.0, p.q.abs().max().item(), 1.0)
    return R.cancel_bound(p) + 2 * (8 + EXP2_ALLOWANCE) * 2.0 ** -24 * abs(gd.kappa) * big * p.scale * (1 + 2.0 ** -8)


def block_ratio(out, ref, yard, factor, floor, live=None, bound=0.0):
    """_attn_refs.worst_ratio, with its `cancel` rule carried from the blocks whose reference is
    exactly zero to the blocks whose reference is below the cancellation bound itself: where dS
    cancels (a single visible key; a row whose weight sits on one key to float32 precision, as on
    the diagonal problem, where the float64 reference is 1e-19 and the float64 twin returns exactly
    0) a float32 kernel leaves rounding noise that no relative bar can meet, and max |out - ref| <=
    bound is accepted in its place.  live: bool [B, 1 or H, T], the rows with a visible pair."""
    ek = R.block_errors(out, ref)
    ey = torch.stack([R.block_errors(y, ref) for y in (yard if isinstance(yard, (list, tuple)) else [yard])]).amax(0)
    allowed = torch.clamp_min(factor * ey, floor)
    ratio = torch.where(ek == 0, torch.zeros_like(ek), ek / allowed)
    if live is not None:
        B, H, T, _ = ref.shape
        lv = R._blocks(live.expand(B, H, T)[..., None].to(F64), 32).amax(-1) > 0
        small = R._blocks(ref, 32).abs().amax(-1) <= bound
        diff = torch.nan_to_num(R._blocks((out - ref).abs(), 32), nan=INF).amax(-1)
        ratio = torch.where(small & lv, torch.fmin(ratio, diff / bound), ratio)      # (fmin: inf / inf above is NaN)
    return ratio.max().item()


def judge_guided_random(out, ref, yard, yard32, p, gd, dtype):
    """Per unit of work: every 32-row block of O, dQ, dK, dV against the guided twin (bf16, factor
    2) or the guided float32 evaluations (f32, factor 4, floor 2 f32 ulp), block_ratio's rule where
    dS cancels; g and delta per row (g_row_figures, delta_row_ratio); the LSE as judge_random."""
    fails, figs = [], {}
    factor, floor = (2.0, 0.0) if dtype == torch.bfloat16 else (4.0, R.F32_FLOOR)
    qlive, klive = R.live_rows(p)
    cb = guided_cancel_bound(p, gd)
    cancel = {"dq": (qlive, cb), "dk": (klive, cb)}
    for n in ("o",) + R.GRADS:
        ys = [y[n] for y in yard] if isinstance(yard, (list, tuple)) else yard[n]
        figs[n] = block_ratio(out[n], ref[n], ys, factor, floor, *cancel.get(n, ()))
        if not figs[n] <= 1:
            fails.append(f"{n}: worst 32-row block at {figs[n]:.3g} times its bar")
    figs["lse"] = R.lse_ratio(out["lse"], ref["lse"], [y["lse"] for y in yard32], unit=True)
    figs["g"], figs["g_excess"] = g_row_figures(out["g"], ref, yard32, p, gd)
    figs["delta"] = delta_row_ratio(out, ref, yard32, p, gd)
    for n, what in (("lse", "lse"), ("g", "g: worst row"), ("delta", "delta: worst row")):
        if not figs[n] <= 1:
            fails.append(f"{what} at {figs[n]:.3g} times its bar")
    return fails, figs


def g_relative_error(g, ref, p, gd):
    """Worst per-row relative error of g over the rows whose reference is not 0."""
    live = ~zero_rows(p, gd) & (ref["g"] > 0)
    return ((g - ref["g"]).abs() / ref["g"].clamp_min(1e-300))[live].max().item() if live.any() else 0.0


def old_guided_bars(out, ref, dtype):
    """The bars of tests/test_gpu_guided_attention.py: relative Frobenius norms over whole tensors,
    g at 2e-6 (f32) / 1e-2 (bf16), O at 2e-6 / 1e-2, gradients at 5e-6 / 2e-2.  True if they accept."""
    def rel(a, b):
        return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
    fwd, bwd = (2e-6, 5e-6) if dtype == F32 else (1e-2, 2e-2)
    return rel(out["g"], ref["g"]) < fwd and rel(out["o"], ref["o"]) < fwd and all(rel(out[n], ref[n]) < bwd for n in R.GRADS)


# ------------------------------------------------------------------ tt2_guided_attn_loss
def loss_rows(c):
    """The g buffers of a loss case: [L][B, H, tq] float64, integers in [0, 7] on the guided heads
    (every float32 partial sum is exact in any order), NaN on the others."""
    g = torch.Generator().manual_seed(c["seed"])
    rows = torch.randint(0, 8, (c["L"], c["B"], c["H"], c["tq"]), generator=g).to(F64)
    rows[:, :, c["gh"]:] = float("nan")
    return rows


def loss_model(c, rows, drop_pair=None):
    """(term, coef, loss_out[0]) as numpy float32 from the header: N = L guide_heads sum_b Tx_b Ty_b,
    term = float32(float64(scale) float64(sum) / N), coef = float32(float64(scale) float64(grad_scale)
    / N), loss_out[0] + term in float32; N = 0: 0, 0 and loss_out untouched.  drop_pair: a (layer,
    batch) pair left out of the sum (mutant)."""
    kl = [c["tk"]] * c["B"] if c["key_len"] is None else c["key_len"]
    ql = [c["tq"]] * c["B"] if c["q_len"] is None else c["q_len"]
    n = c["L"] * c["gh"] * sum(min(max(a, 0), c["tk"]) * min(max(b, 0), c["tq"]) for a, b in zip(kl, ql))
    guided = rows[:, :, :c["gh"]].clone()
    if drop_pair is not None and guided.numel():
        guided.view(c["L"] * c["B"], -1)[drop_pair] = 0
    total = f32(guided.sum().item())
    assert float(total) == guided.sum().item() and guided.sum().item() < 2 ** 24
    scale, gs = np.float64(f32(c["scale"])), np.float64(f32(c["grad_scale"]))
    loss0 = None if c["loss0"] is None else f32(c["loss0"])
    if n == 0:
        return f32(0), f32(0), loss0
    term = f32(scale * np.float64(total) / np.float64(n))
    return term, f32(scale * gs / np.float64(n)), None if loss0 is None else f32(loss0 + term)


def _lc(name, L, B, H, gh, tq, tk, key_len=None, q_len=None, offset=0, loss0=2.5, scale=10.0, grad_scale=0.5, seed=0):
    return dict(name=name, L=L, B=B, H=H, gh=gh, tq=tq, tk=tk, key_len=key_len, q_len=q_len, offset=offset,
                loss0=loss0, scale=scale, grad_scale=grad_scale, seed=seed + 13 * tq + L)


LOSS_CASES = [
    _lc("pairs18-below", 3, 6, 3, 2, 64, 50, [50, 40, 0, 7, 50, 1], [64, 3, 64, 0, 33, 64]),   # 128 < 256 floats per pair
    _lc("pairs18-above", 3, 6, 3, 2, 200, 50, [50, 40, 0, 7, 50, 1], [200, 3, 64, 0, 133, 199]),  # 400 > 256
    _lc("odd-tq", 2, 2, 3, 2, 131, 133, [133, 70], [131, 40]),                                # scalar: 262 % 4 != 0
    _lc("misaligned", 2, 2, 3, 2, 64, 50, [50, 40], [64, 3], offset=1),                       # scalar: pointer
    _lc("all-heads", 1, 2, 3, 3, 64, 50),
    _lc("no-heads", 2, 2, 3, 0, 64, 50),                                                      # N = 0
    _lc("lengths-0", 2, 2, 3, 2, 64, 50, [0, 0], [0, 0]),                                     # N = 0
    _lc("lengths-out", 2, 3, 3, 2, 64, 50, [59, -3, 20], [69, 7, -1]),                        # above tq / tk, negative
    _lc("no-loss-out", 2, 2, 3, 2, 64, 50, [50, 40], [64, 3], loss0=None),
    _lc("layers16", 16, 2, 3, 1, 8, 5),                                                       # every layer slot
]


# ------------------------------------------------------------------ tt2_attn_align
def kernel_c(scale):
    """scale * log2(e) as the kernels form it: one float32 product."""
    return f32(f32(scale) * f32(LOG2E))


def align_valid(B, H, Tq, Tk, key_len, q_len):
    """bool [B, H, Tq]: rows n < Ty_b of utterances with a visible key."""
    tx, ty = R.key_limits(B, Tk, key_len), R.key_limits(B, Tq, q_len)
    return ((torch.arange(Tq)[None, :] < ty[:, None]) & (tx[:, None] > 0))[:, None, :].expand(B, H, Tq)


def masked_scores(p):
    """Q K^T in float64 [B, H, Tq, Tk], -inf on the keys at and past the key limit."""
    B, H, Tq, Tk = p.shape
    return (p.q @ p.k.transpose(-1, -2)).masked_fill(~R.visible(B, Tq, Tk, p.key_len, False), -INF)


def lowest_argmax(s, rule="lowest"):
    """The key index of each row's maximum of s [..., Tk] (Tk > 0).  rule: 'lowest' index of a tie
    (the header), or the mutants 'highest' and 'halves' (the tie is settled inside each lane half
    of the MFMA kernel -- keys with bit 2 clear / set -- and the second half then wins a tie
    between the halves)."""
    tk = s.shape[-1]
    top = s == s.amax(-1, keepdim=True)
    idx = torch.arange(tk).expand_as(s)
    low = torch.where(top, idx, torch.full_like(idx, tk)).amin(-1)
    if rule == "lowest":
        return low
    if rule == "highest":
        return torch.where(top, idx, torch.full_like(idx, -1)).amax(-1)
    second = torch.where(top & ((idx >> 2) & 1 == 1), idx, torch.full_like(idx, tk)).amin(-1)
    return torch.where(second < tk, second, low)


def align_exact_problem(B, H, Tq, Tk, key_len, dup=True):
    """The plain selector problem with a supplied LSE: lse[n] = float32(s_max c) + m, m = n mod 4,
    and +inf on the rows n mod 11 == 5, so pmax = 2^-m exactly (s_max c is below 4096, so adding m
    <= 3 and subtracting again are exact in float32).  amax is the unique key on one-hot rows and
    min(t1, t2) on pair rows; t2 = t1 mod 32 crosses the 32-key halves and the 64-key tiles, and
    with `dup` the keys 8j + 4 .. 8j + 7 of every third group of eight are copies of 8j .. 8j + 3,
    the same key rows in the other lane half, so ties cross the lane halves too.
    Returns (problem, lse [B, H, Tq] float64 holding float32 values)."""
    p = R.selector_problem(B, H, Tq, Tk, key_len, False)
    if dup:
        t = torch.arange(Tk)
        src = torch.where(((t // 8) % 3 == 0) & (t % 8 >= 4), t - 4, t)
        p.k = p.k[:, :, src].clone()
    s = masked_scores(p)
    smax = s.amax(-1) if Tk else torch.full((B, H, Tq), -INF, dtype=F64)
    x = torch.from_numpy((smax.clamp_min(0).numpy().astype(f32) * kernel_c(p.scale)).astype(np.float64))
    n = torch.arange(Tq).expand(B, H, Tq)
    lse = torch.where(n % 11 == 5, torch.full_like(x, INF), x + (n % 4).to(F64))
    assert torch.equal(lse.to(F32).to(F64), lse)
    return p, lse


def align_exact_expected(p, lse, q_len, rule="lowest"):
    """(pmax, amax) the header promises on align_exact_problem: 2^-m and the lowest key of the
    maximum; exactly +0 and -1 on rows >= q_len[b], +inf rows and utterances without a key."""
    B, H, Tq, Tk = p.shape
    ok = align_valid(B, H, Tq, Tk, p.key_len, q_len) & torch.isfinite(lse)
    if Tk == 0:
        return torch.zeros(B, H, Tq, dtype=F64), torch.full((B, H, Tq), -1, dtype=torch.long)
    s = masked_scores(p)
    m = (torch.arange(Tq) % 4).to(F64).expand(B, H, Tq)
    return torch.where(ok, torch.exp2(-m), torch.zeros_like(m)), \
        torch.where(ok, lowest_argmax(s, rule), torch.full((B, H, Tq), -1, dtype=torch.long))


GAP = 1e-4          # tests/test_gpu_align_kernels.py's top-2 gap in scaled score


def align_random_reference(p, q_len, orders=16):
    """For a random problem: the LSE in float64 rounded to float32 (what the test feeds the
    kernel), pmax = exp2(s_max scale log2(e) - lse) in float64 from that rounded LSE, the float32
    evaluations of the same (the dot product in `orders` accumulation orders, each with the product
    s_max * scale * log2(e) associated both ways -- the rounding of that product, at |x| up to 30,
    is the largest error of a row --, the subtraction in float32, torch's float32 exp2), the top-2 keys [B, H, Tq, 2], their gap in scaled score,
    and the valid rows."""
    B, H, Tq, Tk = p.shape
    valid = align_valid(B, H, Tq, Tk, p.key_len, q_len)
    s = masked_scores(p)
    lse = R.ref64(p)["lse"].to(F32)
    smax = s.amax(-1)
    dead = ~torch.isfinite(smax)
    pm = torch.where(valid & ~dead, torch.exp2(smax.masked_fill(dead, 0) * (float(f32(p.scale)) * LOG2E) - lse.to(F64)),
                     torch.zeros_like(smax))
    evals = []
    c32 = torch.tensor(float(kernel_c(p.scale)), dtype=F32)
    sc32, l2e32 = torch.tensor(p.scale, dtype=F32), torch.tensor(LOG2E, dtype=F32)
    vis = R.visible(B, Tq, Tk, p.key_len, False)
    for i in range(orders):
        perm = torch.arange(D) if i == 0 else torch.randperm(D, generator=torch.Generator().manual_seed(i))
        s32 = (p.q[..., perm].to(F32) @ p.k[..., perm].to(F32).transpose(-1, -2)).masked_fill(~vis, -INF).amax(-1)
        for x in (s32.masked_fill(dead, 0) * c32, (s32.masked_fill(dead, 0) * sc32) * l2e32):
            e = torch.exp2(x - lse)
            evals.append(torch.where(valid & ~dead, e, torch.zeros_like(e)).to(F64))
    top = (s * p.scale).topk(min(2, Tk), dim=-1)
    idx = top.indices if Tk > 1 else torch.cat([top.indices, top.indices], -1)
    gap = (top.values[..., 0] - top.values[..., 1]) if Tk > 1 else torch.full_like(smax, INF)
    gap = torch.where(torch.isnan(gap), torch.full_like(gap, INF), gap)
    x = smax.masked_fill(dead, 0) * (float(f32(p.scale)) * LOG2E)
    mag = (p.q.abs() @ p.k.abs().transpose(-1, -2)).gather(-1, idx[..., :1]).squeeze(-1) * (float(f32(p.scale)) * LOG2E)
    return {"lse": lse, "pmax": pm, "x": x, "mag": mag, "evals": evals, "top2": idx, "gap": gap, "valid": valid & ~dead}


def judge_align_exact(pmax, amax, want_p, want_a):
    """Bit for bit: pmax (as float32 bits, so -0 fails) and amax."""
    fails = []
    got_bits, want_bits = pmax.to(F32).view(torch.int32), want_p.to(F32).view(torch.int32)
    if not torch.equal(got_bits, want_bits):
        fails.append(f"pmax differs: {R._first_diff(pmax.to(F64), want_p.to(F64))}")
    if not torch.equal(amax.long(), want_a.long()):
        fails.append(f"amax differs: {R._first_diff(amax.long(), want_a.long())}")
    return fails


def judge_align_random(pmax, amax, ref):
    """pmax per row within max(4 x the float32 evaluations' error on that row, 2 f32 ulp), exactly
    +0 with amax -1 on the invalid rows.  The 2 ulp are taken where float32 rounds: 2 ulp of pmax
    for exp2 and the store, and 2 ulp of the exponent's operand x = s_max scale log2(e) (|x| up to
    30 here, so half an ulp of x alone is 5 ulp of pmax) together with the 64-term float32 dot
    product behind it, sqrt(64) 2^-24 sum_d |q_d k_d| scale log2(e) (the random-walk size of its 64
    roundings; the worst case is 64 2^-24), both carried through exp2 as a factor ln 2 * pmax.
    With 2 ulp of pmax alone a float32 CPU evaluation held out of the yardstick sat at up to 2.3
    times the bar at these shapes (tests/test_align_refs.py prints where one sits under this floor:
    at most 0.42): no float32 computation can be held to that. amax the reference's on rows with a top-2 gap >= GAP, one of
    its top two under it, such rows <= 0.5 % of the valid rows.  Returns (failures, figures)."""
    fails, figs = [], {}
    pmax, amax, valid = pmax.to(F64), amax.long(), ref["valid"]
    if not (_positive_zero(pmax, ~valid) and (amax[~valid] == -1).all()):
        fails.append("an invalid row is not (+0, -1)")
    want = ref["pmax"]
    e32 = torch.stack([(y - want).abs() for y in ref["evals"]]).amax(0)
    xs = ref["x"].abs()
    floor = 2 * ulp(torch.where(want > 0, want, torch.ones_like(want)), F32) \
        + (2 * ulp(torch.where(xs > 0, xs, torch.ones_like(xs)), F32) + 8 * 2.0 ** -24 * ref["mag"]) * math.log(2) * want
    allowed = torch.maximum(4 * e32, floor)
    err = (pmax - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, INF))
    figs["pmax"] = (err / allowed)[valid].max().item() if valid.any() else 0.0
    if not figs["pmax"] <= 1:
        fails.append(f"pmax: worst row at {figs['pmax']:.3g} times its bar")
    if valid.any():
        a, top2, clear = amax[valid], ref["top2"][valid], ref["gap"][valid] >= GAP
        figs["under_gap"] = float((~clear).sum())
        if not (a[clear] == top2[clear][:, 0]).all():
            fails.append("amax differs on a row with a clear top-2 gap")
        if not ((a[~clear] == top2[~clear][:, 0]) | (a[~clear] == top2[~clear][:, 1])).all():
            fails.append("amax under the gap is not one of the top two")
        if not figs["under_gap"] <= 0.005 * int(valid.sum()):
            fails.append(f"{figs['under_gap']} rows under the gap")
    return fails, figs


def align_q_len(Tq):
    """The q_len vector of the align tests for B = 4: above tq, in the middle, 0, negative."""
    return [Tq + 3, (Tq + 1) // 2, 0, -2]


# ------------------------------------------------------------------ tt2_align_durations
BIG_INDEX = 2 ** 30


def _dc(name, L, B, H, tq, tk, key_len=None, q_len=None, head=None, special=()):
    return dict(name=name, L=L, B=B, H=H, tq=tq, tk=tk, key_len=key_len, q_len=q_len, head=head, special=special)


DUR_CASES = [
    _dc("pairs17", 1, 2, 17, 5, 7, [7, 4], [5, 3]),                      # a second trip of the 16 waves
    _dc("pairs24", 3, 2, 8, 70, 37, [37, 20], [70, 0]),
    _dc("pairs24-fixed", 3, 2, 8, 70, 37, [37, 20], [75, 33], head=(2, 5)),
    _dc("pairs1024", 16, 2, 64, 3, 5, [5, 2], [3, 2]),                   # the limit of the LDS table
    _dc("rows1030", 1, 4, 2, 1030, 40, [40, 33, 40, 40], [1030, 1025, 63, 0]),   # a second trip of the 1024 threads
    _dc("keys2049", 2, 2, 2, 300, 2049, [2049, 2048], [300, 150], special=(2047, 2048)),
    _dc("keys4100", 1, 4, 2, 300, 4100, [4107, 3000, -5, 4097], [300, 299, 300, 64],
        special=(2047, 2048, 2049, 4095, 4096, 4099)),                   # three chunks of 2048 keys
    _dc("keys4100-fixed", 1, 2, 2, 300, 4100, None, None, head=(0, 1), special=(2047, 2048, 2049, 4095, 4096, 4099)),
]


def durations_inputs(c):
    """Hand-made (pmax [L, B, H, tq] float32 values as float64, amax [L, B, H, tq] int64): pmax in
    multiples of 2^-10, so every float32 partial sum of up to 1030 rows is exact in any order; amax
    random keys below tk, with -1 on every seventh row, the case's special keys in turn on every
    fifth, and so also keys at and past key_len[b], which count nowhere.  Two (layer, head) pairs --
    flat index min(17, pairs - 2) and the last -- hold all ones, so mode 0 meets an exact tie of the
    greatest focus.  Rows at and past q_len[b] are NaN and a huge index: they must not be read."""
    L, B, H, tq, tk = (c[k] for k in ("L", "B", "H", "tq", "tk"))
    g = torch.Generator().manual_seed(7 * tq + tk + L * H)
    pmax = torch.randint(0, 1025, (L, B, H, tq), generator=g).to(F64) / 1024
    flat = pmax.transpose(1, 2).reshape(L * H, B, tq)            # a copy: [pair, B, tq]
    for pr in (min(17, L * H - 2), L * H - 1):
        flat[pr] = 1.0
    pmax = flat.view(L, H, B, tq).transpose(1, 2).contiguous()
    amax = torch.randint(0, tk, (L, B, H, tq), generator=g)
    n = torch.arange(tq)
    amax[..., n % 7 == 3] = -1
    for i, t in enumerate(c["special"]):
        amax[..., n % (5 * len(c["special"])) == 5 * i + 1] = t
    ty = R.key_limits(B, tq, c["q_len"])
    past = (n[None, :] >= ty[:, None])[None, :, None, :].expand(L, B, H, tq)
    return pmax.masked_fill(past, float("nan")), amax.masked_fill(past, BIG_INDEX)


def durations_model(c, pmax, amax, mut=None):
    """{'focus' [L, B, H] float32, 'sel' [B, 2], 'sel_focus' [B] float32, 'durations' [B, tk]} in
    numpy from the header: focus = float32(sum over n < Ty_b) * (float32(1) / float32(Ty_b)) (0 if
    Ty_b = 0); mode 0 takes the greatest focus, the lowest flat index slot * heads + head of a tie;
    durations[b, t] counts the rows n < Ty_b of the chosen head with amax == t for t < min(tk,
    key_len[b]) and is 0 at and past key_len[b].  sel and durations come from this focus.
    mut: 'chunk' (the second 2048-key chunk dropped), 'pair' (flat pair 17, index 16, skipped),
    'inv_tq' (1 / tq for 1 / Ty_b), 'past_len' (a count landing at t >= key_len), 'high_tie'."""
    L, B, H, tq, tk = (c[k] for k in ("L", "B", "H", "tq", "tk"))
    ty = R.key_limits(B, tq, c["q_len"]).tolist()
    klim = [tk] * B if c["key_len"] is None else [min(tk, x) for x in c["key_len"]]
    pm, am = pmax.numpy(), amax.numpy()
    focus = np.zeros((L, B, H), dtype=f32)
    for b in range(B):
        if ty[b] > 0:
            total = pm[:, b, :, :ty[b]].sum(-1)
            assert (total == total.astype(f32)).all()
            focus[:, b, :] = total.astype(f32) * (f32(1) / f32(tq if mut == "inv_tq" else ty[b]))
    if mut == "pair" and L * H > 16:
        focus[16 // H, :, 16 % H] = 0
    sel = np.zeros((B, 2), dtype=np.int64)
    dur = np.zeros((B, tk), dtype=np.int64)
    for b in range(B):
        flat = focus[:, b, :].reshape(-1)
        best = c["head"][0] * H + c["head"][1] if c["head"] is not None else int(np.argmax(flat))
        if mut == "high_tie" and c["head"] is None:
            best = int(len(flat) - 1 - np.argmax(flat[::-1]))
        sel[b] = best // H, best % H
        a = am[best // H, b, best % H, :ty[b]]
        keep = (a >= 0) & (a < (tk if mut == "past_len" else klim[b])) & (a < tk)
        if mut == "chunk":
            keep &= ~((a >= 2048) & (a < 4096))
        dur[b] = np.bincount(a[keep], minlength=tk)
    sf = np.array([focus[sel[b, 0], b, sel[b, 1]] for b in range(B)], dtype=f32)
    return {"focus": focus, "sel": sel, "sel_focus": sf, "durations": dur}


def judge_durations(out, want):
    """Everything bit for bit (focus and sel_focus as float32 bits)."""
    fails = []
    for n in ("focus", "sel_focus"):
        if not np.array_equal(np.asarray(out[n], dtype=f32).view(np.int32), want[n].view(np.int32)):
            fails.append(f"{n} differs")
    for n in ("sel", "durations"):
        if not np.array_equal(np.asarray(out[n], dtype=np.int64), want[n]):
            fails.append(f"{n} differs")
    return fails


# ------------------------------------------------------------------ the cases of the guided GPU test
# key_len / q_len of the exact problem per shape of CROSS_TQ_TK: every Ty_b is Tx_b times a power
# of two (assert_indicator), one utterance has Ty_b < tq and one Tx_b < tk wherever the shape allows
# it, klim meets 64, 65 and 128, and entries above tk / tq are cut.
EXACT_LENS = {(1, 1): ([3, 1], [1, 0]), (33, 64): ([33, 16], [33, 32]), (70, 65): ([65, 35], [65, 75]),
              (129, 128): ([128, 64], [128, 128]), (131, 193): ([131, 65], [131, 130]), (257, 37): ([37, 32], [148, 64])}
GUIDE_HEADS = (0, 2, 3)
KAPPAS = (0.5, -2.0)
RANDOM_SIGMA, RANDOM_KAPPA = 0.4, 3.0     # kappa large against a real step's, so the guided term weighs in


def exact_cases():
    """[(id, tq, tk, key_len, Guide)]: the six shapes, guide.heads and kappa taken in turn."""
    out = []
    for i, (tq, tk) in enumerate(R.CROSS_TQ_TK):
        kl, ql = EXACT_LENS[(tq, tk)]
        for j, kappa in enumerate(KAPPAS):
            gd = Guide(tuple(ql), INDICATOR_SIGMA, GUIDE_HEADS[(i + j + 1) % 3], kappa)
            out.append((f"{tq}x{tk}-h{gd.heads}-k{kappa:g}", tq, tk, tuple(kl), gd))
    return out


def random_cases():
    """[(id, tq, tk, key_len, Guide)]: the six shapes, each with one key_len_options entry, one
    q_len option and one guide.heads taken in turn."""
    out = []
    for i, (tq, tk) in enumerate(R.CROSS_TQ_TK):
        kl = R.key_len_options(tk)[i % 4]
        ql = (None, (tq // 2 + 1, tq), (tq + 2, (2 * tq + 2) // 3), (0, tq), (tq + 2, (2 * tq + 2) // 3), (tq // 2 + 1, tq))[i]
        gd = Guide(ql, RANDOM_SIGMA, (2, 3, 2, 3, 2, 0)[i], RANDOM_KAPPA)
        tag = "none" if kl is None else "_".join(str(x) for x in kl)
        out.append((f"{tq}x{tk}-kl_{tag}-h{gd.heads}", tq, tk, None if kl is None else tuple(kl), gd))
    return out


def build_exact_guided(tq, tk, kl, gd):
    """(problem, float64 reference) of the guided selector problem, the pair rows thinned until
    every sum stays in bf16 (assert_exact_guided); the indicator predicate is checked first."""
    last = None
    for pair_frac in (0.5, 0.25, 0.125, 0.0625):
        p = guided_selector_problem(R.BATCH, R.HEADS, tq, tk, list(kl), gd, pair_frac)
        assert_indicator(p, gd)
        ref = guided_ref64(p, gd)
        try:
            assert_exact_guided(ref, p, gd, f"{tq}x{tk}")
            return p, ref
        except AssertionError as e:
            last = e
    raise last
