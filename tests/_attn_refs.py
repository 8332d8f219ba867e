"""References, problem builders and checkers of the fused attention kernels (csrc/attention*.hip),
written from the contract in include/tt2_capi.h.  Everything runs on the CPU; the tensors of a
problem are float64 [B, H, T, 64].  tests/test_attn_refs.py validates this file against torch's
own attention and autograd and proves with mutants that the checkers bite;
tests/test_gpu_attention_exact.py holds the kernels to it.

ref64:   float64, gradients by autograd.
Twin:    the same computation written out (forward, then the backward from the saved LSE as the
         kernels run it), in float64 or float32, rounded to bf16 where the bf16 kernels round:
           forward   P = exp2(s c - m) is summed unrounded into l and rounded for P V; O on store
           backward  P recomputed from the saved LSE, rounded for dV = P^T dO;
                     dS = P (dP - delta) from the unrounded P, rounded for dQ and dK;
                     delta = rowsum(dO * O) from the rounded O; dQ, dK, dV rounded on store,
                     dQ and dK multiplied by `scale` at the store
         (attn_fwd3 / attn_bwd_dq3 / attn_bwd_dkdv3 and the v1 kernels attn_fwd / attn_bwd_dq /
         attn_bwd_dkdv round at the same points, so the twin has no v1 switch).  What it leaves
         out is float32-level: accumulation order, the online rescale, the hardware exp2.
         Twin(torch.float32, None) is the float32 CPU evaluation, the yardstick of the f32 kernels.
"""
import math
from dataclasses import dataclass

import torch

from _misc_refs import ulp

F64 = torch.float64
D = 64
LOG2E = 1.4426950408889634
INF = float("inf")


@dataclass
class Problem:
    q: torch.Tensor          # [B, H, Tq, 64] float64, values representable in the kernel's type
    k: torch.Tensor          # [B, H, Tk, 64]
    v: torch.Tensor          # [B, H, Tk, 64]
    do: torch.Tensor         # [B, H, Tq, 64]
    key_len: object          # list of B ints, or None
    causal: bool
    scale: float             # a float32 value

    @property
    def shape(self):
        B, H, Tq, _ = self.q.shape
        return B, H, Tq, self.k.shape[2]


def key_limits(B, Tk, key_len):
    """min(tk, max(key_len[b], 0)) per batch element (tk without key_len)."""
    if key_len is None:
        return torch.full((B,), Tk, dtype=torch.long)
    return torch.tensor(key_len, dtype=torch.long).clamp(0, Tk)


def visible(B, Tq, Tk, key_len, causal):
    """bool [B, 1, Tq, Tk]: key j is visible to query t iff j < the key limit and, if causal, j <= t."""
    j = torch.arange(Tk)
    vis = (j[None, :] < key_limits(B, Tk, key_len)[:, None])[:, None, None, :].expand(B, 1, Tq, Tk)
    if causal:
        vis = vis & (j[None, :] <= torch.arange(Tq)[:, None])[None, None]
    return vis


def f32_scale(scale):
    return float(torch.tensor(scale, dtype=torch.float32))


# ------------------------------------------------------------------ float64 reference
def ref64(p):
    """{'o', 'lse', 'dq', 'dk', 'dv'} in float64: lse in the log2 domain (+inf on empty rows, whose
    o is 0), the gradients those of sum(o * do) by autograd."""
    B, H, Tq, Tk = p.shape
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (p.q, p.k, p.v))
    vis = visible(B, Tq, Tk, p.key_len, p.causal)
    # natural exp: no log2(e) * ln 2 product on the gradient's way back, so dyadic inputs give
    # dyadic gradients exactly
    x = (q @ k.transpose(-1, -2)) * p.scale
    x = x.masked_fill(~vis, -INF)
    m = x.amax(-1, keepdim=True) if Tk > 0 else torch.full((B, H, Tq, 1), -INF, dtype=F64)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m)).detach()
    e = torch.exp(x - m)
    den = e.sum(-1, keepdim=True)
    live = den > 0
    o = (e / torch.where(live, den, torch.ones_like(den))) @ v
    lse = torch.where(live, m * LOG2E + torch.log2(torch.where(live, den, torch.ones_like(den))),
                      torch.full_like(m, INF))
    (o * p.do).sum().backward()
    return {"o": o.detach(), "lse": lse.detach().squeeze(-1), "dq": q.grad, "dk": k.grad, "dv": v.grad}


# ------------------------------------------------------------------ the twin
class Twin:
    """See the module docstring.  The steps a kernel could get wrong are methods, so that
    tests/test_attn_refs.py can derive deliberately wrong copies (mutants)."""

    def __init__(self, dtype=F64, rnd=torch.bfloat16):
        self.dtype, self.rnd = dtype, rnd

    def r(self, x):
        return x if self.rnd is None else x.to(self.rnd).to(x.dtype)

    def visible(self, p):
        B, H, Tq, Tk = p.shape
        return visible(B, Tq, Tk, p.key_len, p.causal)

    def stats(self, x):
        """Row maximum m (0 on empty rows) and l = sum exp2(x - m) of the masked scores x."""
        m = x.amax(-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        return m, torch.exp2(x - m).sum(-1, keepdim=True)

    def lse(self, m, l):
        safe = torch.where(l > 0, l, torch.ones_like(l))
        return torch.where(l > 0, m + torch.log2(safe), torch.full_like(m, INF))

    def saved(self, o_acc, o, lse):
        """What the forward leaves behind: (O the backward's delta reads, O stored, LSE stored)."""
        return o, o, lse

    def round_ds(self, ds):
        return self.r(ds)

    def __call__(self, p):
        dt = self.dtype
        q, k, v, do = (t.to(dt) for t in (p.q, p.k, p.v, p.do))
        scale = torch.tensor(p.scale, dtype=dt)
        c = scale * torch.tensor(LOG2E, dtype=dt)
        vis = self.visible(p)
        x = ((q @ k.transpose(-1, -2)) * c).masked_fill(~vis, -INF)
        m, l = self.stats(x)
        pf = torch.exp2(x - m)                              # masked: exp2(-inf) = 0
        o_acc = (self.r(pf) @ v) / torch.where(l > 0, l, torch.ones_like(l))
        o_delta, o, lse = self.saved(o_acc, self.r(o_acc), self.lse(m, l))
        pb = torch.exp2(x - lse)                            # empty row: lse = +inf, every p = 0
        dp = do @ v.transpose(-1, -2)
        delta = (do * o_delta).sum(-1, keepdim=True)
        ds = self.round_ds(pb * (dp - delta))
        return {"o": o.to(F64), "lse": lse.squeeze(-1).to(F64),
                "dq": self.r((ds @ k) * scale).to(F64),
                "dk": self.r((ds.transpose(-1, -2) @ q) * scale).to(F64),
                "dv": self.r(self.r(pb).transpose(-1, -2) @ do).to(F64)}


def float32_evaluations(p, orders=8):
    """The float32 CPU evaluation, the yardstick of the f32 kernels, in `orders` accumulation
    orders (the head dimension permuted; the first is the plain one).  One evaluation is one draw
    of the rounding errors, and a block can be a single ill-conditioned number: the last key block
    of the causal 33 x 33 case is one key seen by one query, dK = scale dS Q with dS = p (dP - delta)
    = p (0.916 - 1.115) from terms whose absolute values sum to 61, and the eight orders are off
    there by 9.6e-7 to 8.5e-6.  The worst of them is what float32 can be held to on that block."""
    outs = []
    for i in range(orders):
        perm = torch.arange(D) if i == 0 else torch.randperm(D, generator=torch.Generator().manual_seed(i))
        out = Twin(torch.float32, None)(Problem(p.q[..., perm], p.k[..., perm], p.v[..., perm], p.do[..., perm],
                                                p.key_len, p.causal, p.scale))
        inv = torch.argsort(perm)
        outs.append({n: (x if n == "lse" else x[..., inv]) for n, x in out.items()})
    return outs


# ------------------------------------------------------------------ problems
def _round_in(x, dtype):
    return x.to(dtype).to(F64)


def random_problem(B, H, Tq, Tk, key_len, causal, dtype, seed=0):
    """randn inputs rounded to `dtype`; scale = 0.1, so c = scale log2(e) is no power of two
    times log2(e)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * Tq + Tk)
    q, k, v, do = (_round_in(torch.randn(B, H, T, D, generator=g), dtype) for T in (Tq, Tk, Tk, Tq))
    return Problem(q, k, v, do, key_len, causal, f32_scale(0.1))


def _int_tensor(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def uniform_problem(B, H, Tq, Tk, key_len, causal, dtype=torch.bfloat16, seed=0):
    """Q = 0: every visible key has p = 1, l = the number of visible keys, O = the mean of the
    visible V rows and LSE = log2(count).  K and V in [-2, 2] and dO in {-1, 0, 1} are integers.

    A row whose count is a power of two, 2^k, is exact in the backward as well: p = 2^-k, O is
    the sum of at most 256 small integers over 2^k (a bf16 value), so delta and dS = p (dP - delta)
    are dyadic numbers of a few bits before dS is rounded to bf16 for dQ, and dQ = scale sum dS K
    spans at most 14 + k <= 22 bits: every float32 partial sum is exact in any order.  On those
    rows a kernel that rounds where the twin rounds returns the twin's dQ bit for bit
    (judge_uniform); one that rounds dS elsewhere, or not at all, does not."""
    g = torch.Generator().manual_seed(2000 * seed + 7 * Tq + Tk)
    q = torch.zeros(B, H, Tq, D, dtype=F64)
    k = _int_tensor(g, -2, 2, B, H, Tk, D)
    return Problem(q, k, _int_tensor(g, -2, 2, B, H, Tk, D), _int_tensor(g, -1, 1, B, H, Tq, D), key_len, causal, 0.125)


def visible_counts(p):
    """[B, Tq] number of visible keys of each query row."""
    B, H, Tq, Tk = p.shape
    n = key_limits(B, Tk, p.key_len)[:, None].expand(B, Tq)
    return torch.minimum(n, torch.arange(1, Tq + 1)[None, :]) if p.causal else n


def selector_codes(Tk):
    """K[t] = 64 e[t % 32] + 64 e[32 + (t // 32) % 32]: unique for Tk <= 1024."""
    assert Tk <= 1024
    t = torch.arange(Tk)
    k = torch.zeros(Tk, D, dtype=F64)
    k[t, t % 32] = 64.0
    k[t, 32 + (t // 32) % 32] = 64.0
    return k


def selector_problem(B, H, Tq, Tk, key_len, causal, pair_frac=0.5, seed=0, diag=None):
    """The exact problem.  Each query row copies the code of one visible key (Q = K[t1]) or of two
    that share the first code (Q = K[t1] + K[t2], t2 = t1 mod 32): the best match leads every other
    key by 4096 in the dot product, 4096 * 0.125 * log2(e) = 738 in the log2 domain, so every other
    probability is exactly 0 in float32 (and below 1e-221 in float64).  P is 1, or 1/2 twice;
    O = V[t1] or (V[t1] + V[t2]) / 2; dS = 0 on the one-hot rows and +-(dP1 - dP2) / 4 on the pair
    rows; every partial sum is a small dyadic number.  A row with no visible key gets Q = 0.

    diag = (q_len, share) (non-causal; default None changes nothing): a row n < Ty_b that has a key
    on the guided-attention diagonal, t Ty_b == n Tx_b (Tx_b the visible keys, Ty_b = q_len[b] cut
    to [0, Tq]), takes that key as t1 with probability `share`; t2 is then off the diagonal, so a
    pair row mixes an on-diagonal key with an off-diagonal one (tests/_align_refs.py)."""
    g = torch.Generator().manual_seed(3000 * seed + 7 * Tq + Tk)
    codes = selector_codes(Tk)
    p0 = Problem(torch.zeros(B, H, Tq, D, dtype=F64), codes.expand(B, H, Tk, D).clone(),
                 _int_tensor(g, -2, 2, B, H, Tk, D), _int_tensor(g, -1, 1, B, H, Tq, D), key_len, causal, 0.125)
    nvis = visible_counts(p0)[:, None, :].expand(B, H, Tq)                  # keys 0 .. nvis - 1 are visible
    u = torch.rand(3, B, H, Tq, generator=g, dtype=F64)
    t1 = (u[0] * nvis).long().clamp(max=(nvis - 1).clamp_min(0))
    if diag is not None:
        assert not causal
        q_len, share = diag
        ty = (torch.full((B,), Tq) if q_len is None else torch.tensor(q_len).clamp(0, Tq))[:, None, None]
        n = torch.arange(Tq)[None, None, :]
        td = (n * nvis) // ty.clamp_min(1)
        on = (n < ty) & (nvis > 0) & (td * ty == n * nvis) & (torch.rand(B, H, Tq, generator=g, dtype=F64) < share)
        t1 = torch.where(on, td, t1)
    res = t1 % 32
    cnt = (nvis - res + 31) // 32                                           # visible keys = t1 mod 32
    i2 = (t1 // 32 + 1 + (u[1] * (cnt - 1)).long().clamp(max=(cnt - 2).clamp_min(0))) % cnt.clamp_min(1)
    t2 = res + 32 * i2
    pair = (u[2] < pair_frac) & (cnt >= 2)
    live = nvis > 0
    q = codes[t1] * live[..., None] + codes[t2.clamp(max=max(Tk - 1, 0))] * (pair & live)[..., None]
    assert not (pair & (t1 == t2)).any() and (t2[pair] < nvis[pair]).all()
    p0.q = q
    return p0


def representable(x, dtype=torch.bfloat16):
    """Every element of the float64 x is a value of `dtype` once what neither output type can see
    is dropped: the float64 reference keeps probabilities of 2^-738 where float32 has 0, and they
    leave terms below 1e-200, far under the smallest float32 subnormal (1.4e-45)."""
    x32 = x.to(torch.float32)
    unseen = (x - x32.to(F64)).abs().max().item() if x.numel() else 0.0
    finite = torch.isfinite(x32)
    return unseen < 1e-100 and bool((x32[finite] == x32[finite].to(dtype).to(torch.float32)).all())


def assert_exact_problem(ref, what=""):
    """The suite's 'sum |terms| < 2^24' idiom for the selector problem: O and every gradient of
    the float64 reference are bf16 values, so each kernel must return them bit for bit."""
    for name in ("o", "dq", "dk", "dv"):
        assert representable(ref[name]), f"{what}: {name} of the float64 reference is not bf16-representable " \
                                         f"(max |x| = {ref[name].abs().max().item()}): thin the pair rows"


# ------------------------------------------------------------------ checkers
def ulp_distance(out, ref, dtype):
    """|out - ref| in ulps of `dtype` at |ref|, per element; 0 where both are the same infinity,
    inf where only one of them is finite or out is NaN."""
    out, ref = torch.as_tensor(out).to(F64).cpu(), torch.as_tensor(ref).to(F64).cpu()
    same = out == ref
    fin = torch.isfinite(out) & torch.isfinite(ref)
    d = (out - ref).abs() / ulp(torch.where(fin, ref, torch.ones_like(ref)), dtype)
    return torch.where(same, torch.zeros_like(d), torch.where(fin, d, torch.full_like(d, INF)))


def _blocks(x, rows):
    B, H, T, C = x.shape
    nb = max((T + rows - 1) // rows, 1)
    pad = torch.zeros(B, H, nb * rows, C, dtype=F64)
    pad[:, :, :T] = x.to(F64)
    return pad.view(B, H, nb, rows * C)


def block_errors(out, ref, rows=32):
    """[B, H, blocks] relative L2 error of every 32-row block of a [B, H, T, 64] tensor, one
    wave's unit of work (query blocks of O and dQ, key blocks of dK and dV).  A block whose
    reference is all zero has error 0 if out is all zero there and inf otherwise; NaN / inf in
    out gives inf."""
    o, r = _blocks(torch.as_tensor(out).cpu(), rows), _blocks(torch.as_tensor(ref).cpu(), rows)
    num, den = (o - r).norm(dim=-1), r.norm(dim=-1)
    err = num / torch.where(den > 0, den, torch.ones_like(den))
    err = torch.where(den > 0, err, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, INF)))
    return torch.where(torch.isfinite(num), err, torch.full_like(err, INF))


def worst_ratio(out, ref, yard, factor=2.0, floor=0.0, rows=32, cancel=None):
    """max over the 32-row blocks of err(out, ref) / max(factor * err(yard, ref), floor), <= 1
    passes, every error measured against the same float64 reference on the same block.  `yard` is
    the twin (factor 2), or the list of float32 CPU evaluations of float32_evaluations() (factor 4,
    floor 2 f32 ulp), whose error on a block is the worst of the list's.  A block whose reference
    is all zero passes only if out is all zero there.

    cancel = (live, bound): live is a bool [B, 1 or H, T] of the rows that have a visible
    (query, key) pair.  A zero-reference block made of such rows is zero by cancellation, not by
    masking (a row with a single visible key has dS = p (dP - delta) = 0 identically), where a
    float32 kernel leaves rounding noise; there max |out| <= bound is asked instead."""
    ek = block_errors(out, ref, rows)
    ey = torch.stack([block_errors(y, ref, rows) for y in (yard if isinstance(yard, (list, tuple)) else [yard])]).amax(0)
    allowed = torch.clamp_min(factor * ey, floor)
    ratio = torch.where(ek == 0, torch.zeros_like(ek), ek / allowed)       # 0 / 0 passes, x / 0 does not
    if cancel is not None:
        live, bound = cancel
        B, H, T, _ = ref.shape
        lv = _blocks(live.expand(B, H, T)[..., None].to(F64), rows).amax(-1) > 0
        zero_ref = _blocks(torch.as_tensor(ref).cpu(), rows).norm(dim=-1) == 0
        amax = torch.nan_to_num(_blocks(torch.as_tensor(out).cpu(), rows).abs(), nan=INF).amax(-1)
        ratio = torch.where(zero_ref & lv, amax / bound, ratio)
    return ratio.max().item()


def cancel_bound(p):
    """A-priori bound on what a float32 kernel may leave in dQ / dK where dS cancels exactly:
    dP and delta are each a float32 sum of 64 products, off by at most gamma_64 = 64 * 2^-24 times
    sum |dO_d V_d| (Higham, Accuracy and Stability, 3.1), p <= 1, and the row is then multiplied by
    one K (or Q) row and by scale.  Store rounding is relative and cannot exceed it by more than
    2^-8."""
    s = (p.do.abs() @ p.v.abs().transpose(-1, -2)).max().item() if p.k.shape[2] else 0.0
    big = max(p.k.abs().max().item() if p.k.numel() else 0.0, p.q.abs().max().item(), 1.0)
    return 2 * 64 * 2.0 ** -24 * s * big * p.scale * (1 + 2.0 ** -8) + 1e-300


def live_rows(p):
    """(query rows with a visible key [B, 1, Tq], keys visible to some query [B, 1, Tk])."""
    B, H, Tq, Tk = p.shape
    vis = visible(B, Tq, Tk, p.key_len, p.causal)
    return vis.any(-1), vis.any(-2)


def old_global_bar(out, ref):
    """The bars of tests/test_gpu_attention.py: relative Frobenius norm over the whole tensor,
    < 1e-2 for O and < 2e-2 for dQ, dK, dV.  True if they accept `out`."""
    def rel(a, b):
        return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
    return rel(out["o"], ref["o"]) < 1e-2 and all(rel(out[n], ref[n]) < 2e-2 for n in ("dq", "dk", "dv"))


def lse_ratio(lse, ref, yard=None, unit=False):
    """max |lse - ref| / max(4 f32 ulp at |ref| (at max(|ref|, 1) if `unit`), 4 * the worst error of
    `yard`, the float32 CPU evaluation's LSE), <= 1 passes; +inf must match exactly."""
    lse, ref = torch.as_tensor(lse).to(F64).cpu(), ref.to(F64)
    if lse.numel() == 0:
        return 0.0
    if not torch.equal(torch.isposinf(lse), torch.isposinf(ref)) or torch.isnan(lse).any():
        return INF
    fin = torch.isfinite(ref)
    at = ref.abs().clamp_min(1.0) if unit else ref.abs()
    allowed = 4 * ulp(torch.where(fin, at, torch.ones_like(at)), torch.float32)
    if yard is not None and fin.any():
        e32 = max((y.to(F64) - ref)[fin].abs().max().item() for y in (yard if isinstance(yard, (list, tuple)) else [yard]))
        allowed = allowed.clamp_min(4 * e32)
    r = torch.where(fin, (lse - ref).abs() / allowed, torch.zeros_like(ref))
    return r.max().item()


def uniform_o(p):
    """O of the uniform problem in closed form: the exact integer sum of the visible V rows, divided
    once by their number (the autograd reference sums v / n and is off by float64 rounding, which
    matters where the mean is 0)."""
    B, H, Tq, Tk = p.shape
    vis = visible(B, Tq, Tk, p.key_len, p.causal).to(F64)
    return (vis @ p.v) / visible_counts(p).clamp_min(1)[:, None, :, None]


def log2_count_lse(p):
    """LSE of the uniform problem from the counts alone: log2(visible keys), +inf on empty rows."""
    n = visible_counts(p).to(F64)
    B, H, Tq, _ = p.shape
    return torch.where(n > 0, torch.log2(n.clamp_min(1)), torch.full_like(n, INF))[:, None, :].expand(B, H, Tq)


assert math.isclose(LOG2E, 1 / math.log(2))


# ------------------------------------------------------------------ the shapes of the GPU test
# Each is the smallest that reaches its edge of the tile structure (32 rows per wave, 64 or 128
# rows per work group, 64-key tiles walked as two 32-key halves, two LDS buffers taken in turn).
BATCH, HEADS = 2, 3        # bh / H and bh % H both matter
CAUSAL_T = (1, 31, 33, 64, 65, 128, 129, 193, 257)     # one partly filled wave; 1 .. 5 key tiles
CROSS_TQ_TK = ((1, 1), (33, 64), (70, 65), (129, 128), (131, 193), (257, 37))


def key_len_options(Tk):
    half = Tk // 2
    if half % 32 == 0:
        half += 1
    return (None, [Tk + 5, half], [0, Tk], [-3, 1])


def cases(rot):
    """[(id, Tq, Tk, causal, key_len)]: every shape with one of its four key_len options, taken in
    turn from option `rot` on (each problem passes another rot, so a shape meets three of them)."""
    shapes = [(T, T, True) for T in CAUSAL_T] + [(tq, tk, False) for tq, tk in CROSS_TQ_TK]
    out = []
    for i, (tq, tk, causal) in enumerate(shapes):
        kl = key_len_options(tk)[(i + rot) % 4]
        tag = "none" if kl is None else "_".join(str(x) for x in kl)
        out.append((f"{'causal' if causal else 'cross'}-{tq}x{tk}-kl_{tag}", tq, tk, causal, kl))
    return out


SELECTOR_ROT, UNIFORM_ROT, RANDOM_ROT = 1, 3, 0


# ------------------------------------------------------------------ the bars, one judge per problem
# Each judge takes what a kernel (or a mutant of the twin) returned as float64 [B, H, T, 64]
# tensors {'o', 'lse' [B, H, Tq], 'dq', 'dk', 'dv'} and returns (failures, figures): the list of
# bars missed, in words, and the measured worst ratios (<= 1 passes) for `pytest -s`.
GRADS = ("dq", "dk", "dv")
F32_FLOOR = 2 * 2.0 ** -23          # 2 f32 ulp as a relative block error


def _first_diff(a, b):
    i = (a != b).nonzero()[0].tolist()
    return f"first at {i}: got {a[tuple(i)].item()!r}, expected {b[tuple(i)].item()!r} ({int((a != b).sum())} differ)"


def judge_selector(out, ref, p, dtype):
    """Exact: O, dQ, dK, dV equal the float64 reference cast to `dtype` bit for bit; the LSE is
    within 4 f32 ulp of |ref| (c is rounded to f32 once and 8192 c or 12288 c once more, log2f adds
    1 ulp and the add 1/2) and exactly +inf on the empty rows."""
    fails, figs = [], {}
    for n in ("o",) + GRADS:
        want = ref[n].to(dtype).to(F64)
        if not torch.equal(out[n], want):
            fails.append(f"{n} differs from the float64 reference: {_first_diff(out[n], want)}")
    empty, dead = (~x for x in live_rows(p))
    B, H, Tq, Tk = p.shape
    if (out["o"] * empty.expand(B, H, Tq)[..., None] != 0).any():
        fails.append("an empty row of O is not 0")
    for n in ("dk", "dv"):
        if (out[n] * dead.expand(B, H, Tk)[..., None] != 0).any():
            fails.append(f"{n} of a key no query sees is not 0")
    figs["lse"] = lse_ratio(out["lse"], ref["lse"])
    if not figs["lse"] <= 1:
        fails.append(f"lse ratio {figs['lse']:.3g} (4 f32 ulp)")
    return fails, figs


def _block_bars(out, ref, yard, p, dtype, names, fails, figs):
    factor, floor = (2.0, 0.0) if dtype == torch.bfloat16 else (4.0, F32_FLOOR)
    qlive, klive = live_rows(p)
    cancel = {"dq": (qlive, cancel_bound(p)), "dk": (klive, cancel_bound(p))}
    for n in names:
        ys = [y[n] for y in yard] if isinstance(yard, (list, tuple)) else yard[n]
        figs[n] = worst_ratio(out[n], ref[n], ys, factor, floor, cancel=cancel.get(n))
        if not figs[n] <= 1:
            fails.append(f"{n}: worst 32-row block at {figs[n]:.3g} times its bar")


def judge_uniform(out, ref, yard, p, dtype):
    """Forward, bf16: O within 1 bf16 ulp of RN_bf16(ref) (the f32 error before the store is about
    2^-22 against a half ulp of 2^-9: only near-ties land on the neighbour) and equal where the
    count of visible keys is a power of two; f32: within 4 f32 ulp.  LSE within 4 f32 ulp of
    max(|ref|, 1).  The backward goes under the block bars, against `yard`, and on the rows whose
    count is a power of two dQ equals the twin's bit for bit (uniform_problem: exact arithmetic up
    to the one rounding of dS; in f32 nothing is rounded and it is the float64 reference's)."""
    fails, figs = [], {}
    B, H, Tq, Tk = p.shape
    o_ref = uniform_o(p)
    if dtype == torch.bfloat16:
        want = o_ref.to(dtype).to(F64)
        figs["o_ulp"] = ulp_distance(out["o"], want, dtype).max().item() if want.numel() else 0.0
        n = visible_counts(p)
        pow2 = ((n & (n - 1)) == 0)[:, None, :, None].expand(B, H, Tq, D)      # 0 counts: the empty rows
        if not torch.equal(out["o"][pow2], want[pow2]):
            fails.append("O differs where the count is a power of two")
        if not figs["o_ulp"] <= 1:
            fails.append(f"O is {figs['o_ulp']:.3g} bf16 ulp from RN(ref)")
    else:
        figs["o_ulp"] = ulp_distance(out["o"], o_ref, dtype).max().item()
        if not figs["o_ulp"] <= 4:
            fails.append(f"O is {figs['o_ulp']:.3g} f32 ulp from the reference")
    figs["lse"] = lse_ratio(out["lse"], ref["lse"], unit=True)
    if not figs["lse"] <= 1:
        fails.append(f"lse ratio {figs['lse']:.3g} (4 f32 ulp of max(|ref|, 1))")
    _block_bars(out, ref, yard, p, dtype, GRADS, fails, figs)
    n = visible_counts(p)
    rows = ((n > 0) & ((n & (n - 1)) == 0))[:, None, :].expand(B, H, Tq)
    want = Twin(F64, None if dtype == torch.float32 else dtype)(p)["dq"][rows]
    figs["dq_pow2_rows"] = float(rows.sum())
    if not torch.equal(out["dq"][rows], want):
        fails.append(f"dQ differs from the twin on the rows with a power-of-two count: {_first_diff(out['dq'][rows], want)}")
    return fails, figs


def judge_random(out, ref, yard, yard32_lse, p, dtype):
    """Every 32-row block of O, dQ, dK, dV: err(out, ref64) <= 2 err(twin, ref64) in bf16,
    <= max(4 err(float32 CPU evaluations), 2 f32 ulp) in f32; LSE within 4 f32 ulp of max(|ref|, 1)
    or 4 times the float32 CPU evaluation's worst LSE error."""
    fails, figs = [], {}
    _block_bars(out, ref, yard, p, dtype, ("o",) + GRADS, fails, figs)
    figs["lse"] = lse_ratio(out["lse"], ref["lse"], yard32_lse, unit=True)
    if not figs["lse"] <= 1:
        fails.append(f"lse ratio {figs['lse']:.3g}")
    return fails, figs


def show(figs):
    return ", ".join(f"{k} {v:.3f}" for k, v in figs.items())
