"""Problems, float64 references, bars and case lists of the GEMM kernels (tt2_gemm, tt2_gemm_grouped),
written from the contract in include/tt2_capi.h.  Everything here runs on the CPU.
tests/test_gemm_refs.py validates this file (a triple loop, F.conv1d, a tile model and its mutants);
tests/test_gpu_gemm_exact.py holds every kernel family to it.

    C[m, n] = epi(alpha * sum_k A(m, k) B(n, k))
    epi: * alpha, + bias[n], + res[m, n], act, gate (gate[m, n] != 0 ? * gate_scale : 0),
         dropout (index m * n + col), + beta * C0[m, n]                      (epi_value's order)

exact problem   A, B in {-1, 0, +1}, every epilogue input a small integer, every factor a power of
                two: each f32 partial sum is an exact integer in any order and under any split, and
                the result is a value of the output type.  A kernel returns the float64 reference
                bit for bit or it is wrong.
random problem  N(0, 1) operands rounded to the input type, B scaled by k^-0.5.  The bar is per
                element: E = 2 k u |A| |B|^T (u = 2^-24: k-term accumulation in any order, under one
                ulp of error per operation, so round-to-nearest and truncation are both inside it),
                pushed through the epilogue (1-Lipschitz steps, known factors), plus 8 u times the
                magnitudes of the epilogue's own terms, plus 4 f32 ulp of the result for tanh.  An
                f32 output lies within E of the reference; a bf16 (f16) output is one of the values
                of its type in [round(ref - E), round(ref + E)].
"""
import math
from collections import namedtuple
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from _misc_refs import ulp
from tt2_oracle import dropout_keep

F64, F32, BF16, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
U = 2.0 ** -24
NAN = float("nan")
INF = float("inf")
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
# guards: one row before, two after; pad columns per buffer, all different so that a row length
# taken from the wrong buffer lands on NaN (each keeps 16-B aligned rows in bf16 and f32)
ROW_BEFORE, ROW_AFTER, VEC_GUARD = 1, 2, 4
PAD_C, PAD_RES, PAD_GATE, PAD_OPERAND = 8, 16, 24, 8
KS, CONV_PAD, CONV_BATCH = 5, 2, 3          # Conv1d(k5, pad 2) over three sequences
V8_RING = 4                                 # G8_RING of csrc/gemm_v8.hip (test_gemm_refs.py checks the source)


@dataclass
class Problem:
    a: torch.Tensor            # float64 logical [m, k]; with a_conv the sequence rows [m, C]
    b: torch.Tensor            # float64 logical [n, k]; with b_conv the sequence rows [k, C]
    m: int
    n: int
    k: int
    trans_a: bool = False      # layout flags: how the launch stores a / b (the values do not change)
    trans_b: bool = False
    a_conv: object = None      # (T, C, pad) or None
    b_conv: object = None
    in_dtype: object = BF16
    out_dtype: object = BF16
    alpha: float = 1.0
    bias: object = None        # [n]
    res: object = None         # [m, n]
    res_dtype: object = BF16
    act: int = ACT_NONE
    gate: object = None        # [m, n], >= 0
    gate_dtype: object = BF16
    gate_scale: float = 1.0
    drop: object = None        # (seed, site, p)
    beta: float = 0.0
    c0: object = None          # [m, n], the initial C of a beta request
    splits: int = 1
    ksum0: object = None       # [m]: a weight-gradient request's initial bias sums
    ksum_beta: float = 0.0


def conv_expand(x, T, pad, taps):
    """im2col of channels-last sequences: x [B T, C] -> [B T, taps C], column tap * C + c of row
    (b, t) = x[b, t + tap - pad, c], zero outside [0, T) of its own sequence."""
    M, C = x.shape
    xp = F.pad(x.view(M // T, T, C), (0, 0, pad, taps - 1 - pad))
    return torch.cat([xp[:, t:t + T] for t in range(taps)], dim=2).reshape(M, taps * C)


def logical(p):
    """(A [m, k], B [n, k]) in float64, conv operands expanded."""
    a, b = p.a, p.b
    if p.a_conv:
        T, C, pad = p.a_conv
        a = conv_expand(a, T, pad, p.k // C)
    if p.b_conv:
        T, C, pad = p.b_conv
        b = conv_expand(b, T, pad, p.n // C).t()
    assert a.shape == (p.m, p.k) and b.shape == (p.n, p.k), (a.shape, b.shape, p.m, p.n, p.k)
    return a, b


def stored(p):
    """(a, b) as the launch lays them out (tt2_capi.h): A(m, k) = a[m * lda + k], or a[k * lda + m]
    with trans_a; B likewise; a conv operand is its sequence rows, ld == C."""
    a = p.a if p.a_conv or not p.trans_a else p.a.t()
    b = p.b if p.b_conv or not p.trans_b else p.b.t()
    return a.contiguous(), b.contiguous()


def drop_scale(prob):
    """1 / (1 - p) as the f32 the launch passes."""
    return float(np.float32(1.0 / (1.0 - prob)))


def keep_mask(p):
    seed, site, prob = p.drop
    return torch.from_numpy(dropout_keep(seed, site, p.m * p.n, prob)).view(p.m, p.n)


def _epilogue(p, acc, e_acc):
    """(value, bound) of the epilogue on the float64 products `acc` whose error bound is `e_acc`."""
    v, e = p.alpha * acc, abs(p.alpha) * e_acc
    mag = v.abs()                                    # magnitudes of the terms of the epilogue's own f32 operations
    if p.bias is not None:
        v, mag = v + p.bias[None, :], mag + p.bias.abs()[None, :]
    if p.res is not None:
        v, mag = v + p.res, mag + p.res.abs()
    extra = torch.zeros_like(v)
    if p.act == ACT_RELU:
        v = v.clamp_min(0.0)
    elif p.act == ACT_TANH:
        v = torch.tanh(v)
        extra = 4 * ulp(v, F32)
    f = torch.ones_like(v)
    if p.gate is not None:
        f = f * torch.where(p.gate != 0, torch.full_like(v, p.gate_scale), torch.zeros_like(v))
    if p.drop is not None:
        f = f * torch.where(keep_mask(p), torch.full_like(v, drop_scale(p.drop[2])), torch.zeros_like(v))
    v, e, mag, extra = torch.where(f != 0, v * f, torch.zeros_like(v)), e * f, mag * f, extra * f
    if p.beta != 0.0:
        v, mag = v + p.beta * p.c0, mag + (p.beta * p.c0).abs()
    return v + 0.0, e + 8 * U * mag + extra          # + 0.0: no negative zero


def ref64(p, bound=False):
    """(C [m, n], a_ksum [m] or None) in float64; with bound=True also the per-element bar E."""
    a, b = logical(p)
    acc = a @ b.t()
    e_acc = 2 * p.k * U * (a.abs() @ b.abs().t())
    c, e = _epilogue(p, acc, e_acc)
    ksum = None if p.ksum0 is None else p.ksum_beta * p.ksum0 + a.sum(1)
    return (c, ksum, e) if bound else (c, ksum)


# ------------------------------------------------------------------ epilogue sets and cases
# name -> (bias, res dtype, act, gate dtype, dropout, alpha != 1, beta)
EPIS = {
    "none": (False, None, ACT_NONE, None, False, False, False),
    "bias": (True, None, ACT_NONE, None, False, False, False),
    "brd": (True, None, ACT_RELU, None, True, False, False),         # bias + ReLU + dropout
    "res16": (False, BF16, ACT_NONE, None, False, False, False),
    "res32": (False, F32, ACT_NONE, None, False, False, False),
    "gate": (False, None, ACT_NONE, BF16, False, False, False),      # the ReLU gate of an activation gradient
    "all": (True, BF16, ACT_RELU, F32, True, True, False),           # bias + residual + ReLU + gate + dropout + alpha
    "beta": (False, None, ACT_NONE, None, False, False, True),       # f32 C
    "tanh": (False, None, ACT_TANH, None, False, False, False),      # f32 C, random problem only
}
EPI_NAMES = list(EPIS)
EXACT_EPIS = [e for e in EPI_NAMES if e != "tanh"]
BF16_OUT_EPIS = [e for e in EXACT_EPIS if e != "beta"]

# variant: the kernel_variant forced; conv: None or (kind, T, cin, cout); ksum: fused bias sums
Case = namedtuple("Case", "variant in_dt m n k ta tb epi splits conv ksum", defaults=(1, None, False))
KERNEL = {1: 1, 2: 2, 3: 3, 13: 13, 14: 13, 15: 15, 16: 16, 17: 17}       # variant -> tt2_gemm_plan code
FAMILY = {1: "v1", 2: "v2", 3: "skinny", 13: "v7", 15: "v8", 16: "v10", 17: "v11"}   # plan code -> family
_DT = {F32: "f32", BF16: "bf16", F16: "f16"}


def out_dtype(c):
    """f32 for f32 operands, a beta or tanh request and a weight gradient; else the operands' type."""
    return F32 if c.in_dt == F32 or c.epi in ("beta", "tanh") or (c.conv and c.conv[0] == "wgrad") or c.ksum else c.in_dt


def case_id(c):
    s = f"var{c.variant}-{_DT[c.in_dt]}-{c.m}x{c.n}x{c.k}-{'T' if c.ta else 'N'}{'N' if c.tb else 'T'}-{c.epi}"
    if c.splits > 1:
        s += f"-s{c.splits}"
    if c.conv:
        s += f"-{c.conv[0]}{c.conv[1]}"
    return s + ("-ksum" if c.ksum else "")


def eligible(c):
    """Whether the family forced by c.variant takes the request, from gemm_plan's and the route's
    conditions (csrc/gemm.hip) for the aligned buffers the test launches with.  Variant 0 takes
    everything."""
    bias, res, act, gate, drop, _, beta = EPIS[c.epi]
    out = out_dtype(c)
    a_inner, b_inner = (c.m if c.ta else c.k), (c.n if c.tb else c.k)
    kind = c.conv[0] if c.conv else None
    a_conv, b_conv = kind in ("fwd", "dgrad"), kind == "wgrad"
    T = c.conv[1] if c.conv else 0
    conv_c = {None: 0, "fwd": c.conv[2] if c.conv else 0, "dgrad": c.conv[3] if c.conv else 0,
              "wgrad": c.conv[2] if c.conv else 0}[kind]
    dma = c.in_dt == BF16 and a_inner % 8 == 0 and b_inner % 8 == 0          # the LDS-DMA kernels
    v7 = dma and (not c.conv or (T >= 64 and conv_c >= 64))
    if c.ksum and not (dma and c.variant != 1 and c.ta and not a_conv):
        return False
    if c.variant in (0, 1):
        return True
    if c.variant == 3:
        return c.in_dt in (BF16, F16) and c.m <= 64 and not c.ta and not c.tb and c.k % 8 == 0 and not c.conv \
            and c.splits == 1
    if c.in_dt != BF16:
        return False
    if c.variant == 2:
        return dma
    if c.variant in (13, 14):
        return v7
    if c.variant == 15:    # (v8 takes a split-K request and runs it unsplit)
        return dma and out == BF16 and not c.ksum and not c.ta and not b_conv and c.n % 8 == 0 and c.m >= 64
    plain = out == BF16 and c.splits == 1 and not c.ksum
    no_xtra = not beta and act != ACT_TANH
    if c.variant == 16:
        return v7 and plain and not c.ta and not c.tb and not c.conv and c.n % 256 == 0 and c.k % 64 == 0 \
            and no_xtra and res is None and gate is None
    if c.variant == 17:
        ok = v7 and plain and not c.ta and not c.conv and c.n % 128 == 0 and c.k % 64 == 0 and no_xtra
        if c.tb:       # an activation gradient: a bf16 residual or gate alone
            return ok and not bias and act == ACT_NONE and not drop and not (res is not None and gate is not None) \
                and res in (None, BF16) and gate in (None, BF16)
        return ok and res is None and gate is None
    raise ValueError(c.variant)


LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]    # (trans_a, trans_b); ids: NT = both K-contiguous
MN_BIG = [(40, 24), (136, 264), (264, 136), (520, 264)]
K_BIG = [8, 64, 72, 128, 192, 200, 256, 448, 1000]   # < 1 step, 1, 1 + tail, 2, 3, 3 + tail, 4, 7 steps, 15 + tail


def _big(variant, in_dt):
    """v1, v2, v7: tiles 128 x 128 / 256 x 128, K steps 32 / 64, three stages."""
    out = []
    for i, k in enumerate(K_BIG):                                    # every k, tails in m and n
        out.append(Case(variant, in_dt, 520, 264, k, False, False, EXACT_EPIS[i % len(EXACT_EPIS)]))
    for m, n in MN_BIG[:3]:
        out += [Case(variant, in_dt, m, n, 72, False, False, "bias"), Case(variant, in_dt, m, n, 200, False, False, "all")]
    for ta, tb in LAYOUTS:                                           # every layout
        out += [Case(variant, in_dt, 264, 136, 200, ta, tb, e) for e in ("none", "all")]
    for e in EPI_NAMES:                                              # every epilogue set, forward and dgrad layout
        out += [Case(variant, in_dt, 136, 264, 192, False, tb, e) for tb in (False, True)]
    for sp in (2, 3, 7):                                             # uneven split-K
        for k in (200, 1000):
            out += [Case(variant, in_dt, 136, 264, k, False, False, "all", sp),
                    Case(variant, in_dt, 136, 264, k, True, True, "beta", sp)]
    # a split with no K step: the launchers re-derive the count from 64-deep (v1: 32-deep) slices,
    # ceil(64 / 64) = 1 (v1: 2) splits run and no empty slab exists
    out.append(Case(variant, in_dt, 136, 264, 64, False, False, "bias", 3))
    # n = 81: rows of C, residual and gate that are not 16-B aligned take the per-element epilogue
    out += [Case(variant, in_dt, 137, 81, 200, False, False, e) for e in ("all", "beta", "res16", "brd")]
    out.append(Case(variant, in_dt, 137, 81, 200, False, False, "all", 3))
    return out


def _v11():
    out = []
    for m, n in [(264, 128), (520, 384)]:
        out += [Case(17, BF16, m, n, k, False, False, ("none", "bias", "brd")[i % 3])
                for i, k in enumerate([64, 128, 192, 256, 448])]
    out += [Case(17, BF16, 264, 128, 192, False, True, e) for e in ("none", "res16", "gate")]
    out += [Case(17, BF16, 520, 384, 448, False, True, "res16"), Case(17, BF16, 264, 128, 192, False, False, "brd")]
    return out


def _v10():
    out = []
    for j, (m, n) in enumerate([(264, 256), (520, 512)]):
        out += [Case(16, BF16, m, n, k, False, False, ("none", "bias", "brd")[(i + j) % 3])
                for i, k in enumerate([64, 128, 192, 256, 320, 384, 448])]     # across the 5-slot ring's wrap
    return out


def _v8():
    ks = [8, 72] + [64 * r + 8 for r in (V8_RING - 1, V8_RING, V8_RING + 1)]
    out, i = [], 0
    for m, n in [(64, 8), (72, 72), (200, 136)]:
        for k in ks:
            out.append(Case(15, BF16, m, n, k, False, False, BF16_OUT_EPIS[i % len(BF16_OUT_EPIS)]))
            i += 1
    for k in (72, 64 * V8_RING + 8):
        out += [Case(15, BF16, 200, 136, k, False, True, e) for e in ("none", "all", "res16", "gate")]
    out += [Case(15, BF16, 200, 136, 192, False, False, e) for e in BF16_OUT_EPIS]
    out.append(Case(15, BF16, 200, 136, 200, False, False, "all", 3))     # v8 has no split-K: it runs this unsplit
    return out


def _skinny():
    out, i = [], 0
    for dt in (BF16, F16):
        for m in (1, 17, 64):
            for n in (16, 24, 88):
                for k in (8, 80, 520, 2104):
                    out.append(Case(3, dt, m, n, k, False, False, EPI_NAMES[i % len(EPI_NAMES)]))
                    i += 1
    return out


def _auto():
    return [Case(0, BF16, 40, 24, 72, False, False, "bias"), Case(0, BF16, 520, 264, 200, False, False, "brd"),
            Case(0, BF16, 520, 264, 200, True, True, "beta"), Case(0, BF16, 264, 256, 128, False, False, "bias"),
            Case(0, BF16, 264, 136, 200, False, True, "gate"), Case(0, F32, 136, 264, 72, False, False, "all"),
            Case(0, BF16, 136, 264, 1000, False, False, "all", 3), Case(0, BF16, 136, 264, 192, False, False, "tanh"),
            Case(0, BF16, 264, 136, 200, True, False, "res32")]


def _conv():
    """a_conv forward and dgrad, the b_conv weight gradient: T in {37, 64, 100}, C in {64, 80}."""
    out = []
    for variant, in_dt in [(1, F32), (1, BF16), (2, BF16), (13, BF16), (14, BF16), (15, BF16), (0, BF16)]:
        for T in (37, 64, 100):
            M = CONV_BATCH * T
            for cin, cout in [(64, 80), (80, 64)]:
                out.append(Case(variant, in_dt, M, cout, KS * cin, False, False, "bias", 1, ("fwd", T, cin, cout)))
                out.append(Case(variant, in_dt, M, cin, KS * cout, False, False, "none", 1, ("dgrad", T, cin, cout)))
                for sp in (1, 3):
                    out.append(Case(variant, in_dt, cout, KS * cin, M, True, True, "none", sp, ("wgrad", T, cin, cout),
                                    ksum=variant != 1 and sp == 3))
            out.append(Case(variant, in_dt, M, 80, KS * 64, False, False, "brd", 2, ("fwd", T, 64, 80)))
    return out


T_GROUP = 100
# grouped weight gradients, (n_out, n_in, conv channels or 0): dW[n_out, n_in] = dY^T X over
# k = 3 * 100 tokens (four K steps and a tail of 44); a problem below 256 rows first, conv-B
# problems, ragged and full tiles
GROUP = [(200, 64, 0), (136, 5 * 64, 64), (512, 264, 0), (72, 72, 0), (1536, 128, 0), (264, 136, 0), (80, 5 * 80, 80),
         (520, 512, 0)]


def group_cases(count, splits):
    """The first `count` problems of GROUP as weight-gradient cases with fused bias sums."""
    return [Case(0, BF16, n_out, n_in, CONV_BATCH * T_GROUP, True, True, "none", splits,
                 ("wgrad", T_GROUP, cc, n_out) if cc else None, True) for n_out, n_in, cc in GROUP[:count]]


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if c not in seen and eligible(c):
            seen.add(c)
            out.append(c)
    return out


CASES = {
    "v1-f32": _unique(_big(1, F32)), "v1-bf16": _unique(_big(1, BF16)), "v2": _unique(_big(2, BF16)),
    "v7-13": _unique(_big(13, BF16)), "v7-14": _unique(_big(14, BF16)), "v8": _unique(_v8()), "v10": _unique(_v10()),
    "v11": _unique(_v11()), "skinny": _unique(_skinny()), "auto": _unique(_auto()),
}
ALL_CASES = [c for group in CASES.values() for c in group]
EXACT_CASES = [c for c in ALL_CASES if c.epi != "tanh"]
RANDOM_CASES = ALL_CASES
CONV_CASES = _unique(_conv())


# ------------------------------------------------------------------ problem builders
def _seed(c, kind):
    conv = 0 if not c.conv else 1 + ("fwd", "dgrad", "wgrad").index(c.conv[0]) + 3 * c.conv[1]
    return (c.m * 7919 + c.n * 104729 + c.k * 31 + EPI_NAMES.index(c.epi) * 17 + conv * 1009 + kind) % (2 ** 31 - 1)


def problem_key(c):
    """What the values of a case's problem depend on: variants, layouts and splits share them."""
    return (c.in_dt, c.m, c.n, c.k, c.epi, c.conv, c.ksum)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _ternary(g, shape, k):
    keep = torch.rand(shape, generator=g, dtype=F64) < min(1.0, math.sqrt(144.0 / k))
    sign = torch.randint(0, 2, shape, generator=g).to(F64) * 2 - 1
    return sign * keep


def _operand_shapes(c):
    """Shapes of Problem.a / .b and the conv descriptors of a case."""
    if not c.conv:
        return (c.m, c.k), (c.n, c.k), None, None
    kind, T, cin, cout = c.conv
    if kind == "fwd":
        return (c.m, cin), (c.n, c.k), (T, cin, CONV_PAD), None
    if kind == "dgrad":
        return (c.m, cout), (c.n, c.k), (T, cout, CONV_PAD), None
    return (c.m, c.k), (c.k, cin), None, (T, cin, CONV_PAD)


def make_problem(c, exact):
    """The exact or the random problem of a case (see the module docstring)."""
    g = torch.Generator().manual_seed(_seed(c, 0 if exact else 1))
    sa, sb, a_conv, b_conv = _operand_shapes(c)
    bias, res, act, gate, drop, alpha, beta = EPIS[c.epi]
    m, n, out = c.m, c.n, out_dtype(c)
    if exact:
        a, b = _ternary(g, sa, c.k), _ternary(g, sb, c.k)
    else:
        a = torch.randn(sa, generator=g, dtype=F64).to(c.in_dt).to(F64)
        b = (torch.randn(sb, generator=g, dtype=F64) * c.k ** -0.5).to(c.in_dt).to(F64)
    p = Problem(a, b, m, n, c.k, c.ta, c.tb, a_conv, b_conv, c.in_dt, out, act=act, splits=c.splits)

    def values(lo, hi, dtype, *shape):
        return _ints(g, lo, hi, *shape) if exact else torch.randn(shape, generator=g, dtype=F64).to(dtype).to(F64)
    if alpha:
        p.alpha = 0.5 if exact else 0.75
    if bias:
        p.bias = values(-4, 4, F32, n)
    if res is not None:
        p.res, p.res_dtype = values(-8, 8, res, m, n), res
    if gate is not None:
        on = torch.rand((m, n), generator=g, dtype=F64) < 0.5
        p.gate = (_ints(g, 1, 3, m, n) if exact else values(0, 0, gate, m, n).abs() + 2.0 ** -6) * on
        p.gate_dtype, p.gate_scale = gate, 2.0 if exact else 1.5
        p.gate = p.gate.to(gate).to(F64)
    if drop:
        p.drop = (1234 + c.k, 77, 0.5 if exact else 0.25)
    if beta:
        p.beta, p.c0 = 1.0, values(-8, 8, out, m, n)
    if c.ksum:
        p.ksum0, p.ksum_beta = (2 * _ints(g, -4, 4, m) if exact else values(0, 0, F32, m)), 0.5
    return p


# ------------------------------------------------------------------ the bars
def representable(x, dtype):
    return bool((x.to(dtype).to(F64) == x).all()) and bool(torch.isfinite(x).all())


def assert_exact_problem(p, ref, ksum=None):
    """A condition of the exact test, not a tolerance: the float64 reference is a value of the
    output type (the bias sums of f32), so any accumulation order returns it bit for bit."""
    assert representable(ref, p.out_dtype), f"reference not representable in {p.out_dtype}: max |x| = {ref.abs().max().item()}"
    if ksum is not None:
        assert representable(ksum, F32)
    a, b = logical(p)
    assert (a.abs() @ b.abs().t()).max().item() < 2 ** 24, "a partial sum could leave the f32 integers"


def _bits(x):
    return x.contiguous().view({4: torch.int32, 2: torch.int16}[x.element_size()])


def judge_exact(out, ref, what="C"):
    """`out` (a CPU tensor of the output type) equals the float64 reference bit for bit."""
    want = ref.to(out.dtype)
    if torch.equal(_bits(out), _bits(want)):
        return []
    bad = (_bits(out) != _bits(want)).nonzero()
    i = tuple(bad[0].tolist())
    return [f"{what} differs from the float64 reference at {len(bad)} elements, first at {i}: got {out[i].item()!r}, "
            f"expected {want[i].item()!r}"]


def _neighbour(x, step):
    """The next value of x's 16-bit type above (step = 1) or below (step = -1) x."""
    b = x.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
    mag = b & 0x7FFF
    o = torch.where((b >> 15) == 1, -mag, mag) + step            # sign-magnitude bits are ordered
    nb = torch.where(o < 0, (-o) | 0x8000, o)
    return torch.where(nb >= 32768, nb - 65536, nb).to(torch.int16).view(x.dtype)


def judge_random(out, ref, e):
    """(failures, worst ratio).  f32: |out - ref| <= E.  bf16 / f16: out is one of the values of its
    type in [round(ref - E), round(ref + E)].  The ratio is d / E with d the smallest change of the
    reference that makes `out` its correctly rounded value: |out - ref| for f32; for a 16-bit type 0
    where out = round(ref), else the distance from ref to the rounding boundary of `out` that faces
    it.  Rounding is monotonic, so ratio <= 1 is the interval test (up to ties); NaN gives inf."""
    o = out.to(F64)
    if out.dtype == F32:
        lo, hi = ref - e, ref + e
        d = (o - ref).abs()
    else:
        lo, hi = (ref - e).to(out.dtype).to(F64), (ref + e).to(out.dtype).to(F64)
        r = ref.to(out.dtype).to(F64)
        fin = torch.where(torch.isfinite(o), out, torch.zeros_like(out))
        above = (o + _neighbour(fin, -1).to(F64)) / 2 - ref      # out > round(ref): its lower boundary
        below = ref - (o + _neighbour(fin, 1).to(F64)) / 2
        d = torch.where(o > r, above, torch.where(o < r, below, torch.zeros_like(o))).clamp_min(0.0)
    ok = (o >= lo) & (o <= hi)
    ratio = torch.where(d == 0, torch.zeros_like(d), d / e)
    ratio = torch.where(torch.isfinite(o) & ~torch.isnan(ratio), ratio, torch.full_like(d, INF))
    worst = ratio.max().item() if ratio.numel() else 0.0
    fails = []
    if not ok.all():
        i = tuple((~ok).nonzero()[0].tolist())
        fails.append(f"{int((~ok).sum())} elements outside their interval, first at {i}: got {o[i].item()!r}, "
                     f"reference {ref[i].item()!r}, E {e[i].item():.3g}; worst ratio {worst:.3g}")
    return fails, worst


def old_global_bar(out, ref):
    """The bar of tests/test_gpu_gemm.py on a bf16 C: relative Frobenius norm over the matrix < 8e-3."""
    return ((out.to(F64) - ref).norm() / ref.norm().clamp_min(1e-30)).item() < 8e-3


# ------------------------------------------------------------------ guarded buffers
class Guarded:
    """A NaN-filled [rows + 3, cols + pad] buffer; .body is its logical [rows, cols] part (one guard
    row before, two after, `pad` guard columns), .ld its row length."""

    def __init__(self, rows, cols, dtype, pad, device="cpu", fill=None):
        self.buf = torch.full((rows + ROW_BEFORE + ROW_AFTER, cols + pad), NAN, dtype=dtype, device=device)
        self.body = self.buf[ROW_BEFORE:ROW_BEFORE + rows, :cols]
        self.ld = cols + pad
        if fill is not None:
            self.body.copy_(fill.to(dtype))
        self.before = _bits(self.buf).clone()

    def guard_failures(self, what):
        """Guards still NaN; no NaN inside."""
        nan = torch.isnan(self.buf).cpu()
        inside = torch.zeros_like(nan)
        inside[ROW_BEFORE:ROW_BEFORE + self.body.shape[0], :self.body.shape[1]] = True
        out = []
        if not nan[~inside].all():
            out.append(f"{what}: written outside its rows and columns")
        if nan[inside].any():
            out.append(f"{what}: {int(nan[inside].sum())} NaN inside")
        return out

    def unchanged(self):
        return torch.equal(_bits(self.buf), self.before)


class GuardedVec:
    """[n] floats with four NaN guard floats on each side."""

    def __init__(self, n, device="cpu", fill=None, dtype=F32):
        self.buf = torch.full((n + 2 * VEC_GUARD,), NAN, dtype=dtype, device=device)
        self.body = self.buf[VEC_GUARD:VEC_GUARD + n]
        if fill is not None:
            self.body.copy_(fill.to(dtype))
        self.before = _bits(self.buf).clone()

    def guard_failures(self, what):
        nan = torch.isnan(self.buf).cpu()
        out = []
        if not (nan[:VEC_GUARD].all() and nan[-VEC_GUARD:].all()):
            out.append(f"{what}: guard floats written")
        if nan[VEC_GUARD:-VEC_GUARD].any():
            out.append(f"{what}: NaN inside")
        return out

    def unchanged(self):
        return torch.equal(_bits(self.buf), self.before)
