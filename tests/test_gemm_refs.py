"""tests/_gemm_refs.py against independent evaluations (a triple loop over the stored operands,
F.conv1d and its autograd), its exact problem at every shape of the GPU test, the host plan of
every GPU case, and the proof that its bars bite: a small f32 tile model of a GEMM, written here
and taken from no kernel, passes both bars, and twelve deliberately wrong copies of it do not
(CPU only).  The mutants that touch one element or one row pass the old whole-matrix bar of
tests/test_gpu_gemm.py: that is why tests/test_gpu_gemm_exact.py exists."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _gemm_refs as R
from _gemm_refs import BF16, F32, F64, Case
from tt2 import _lib
from tt2_oracle import dropout_keep


# ------------------------------------------------------------------ the reference
def _loop(p):
    """C by the header's formulas, one scalar at a time, from the stored operands."""
    a, b = R.stored(p)
    lda, ldb = a.shape[1], b.shape[1]
    a, b = a.flatten().tolist(), b.flatten().tolist()
    keep = R.keep_mask(p) if p.drop else None

    def A(m, k):
        return a[k * lda + m] if p.trans_a else a[m * lda + k]

    def B(n, k):
        return b[k * ldb + n] if p.trans_b else b[n * ldb + k]
    out = torch.zeros(p.m, p.n, dtype=F64)
    for m in range(p.m):
        for n in range(p.n):
            v = 0.0
            for k in range(p.k):
                v += A(m, k) * B(n, k)
            v *= p.alpha
            if p.bias is not None:
                v += p.bias[n].item()
            if p.res is not None:
                v += p.res[m, n].item()
            if p.act == R.ACT_RELU:
                v = max(v, 0.0)
            if p.gate is not None:
                v = v * p.gate_scale if p.gate[m, n].item() != 0 else 0.0
            if keep is not None:
                v = v * R.drop_scale(p.drop[2]) if keep[m, n] else 0.0
            if p.beta:
                v += p.beta * p.c0[m, n].item()
            out[m, n] = v
    return out


@pytest.mark.parametrize("ta,tb", R.LAYOUTS)
@pytest.mark.parametrize("epi", ["all", "beta"])
def test_ref64_is_the_triple_loop(ta, tb, epi):
    p = R.make_problem(Case(1, BF16, 16, 24, 40, ta, tb, epi), exact=False)
    ref, _ = R.ref64(p)
    assert (ref - _loop(p)).abs().max().item() < 1e-12
    assert ref.abs().max().item() > 0.1


@pytest.mark.parametrize("T", [5, 37])
def test_conv_expansion_is_conv1d(T):
    """The a_conv forward, its dgrad and the b_conv weight gradient against F.conv1d in float64."""
    cin, cout, M = 8, 16, R.CONV_BATCH * T
    g = torch.Generator().manual_seed(T)
    x, dy = torch.randn(M, cin, generator=g, dtype=F64), torch.randn(M, cout, generator=g, dtype=F64)
    w = torch.randn(cout, cin, R.KS, generator=g, dtype=F64).requires_grad_(True)
    xs = x.view(-1, T, cin).transpose(1, 2).clone().requires_grad_(True)
    y = F.conv1d(xs, w, padding=R.CONV_PAD)
    (y * dy.view(-1, T, cout).transpose(1, 2)).sum().backward()
    conv = (T, cin, R.CONV_PAD)
    wp = w.detach().permute(0, 2, 1).reshape(cout, R.KS * cin)            # [Cout][tap][Cin]
    fwd, _ = R.ref64(R.Problem(x, wp, M, cout, R.KS * cin, a_conv=conv, in_dtype=F32, out_dtype=F32))
    assert (fwd - y.detach().transpose(1, 2).reshape(M, cout)).abs().max().item() < 1e-12
    wflip = w.detach().flip(2).permute(1, 2, 0).reshape(cin, R.KS * cout)  # [Cin][tap'][Cout]
    dx, _ = R.ref64(R.Problem(dy, wflip, M, cin, R.KS * cout, a_conv=(T, cout, R.CONV_PAD), in_dtype=F32, out_dtype=F32))
    assert (dx - xs.grad.transpose(1, 2).reshape(M, cin)).abs().max().item() < 1e-12
    ks0 = torch.arange(cout, dtype=F64)
    dw, ks = R.ref64(R.Problem(dy.t().contiguous(), x, cout, R.KS * cin, M, True, True, b_conv=conv, in_dtype=F32,
                               out_dtype=F32, ksum0=ks0, ksum_beta=0.5))
    assert (dw - w.grad.permute(0, 2, 1).reshape(cout, R.KS * cin)).abs().max().item() < 1e-12
    assert (ks - (0.5 * ks0 + dy.sum(0))).abs().max().item() < 1e-12


# ------------------------------------------------------------------ the GPU test's cases
def _one_per_problem(cases):
    seen = {}
    for c in cases:
        seen.setdefault(R.problem_key(c), c)
    return list(seen.values())


@pytest.mark.parametrize("case", _one_per_problem(R.EXACT_CASES + R.CONV_CASES + R.group_cases(8, 3)), ids=R.case_id)
def test_exact_problem_is_exact(case):
    p = R.make_problem(case, exact=True)
    ref, ksum = R.ref64(p)
    R.assert_exact_problem(p, ref, ksum)
    assert ref.abs().max().item() > 0


def test_exact_problem_at_long_k():
    """The recipe holds well past the GPU test's k: bias + residual + ReLU, gate x 2, dropout x 2."""
    p = R.make_problem(Case(13, BF16, 64, 64, 6144, False, False, "all"), exact=True)
    ref, _ = R.ref64(p)
    R.assert_exact_problem(p, ref)


def _host_args(c):
    """tt2_gemm_args of a case with aligned stand-in pointers: the plan reads sizes, flags and
    alignment only."""
    bias, res, act, gate, drop, _, beta = R.EPIS[c.epi]
    sa, sb, a_conv, b_conv = R._operand_shapes(c)
    dt = {F32: _lib.DT_F32, BF16: _lib.DT_BF16, R.F16: _lib.DT_F16}
    g = _lib.GemmArgs()
    g.a = g.b = g.c = 4096
    g.m, g.n, g.k = c.m, c.n, c.k
    g.lda = sa[1] if a_conv else (c.m if c.ta else c.k) + R.PAD_OPERAND
    g.ldb = sb[1] if b_conv else (c.n if c.tb else c.k) + R.PAD_OPERAND
    g.ldc, g.ldr, g.ldg = c.n + R.PAD_C, c.n + R.PAD_RES, c.n + R.PAD_GATE
    g.dtype_in, g.dtype_out = dt[c.in_dt], dt[R.out_dtype(c)]
    g.trans_a, g.trans_b, g.act, g.splits, g.kernel_variant = int(c.ta), int(c.tb), act, c.splits, c.variant
    g.alpha, g.beta, g.gate_scale = 1.0, float(beta), 1.0
    g.bias = 4096 if bias else None
    g.res, g.res_dtype = (4096, dt[res]) if res is not None else (None, 0)
    g.gate, g.gate_dtype = (4096, dt[gate]) if gate is not None else (None, 0)
    if drop:
        g.drop_seed, g.drop_thr = 4096, 1 << 31
    if a_conv:
        g.a_conv_t, g.a_conv_c, g.a_conv_pad = a_conv
    if b_conv:
        g.b_conv_t, g.b_conv_c, g.b_conv_pad = b_conv
    g.a_ksum = 4096 if c.ksum else None
    return g


@pytest.mark.parametrize("group", list(R.CASES) + ["conv"])
def test_every_case_plans_to_its_family(group):
    """The eligibility function agrees with the host planner: a forced variant the family takes plans
    to that family, so no case of the GPU test counts a fallback as coverage.  Every family is reached."""
    L = _lib.load()
    cases = R.CONV_CASES if group == "conv" else R.CASES[group]
    assert cases
    for c in cases:
        code = L.tt2_gemm_plan(C.byref(_host_args(c)))
        if c.variant:
            assert code == R.KERNEL[c.variant], (R.case_id(c), code)
        else:
            assert code in R.FAMILY, (R.case_id(c), code)
    if group == "conv":
        assert all(L.tt2_gemm_plan(C.byref(_host_args(c))) == 13 for sp in (1, 3) for c in R.group_cases(8, sp))
        assert {c.variant for c in cases} == {0, 1, 2, 13, 14, 15}
        assert any(c.variant == 13 and c.conv[0] == k for c in cases for k in ("fwd", "dgrad", "wgrad"))


def test_ineligible_requests_plan_elsewhere():
    """The other direction, on requests the lists leave out: the planner sends them to another kernel."""
    L = _lib.load()
    for c in [Case(15, BF16, 200, 136, 72, True, False, "none"), Case(15, BF16, 40, 24, 72, False, False, "none"),
              Case(16, BF16, 264, 128, 64, False, False, "none"), Case(16, BF16, 264, 256, 72, False, False, "none"),
              Case(17, BF16, 264, 128, 64, True, False, "none"), Case(17, BF16, 264, 136, 64, False, False, "none"),
              Case(13, BF16, 111, 80, 320, False, False, "none", 1, ("fwd", 37, 64, 80)),
              Case(3, BF16, 72, 24, 80, False, False, "none"), Case(2, F32, 136, 264, 72, False, False, "none")]:
        assert not R.eligible(c)
        assert L.tt2_gemm_plan(C.byref(_host_args(c))) != R.KERNEL[c.variant], R.case_id(c)


def test_shapes_follow_the_source():
    src = os.path.join(os.path.dirname(_lib.__file__), "..", "csrc")
    v8 = open(os.path.join(src, "gemm_v8.hip")).read()
    assert re.search(r"#define G8_RING (\d+)", v8).group(1) == str(R.V8_RING)
    common = open(os.path.join(src, "gemm_common.h")).read()
    assert "constexpr int BM = 128, BN = 128;" in common


# ------------------------------------------------------------------ a tile model and its mutants
class TileModel:
    """A GEMM as a tiled f32 kernel would run it: per split a slab of 64 x 64 tiles, each
    accumulated over 64-deep K steps made of 8-element chunks (the last step may be short), the
    slabs summed in order, then the epilogue in f32, element by element, reading its inputs from
    the guarded buffers by row length and storing C rounded to the output type.  `mut` names one
    deliberate mistake."""
    TILE, STEP, CHUNK, ROW = 64, 64, 8, 17       # ROW: the row a one-row mutant damages

    def __init__(self, mut=None):
        self.mut = mut

    def slabs(self, p):
        a, b = (t.to(F32) for t in R.logical(p))
        k_split = -(-(-(-p.k // p.splits)) // self.STEP) * self.STEP if p.splits > 1 else p.k
        n_split = -(-p.k // k_split)
        out = torch.zeros(n_split, p.m, p.n, dtype=F32)
        for s in range(n_split):
            k0, k1 = s * k_split, min(p.k, (s + 1) * k_split)
            for tm in range(0, p.m, self.TILE):
                for tn in range(0, p.n, self.TILE):
                    rows, cols = slice(tm, min(tm + self.TILE, p.m)), slice(tn, min(tn + self.TILE, p.n))
                    acc = torch.zeros(rows.stop - tm, cols.stop - tn, dtype=F32)
                    for ks in range(k0, k1, self.STEP):
                        if self.mut == "step_skipped" and (tm, tn, ks) == (0, 0, k0):
                            continue
                        for c0 in range(ks, min(ks + self.STEP, k1), self.CHUNK):
                            ch = slice(c0, min(c0 + self.CHUNK, k1))
                            at = a[rows, ch].clone()
                            if self.mut == "k_tail_dropped" and ch.stop == p.k and tm == 0:
                                at[self.ROW] = 0
                            acc += at @ b[cols, ch].t()
                    if self.mut == "fragments_swapped" and (tm, tn) == (0, 0) and s == 0:
                        acc = torch.cat([acc[16:32], acc[:16], acc[32:]])
                    out[s, rows, cols] = acc
        return out

    def reduce(self, slabs):
        acc = torch.zeros_like(slabs[0])
        for s in range(slabs.shape[0]):
            if self.mut == "slab_left_out" and s == slabs.shape[0] - 1:
                continue
            acc += slabs[s]
            if self.mut == "slab_twice" and s == 0:
                acc += slabs[s]
        return acc

    def __call__(self, p):
        m, n = p.m, p.n
        v = self.reduce(self.slabs(p)) * p.alpha
        row, col = torch.arange(m)[:, None].expand(m, n), torch.arange(n)[None, :].expand(m, n)
        c = R.Guarded(m, n, p.out_dtype, R.PAD_C, fill=p.c0 if p.beta else None)
        if p.bias is not None:
            bias = R.GuardedVec(n, fill=p.bias).buf
            v = v + bias[R.VEC_GUARD + (row % n if self.mut == "bias_by_row" else col)]
        relu_first = self.mut == "relu_before_residual" and p.act == R.ACT_RELU
        if relu_first:
            v = v.clamp_min(0)
        if p.res is not None:
            res = R.Guarded(m, n, p.res_dtype, R.PAD_RES, fill=p.res)
            ld = c.ld if self.mut == "residual_by_ldc" else res.ld
            v = v + res.buf.flatten().to(F32)[R.ROW_BEFORE * res.ld + row * ld + col]
        if p.act == R.ACT_RELU and not relu_first:
            v = v.clamp_min(0)
        elif p.act == R.ACT_TANH:
            v = torch.tanh(v)
        if p.gate is not None:
            gate = R.Guarded(m, n, p.gate_dtype, R.PAD_GATE, fill=p.gate)
            on = gate.buf.flatten().to(F32)[R.ROW_BEFORE * gate.ld + row * gate.ld + col] != 0
            v = torch.where(on, v * torch.tensor(p.gate_scale, dtype=F32), torch.zeros_like(v))
        if p.drop is not None:
            seed, site, prob = p.drop
            ld = c.ld if self.mut == "dropout_by_ldc" else n
            keep = torch.from_numpy(dropout_keep(seed, site, m * ld, prob))[row * ld + col]
            v = torch.where(keep, v * torch.tensor(R.drop_scale(prob), dtype=F32), torch.zeros_like(v))
        if p.beta and self.mut != "beta_dropped":
            v = v + torch.tensor(p.beta, dtype=F32) * c.body.to(F32)
        v = v.to(p.out_dtype)
        if self.mut == "neighbour_value":
            r, j = self.neighbour_target(v)
            v[r, j] = v[r, j + 1]
        c.body.copy_(v)
        if self.mut == "stored_one_right":
            c.buf[R.ROW_BEFORE + self.ROW, n] = v[self.ROW, n - 1]
            c.body[self.ROW, n - 1] = p.c0[self.ROW, n - 1] if p.beta else R.NAN
        return c

    @staticmethod
    def neighbour_target(v):
        """The element whose right neighbour differs from it by the amount closest to 1: a typical
        wrong element, not a lucky or an extreme one."""
        d = ((v[:, 1:].to(F64) - v[:, :-1].to(F64)).abs() - 1.0).abs()
        i = int(d.argmin())
        return i // d.shape[1], i % d.shape[1]


MAIN = Case(1, BF16, 264, 136, 200, False, False, "all", 3)       # tails in m, n and k; three uneven splits
BETA = Case(1, BF16, 136, 72, 200, False, False, "beta", 1)
WIDE = Case(1, BF16, 520, 264, 1000, False, False, "none", 1)     # where the old bar is blind to one row


def _verdicts(model, case):
    """(exact bar's failures, random bar's failures, the random problem's output and reference)."""
    pr, exact = R.make_problem(case, False), []
    if case.epi != "tanh":            # tanh is not part of the exact problem
        pe = R.make_problem(case, True)
        ref, _ = R.ref64(pe)
        R.assert_exact_problem(pe, ref)
        ce = model(pe)
        exact = ce.guard_failures("C") + R.judge_exact(ce.body.clone(), ref)
    ref_r, _, e = R.ref64(pr, bound=True)
    cr = model(pr)
    fails, ratio = R.judge_random(cr.body.clone(), ref_r, e)
    return exact, cr.guard_failures("C") + fails, ratio, cr.body.clone(), ref_r


@pytest.mark.parametrize("case", [MAIN, BETA, WIDE, Case(1, F32, 136, 72, 72, True, True, "tanh", 2),
                                  Case(1, BF16, 111, 80, 320, False, False, "brd", 1, ("fwd", 37, 64, 80))], ids=R.case_id)
def test_the_model_passes_both_bars(case):
    exact, rand, ratio, _, _ = _verdicts(TileModel(), case)
    if case.epi != "tanh":
        assert not exact, exact
    assert not rand, rand
    assert ratio <= 1
    print(f"\nmodel {R.case_id(case)}: worst ratio {ratio:.3f}")


# mutant -> (case, the random bar must reject it too, the old whole-matrix bar accepts it)
MUTANTS = {
    "k_tail_dropped": (WIDE, True, True),
    "step_skipped": (MAIN, True, False),
    "slab_left_out": (MAIN, True, False),
    "slab_twice": (MAIN, True, False),
    "fragments_swapped": (MAIN, True, False),
    "bias_by_row": (MAIN, True, False),
    "residual_by_ldc": (MAIN, True, False),
    "relu_before_residual": (MAIN, True, False),
    "dropout_by_ldc": (MAIN, True, False),
    "beta_dropped": (BETA, True, False),
    # (one element, but what the old bar made of it depended on what an unguarded C held before)
    "stored_one_right": (MAIN, False, False),
    "neighbour_value": (WIDE, True, True),
}


@pytest.mark.parametrize("mut", list(MUTANTS))
def test_the_bars_reject_the_mutant(mut):
    case, by_random, old_accepts = MUTANTS[mut]
    exact, rand, ratio, out, ref = _verdicts(TileModel(mut), case)
    assert exact, f"the exact bar accepted {mut}"
    if by_random:
        assert rand and ratio > 1, f"the per-element bar accepted {mut} (ratio {ratio})"
    if mut == "stored_one_right":
        assert any("outside" in f for f in exact), exact
    if old_accepts:
        assert R.old_global_bar(out, ref), f"{mut}: the whole-matrix bar was expected to accept it"
