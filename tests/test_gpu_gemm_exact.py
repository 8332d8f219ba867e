"""tt2_gemm / tt2_gemm_grouped held to exact and per-element float64 bars (GPU).

Two problems from tests/_gemm_refs.py (validated on the CPU by tests/test_gemm_refs.py, whose
mutants prove that these bars reject a dropped K chunk, a skipped K step, a missing or doubled
split-K slab, swapped fragments, a bias indexed by row, a residual or dropout index built from the
wrong row length, ReLU before the residual, a dropped beta * C0, a store one column off and a
single wrong element):
  exact   operands in {-1, 0, 1}, integer epilogue inputs, power-of-two factors: C (and the fused
          bias sums) bit-equal to the float64 reference, whatever the accumulation order or split
  random  N(0, 1) operands: every element within its own derived bound E, an f32 C by
          |C - ref| <= E, a bf16 / f16 C as one of the values in [round(ref - E), round(ref + E)]
on every kernel family forced through `variant` (v1 in f32 and bf16, v2, skinny, v7 with both
epilogue forms, v8, v10, v11) and on the auto plan, at the edges of each family's tile, K step and
ring (R.CASES), in every layout, with every fused epilogue set and uneven split-K.  The host plan
is asserted first, so a request that falls back to another kernel does not count as coverage.
Every buffer is NaN-poisoned: C, residual, gate and the operands sit in NaN-filled buffers with
guard rows and pad columns (each row length differs from n and from the others), the bias and the
bias sums between guard floats, the split-K workspace starts as NaN.  A read past m, n or k that
is not masked turns C into NaN, a store outside C breaks a guard, and every input must come back
unchanged.  Each random test prints its worst ratio (pytest -s; <= 1 passes)."""
import ctypes as C
import dataclasses
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _gemm_refs as R  # noqa: E402
from _gemm_refs import BF16, Case  # noqa: E402
from tt2 import _lib, ops  # noqa: E402

DEV = "cuda"
WS = ops.Workspace()           # a private split-K workspace, NaN before every launch


def nan_workspace(nbytes):
    WS.get(max(nbytes, 4)).view(torch.float32).fill_(R.NAN)


# ------------------------------------------------------------------ references, computed once
def by_problem(cases):
    """Cases of the same problem next to one another, so the reference cache stays small."""
    return sorted(cases, key=lambda c: repr(R.problem_key(c)))


@functools.lru_cache(maxsize=4)
def _reference(key, exact, first):
    p = R.make_problem(first, exact)
    ref, ksum, e = R.ref64(p, bound=True)
    if exact:
        R.assert_exact_problem(p, ref, ksum)
    return p, ref, ksum, e


def reference(case, exact):
    """(problem, float64 C, float64 bias sums or None, E): the values are shared by every variant,
    layout and split count of the problem and never written to."""
    key = R.problem_key(case)
    first = case._replace(variant=1, ta=False, tb=False, splits=1) if not case.conv else case._replace(variant=1, splits=1)
    p, ref, ksum, e = _reference(key, exact, first)
    return dataclasses.replace(p, trans_a=case.ta, trans_b=case.tb, splits=case.splits), ref, ksum, e


# ------------------------------------------------------------------ one launch
def vec_ok(g):
    """epi_vec_ok of csrc/gemm.hip: rows of C / res / gate start 16-B aligned at every 8th column."""
    def ok(p, ld, dt):
        return not p or (p % 16 == 0 and (ld * (2 if dt == _lib.DT_BF16 else 4)) % 16 == 0)
    return _lib.DT_F16 not in (g.dtype_out, g.res_dtype, g.gate_dtype) and ok(g.c, g.ldc, g.dtype_out) and \
        ok(g.res, g.ldr, g.res_dtype) and ok(g.gate, g.ldg, g.gate_dtype) and (g.bias or 0) % 16 == 0


class Launch:
    def __init__(self, p, variant):
        self.p = p
        a, b = R.stored(p)
        self.a = R.Guarded(a.shape[0], a.shape[1], p.in_dtype, 0 if p.a_conv else R.PAD_OPERAND, DEV, a)
        self.b = R.Guarded(b.shape[0], b.shape[1], p.in_dtype, 0 if p.b_conv else R.PAD_OPERAND, DEV, b)
        self.c = R.Guarded(p.m, p.n, p.out_dtype, R.PAD_C, DEV, p.c0 if p.beta else None)
        self.inputs = {"A": self.a, "B": self.b}
        kw = dict(trans_a=p.trans_a, trans_b=p.trans_b, alpha=p.alpha, beta=p.beta, act=p.act, splits=p.splits,
                  a_conv=p.a_conv, b_conv=p.b_conv, variant=variant)
        if p.bias is not None:
            self.inputs["bias"] = R.GuardedVec(p.n, DEV, p.bias)
            kw["bias"] = self.inputs["bias"].body
        if p.res is not None:
            self.inputs["res"] = R.Guarded(p.m, p.n, p.res_dtype, R.PAD_RES, DEV, p.res)
            kw.update(res=self.inputs["res"].body, ldr=self.inputs["res"].ld)
        if p.gate is not None:
            self.inputs["gate"] = R.Guarded(p.m, p.n, p.gate_dtype, R.PAD_GATE, DEV, p.gate)
            kw.update(gate=self.inputs["gate"].body, ldg=self.inputs["gate"].ld, gate_scale=p.gate_scale)
        if p.drop is not None:
            self.seed = torch.tensor([p.drop[0]], dtype=torch.int32, device=DEV)
            kw["drop"] = ops.Drop(self.seed, p.drop[1], p.drop[2])
        self.ksum = None
        if p.ksum0 is not None:
            self.ksum = R.GuardedVec(p.m, DEV, p.ksum0)
            kw.update(a_ksum=self.ksum.body, a_ksum_beta=p.ksum_beta)
        self.args = (self.a.body, self.b.body, self.c.body, p.m, p.n, p.k, self.a.ld, self.b.ld, self.c.ld)
        self.kw = kw

    def plan(self):
        """The kernel that runs this request, asserted from the host plan and the route's own
        conditions (a v8 / v10 / v11 plan leaves its family only when rows are not vector-aligned
        or the option set is one the family does not fuse: R.eligible)."""
        g = ops.gemm_args(*self.args, ws=WS, **self.kw)
        code = _lib.lib().tt2_gemm_plan(C.byref(g))
        if code in (15, 16, 17):
            assert vec_ok(g), "rows not vector-aligned: the route would leave the planned family"
        return code

    def run(self):
        nan_workspace(self.p.splits * self.p.m * (self.p.n + 1) * 4 if self.p.splits > 1 else 0)
        ops.gemm(*self.args, ws=WS, **self.kw)
        torch.cuda.synchronize()
        return self

    def failures(self):
        """Guards still NaN, no NaN inside, every input unchanged."""
        fails = self.c.guard_failures("C")
        if self.ksum is not None:
            fails += self.ksum.guard_failures("a_ksum")
        return fails + [f"{name} was written" for name, buf in self.inputs.items() if not buf.unchanged()]

    def out(self):
        return self.c.body.cpu().clone()


def launch(case, exact):
    """Plan, run and check one case; returns (family, Launch, reference, bias sums, E)."""
    p, ref, ksum, e = reference(case, exact)
    run = Launch(p, case.variant)
    code = run.plan()
    if case.variant:
        assert code == R.KERNEL[case.variant], f"planned kernel {code}, not the forced family"
    else:
        assert code in R.FAMILY and R.eligible(case._replace(variant=code)), f"auto plan {code}"
    run.run()
    return R.FAMILY[code], run, ref, ksum, e


# ------------------------------------------------------------------ the two problems
@pytest.mark.parametrize("case", by_problem(R.EXACT_CASES), ids=R.case_id)
def test_exact(case):
    """C bit-equal to the float64 reference on every family, layout, epilogue set and split count.
    Measured on an MI355X: equal on every case."""
    family, run, ref, _, _ = launch(case, True)
    fails = run.failures() + R.judge_exact(run.out(), ref)
    assert not fails, (family, fails)


@pytest.mark.parametrize("case", by_problem(R.RANDOM_CASES), ids=R.case_id)
def test_random(case):
    """Every element within its own bound E (f32), or one of the values of its type in
    [round(ref - E), round(ref + E)] (bf16, f16).
    Measured on an MI355X, cases and worst ratio per family (<= 1 passes; E is a worst-case bound,
    so a sound kernel sits far below it): v1 f32 operands 59, 0.177 (k = 8); v1 bf16 58, 0.005;
    v2 58, 0.005; v7 119 (both epilogue forms and the auto plan), 0.005; v8 35, 0.002; v10 14, 0.003;
    v11 14, 0.002; skinny bf16 37, 0.079; skinny f16 36, 0.073."""
    family, run, ref, _, e = launch(case, False)
    fails, ratio = R.judge_random(run.out(), ref, e)
    print(f"\ngemm-random {family} {R.case_id(case)}: worst ratio {ratio:.3f}")
    fails = run.failures() + fails
    assert not fails, (family, fails)


@pytest.mark.parametrize("case", by_problem(R.CONV_CASES), ids=R.case_id)
def test_conv_exact(case):
    """Conv1d(k5, pad 2) as implicit GEMMs, the a_conv forward and dgrad and the b_conv weight
    gradient (with the fused bias sums where the kernel carries them): bit-equal, so a frame that
    leaks across a sequence boundary or in from the guard rows shows."""
    family, run, ref, ksum, _ = launch(case, True)
    fails = run.failures() + R.judge_exact(run.out(), ref)
    if ksum is not None:
        fails += R.judge_exact(run.ksum.body.cpu().clone(), ksum, "a_ksum")
    assert not fails, (family, fails)


CONTROL = Case(13, BF16, 136, 264, 200, False, False, "all")


@pytest.mark.parametrize("variant", [1, 13])
@pytest.mark.parametrize("mistake", ["ldr_is_ldc", "k_one_chunk_short", "c_one_column_right"])
def test_the_harness_sees_a_wrong_request(mistake, variant):
    """Controls of this file's own plumbing: a request that is wrong on purpose, every access still
    inside its buffers, must be reported.  The residual read with C's row length meets the NaN pad,
    a k one chunk short misses eight products, a C one column to the right lands on the guard."""
    p, ref, _, _ = reference(CONTROL._replace(variant=variant), True)
    run = Launch(p, variant)
    args = list(run.args)
    if mistake == "ldr_is_ldc":
        run.kw["ldr"] = run.c.ld
    elif mistake == "k_one_chunk_short":
        args[5] -= 8
    else:
        args[2] = run.c.buf[R.ROW_BEFORE:R.ROW_BEFORE + p.m, 1:1 + p.n]
    run.args = tuple(args)
    run.run()
    fails = run.failures() + R.judge_exact(run.out(), ref)
    assert fails
    if mistake == "c_one_column_right":
        assert any("outside" in f for f in fails), fails


def test_every_family_is_reached():
    """The forced variants of the lists cover every family (each case asserts its own plan)."""
    assert {R.FAMILY[R.KERNEL[c.variant]] for c in R.ALL_CASES if c.variant} == set(R.FAMILY.values())


# ------------------------------------------------------------------ grouped weight gradients
@pytest.mark.parametrize("count,splits,max_groups", [(1, 1, 0), (1, 3, 0), (3, 1, 0), (3, 3, 0), (8, 1, 0), (8, 3, 0),
                                                      (8, 1, 8), (8, 3, 8)])
def test_grouped_exact(count, splits, max_groups):
    """ops.gemm_grouped (gemm7g_kernel) over 1, 3 and 8 weight-gradient problems, unsplit and with
    three splits, and with eight work groups walking all the items: every dW (f32) and every
    fused bias sum (a_ksum_beta = 0.5) bit-equal to the float64 reference."""
    runs, probs, total = [], [], 0
    for case in R.group_cases(count, splits):
        p, ref, ksum, _ = reference(case, True)
        run = Launch(p, 0)
        assert run.plan() == 13
        runs.append((run, ref, ksum))
        probs.append(dict(zip(("a", "b", "c", "m", "n", "k", "lda", "ldb", "ldc"), run.args), **run.kw))
        total += (splits * p.m * (p.n + 1) * 4 + 255) // 256 * 256
    nan_workspace(total)
    ops.gemm_grouped(probs, ws=WS, max_groups=max_groups)
    torch.cuda.synchronize()
    for i, (run, ref, ksum) in enumerate(runs):
        fails = run.failures() + R.judge_exact(run.out(), ref, "dW") + \
            R.judge_exact(run.ksum.body.cpu().clone(), ksum, "a_ksum")
        assert not fails, (i, R.GROUP[i], fails)
