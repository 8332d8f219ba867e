"""tt2_attn_fwd / tt2_attn_bwd held to exact and per-block float64 bars (GPU).

Three problems from tests/_attn_refs.py (validated on the CPU by tests/test_attn_refs.py, whose
mutants prove that these bars reject a dropped key, a mask off by one, a skipped tile, a missing
rescale, swapped heads, an unrounded dS and a wrong LSE):
  selector  exact arithmetic: O, dQ, dK, dV bit-equal to the float64 reference, LSE within 4 f32 ulp
  uniform   Q = 0: LSE = log2(visible keys) within 4 f32 ulp, O within 1 bf16 ulp (4 f32 ulp),
            dQ bit-equal to the twin on the rows whose count is a power of two
  random    every 32-row block (one wave's work) within 2x the error of the bf16 twin, in f32
            within max(4x the float32 CPU evaluations' error, 2 f32 ulp)
on every variant in bf16 and on f32, at the edges of the tile structure (R.cases), with the
engine's strides: causal self-attention reads one packed [B T, 3 HD] qkv and writes dQ | dK | dV as
column slices of one fused buffer; cross-attention reads K / V as column slices of a wider buffer
at a column offset.  Every output is NaN-filled first and carries guard rows and columns that
must still be NaN afterwards.  Each test prints its worst ratios (pytest -s; <= 1 passes)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _attn_refs as R  # noqa: E402
from _attn_refs import BATCH as B, HEADS as H, D, F64, Twin  # noqa: E402
from tt2 import _lib, ops  # noqa: E402

HD = H * D
BF16, F32 = torch.bfloat16, torch.float32
GUARD_COLS, ROW_BEFORE, ROW_AFTER, LSE_GUARD = 8, 1, 2, 4
KV_WIDE, KV_OFF = 2 * HD * 3, 2 * HD           # cross K / V: columns KV_OFF.. of a [B Tk, 6 HD] buffer
NAN = float("nan")


@pytest.fixture(params=[(0, BF16), (1, BF16), (2, BF16), (3, BF16), (0, F32)],
                ids=["auto-bf16", "v1-bf16", "v3w2-bf16", "v3w4-bf16", "auto-f32"])
def variant(request):
    old = ops.ATTN_VARIANT
    ops.ATTN_VARIANT = request.param[0]
    yield request.param[1]
    ops.ATTN_VARIANT = old


# ------------------------------------------------------------------ references, computed once
BUILDERS = {"selector": lambda tq, tk, kl, causal, dt: R.selector_problem(B, H, tq, tk, kl, causal),
            "uniform": lambda tq, tk, kl, causal, dt: R.uniform_problem(B, H, tq, tk, kl, causal, dt),
            "random": lambda tq, tk, kl, causal, dt: R.random_problem(B, H, tq, tk, kl, causal, dt)}


@functools.lru_cache(maxsize=None)
def _reference(kind, tq, tk, causal, kl, dtype):
    """(problem, float64 reference, yardstick of `dtype`, the float32 evaluations' LSE); shared by
    the variants and never written to."""
    p = BUILDERS[kind](tq, tk, None if kl is None else list(kl), causal, dtype)
    ref = R.ref64(p)
    if kind == "selector":
        R.assert_exact_problem(ref, f"{tq}x{tk}")
        return p, ref, None, None
    f32 = R.float32_evaluations(p)
    return p, ref, (Twin()(p) if dtype == BF16 else f32), [y["lse"] for y in f32]


def reference(kind, case, dtype):
    _, tq, tk, causal, kl = case
    return _reference(kind, tq, tk, causal, None if kl is None else tuple(kl), dtype)


# ------------------------------------------------------------------ one launch, the engine's layout
def flat(x, dtype):
    """[B, H, T, 64] float64 -> [B T, H 64] of dtype on the CPU."""
    return x.transpose(1, 2).reshape(-1, HD).to(dtype)


def heads(x):
    """[B T, H 64] device tensor -> [B, H, T, 64] float64 on the CPU."""
    return x.detach().cpu().to(F64).view(B, -1, H, D).transpose(1, 2).contiguous()


class Guarded:
    """A NaN-filled [rows + 3, cols + 8] buffer; .body is its logical [rows, cols] part (one guard
    row before, two after, eight guard columns), .ld its row length."""

    def __init__(self, rows, cols, dtype):
        self.buf = torch.full((rows + ROW_BEFORE + ROW_AFTER, cols + GUARD_COLS), NAN, dtype=dtype, device="cuda")
        self.body = self.buf[ROW_BEFORE:ROW_BEFORE + rows, :cols]
        self.ld = cols + GUARD_COLS

    def check(self, what, written=None):
        """Guards still NaN; no NaN inside (`written`: bool per column, default every column)."""
        nan = torch.isnan(self.buf).cpu()
        inside = torch.zeros_like(nan)
        inside[ROW_BEFORE:ROW_BEFORE + self.body.shape[0], :self.body.shape[1]] = True
        if written is not None:
            inside[:, :self.body.shape[1]] &= written[None, :]
        assert nan[~inside].all(), f"{what}: written outside its slice"
        assert not nan[inside].any(), f"{what}: NaN left inside"


class Launch:
    def __init__(self, p, dtype):
        self.p, self.dtype = p, dtype
        _, _, self.tq, self.tk = p.shape
        tq, tk = self.tq, self.tk
        g = torch.Generator().manual_seed(5)
        if p.causal:      # packed qkv, as the self-attention blocks
            qkv = torch.cat([flat(x, dtype) for x in (p.q, p.k, p.v)], 1).cuda()
            self.q, self.k, self.v = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:]
            self.q_ld = self.k_ld = self.v_ld = 3 * HD
        else:             # K / V inside the wide buffer the decoder's layers share, junk around them
            self.q = flat(p.q, dtype).cuda()
            wide = torch.randn(B * tk, KV_WIDE, generator=g).to(dtype)
            wide[:, KV_OFF:KV_OFF + HD], wide[:, KV_OFF + HD:KV_OFF + 2 * HD] = flat(p.k, dtype), flat(p.v, dtype)
            wide = wide.cuda()
            self.k, self.v = wide[:, KV_OFF:], wide[:, KV_OFF + HD:]
            self.q_ld, self.k_ld, self.v_ld = HD, KV_WIDE, KV_WIDE
        self.do = flat(p.do, dtype).cuda()
        self.key_len = None if p.key_len is None else torch.tensor(p.key_len, dtype=torch.int32).cuda()
        self.kw = dict(key_len=self.key_len, causal=p.causal, scale=p.scale)

    def fwd(self):
        self.out = Guarded(B * self.tq, HD, self.dtype)
        self.lse_buf = torch.full((B * H * self.tq + 2 * LSE_GUARD,), NAN, dtype=F32, device="cuda")
        self.lse = self.lse_buf[LSE_GUARD:LSE_GUARD + B * H * self.tq]
        ops.attn_fwd(self.q, self.k, self.v, self.out.body, self.lse, self.q_ld, self.k_ld, self.v_ld, self.out.ld,
                     B, H, self.tq, self.tk, **self.kw)
        torch.cuda.synchronize()
        self.out.check("out")
        lse = self.lse_buf.cpu()
        assert torch.isnan(lse[:LSE_GUARD]).all() and torch.isnan(lse[-LSE_GUARD:]).all(), "lse: guards written"
        assert not torch.isnan(lse[LSE_GUARD:-LSE_GUARD]).any(), "lse: NaN left"
        return self

    def bwd(self, parts=0):
        """dQ | dK | dV as column slices of one fused buffer (causal), or dQ alone and dK | dV in one
        (cross).  Returns the guarded buffers; their guards and NaNs are checked for `parts`."""
        tq, tk = self.tq, self.tk
        if self.p.causal:
            fused = Guarded(B * tq, 3 * HD, self.dtype)
            gq = gkv = fused
            dq, dk, dv = fused.body[:, :HD], fused.body[:, HD:2 * HD], fused.body[:, 2 * HD:]
        else:
            gq, gkv = Guarded(B * tq, HD, self.dtype), Guarded(B * tk, 2 * HD, self.dtype)
            dq, dk, dv = gq.body, gkv.body[:, :HD], gkv.body[:, HD:]
        delta = torch.full((B * H * tq,), NAN, dtype=F32, device="cuda")
        ops.attn_bwd(self.q, self.k, self.v, self.out.body, self.do, self.lse, delta, dq, dk, dv,
                     self.q_ld, self.k_ld, self.v_ld, self.out.ld, HD, gq.ld, gkv.ld, gkv.ld,
                     B, H, tq, tk, parts=parts, **self.kw)
        torch.cuda.synchronize()
        if self.p.causal:
            fused.check("dq | dk | dv")
        else:
            gq.check("dq", None if parts != 2 else torch.zeros(HD, dtype=torch.bool))
            gkv.check("dk | dv", None if parts != 1 else torch.zeros(2 * HD, dtype=torch.bool))
        self.grads = (dq, dk, dv)
        return gq, gkv

    def results(self):
        dq, dk, dv = self.grads
        return {"o": heads(self.out.body), "lse": self.lse.cpu().to(F64).view(B, H, self.tq),
                "dq": heads(dq), "dk": heads(dk), "dv": heads(dv)}

    def raw(self):
        """Every output buffer with its guards, as bits."""
        bits = torch.int16 if self.dtype == BF16 else torch.int32
        bufs = {id(g): g for g in self.guards}.values()
        return [self.out.buf.view(bits).cpu(), self.lse_buf.view(torch.int32).cpu()] + [g.buf.view(bits).cpu() for g in bufs]

    def run(self):
        self.fwd()
        self.guards = self.bwd()
        return self.results()


def finish(kind, case, fails, figs):
    print(f"\n{kind} {case[0]}: {R.show(figs)}")
    assert not fails, fails


# ------------------------------------------------------------------ the three problems
@pytest.mark.parametrize("case", R.cases(R.SELECTOR_ROT), ids=lambda c: c[0])
def test_selector_exact(case, variant):
    """O, dQ, dK, dV bit-equal to the float64 reference cast to the output type; LSE within 4 f32
    ulp and +inf on empty rows; empty rows of O and dK / dV past key_len exactly 0.
    Measured on an MI355X: equal on all 75 cases; the LSE's worst ratio is 0.093 (0.37 ulp)."""
    p, ref, _, _ = reference("selector", case, variant)
    finish("selector", case, *R.judge_selector(Launch(p, variant).run(), ref, p, variant))


@pytest.mark.parametrize("case", R.cases(R.UNIFORM_ROT), ids=lambda c: c[0])
def test_uniform(case, variant):
    """LSE = log2(count) within 4 f32 ulp of max(|ref|, 1); O within 1 bf16 ulp of RN(mean) and
    equal where the count is a power of two (f32: 4 f32 ulp); the backward under the block bars.
    On the rows whose count is a power of two dQ equals the twin's bit for bit.
    Measured on an MI355X, worst over the cases: bf16 O 0 ulp from RN(ref) on every variant, f32 O
    1.24 ulp; LSE ratio 0.25; block ratios bf16 dQ 0.52, dV 0.50, f32 dQ 0.52, dV 0.52 (dK = 0);
    dQ equal on every power-of-two row (up to 771 of them in a case, 12 of the 15 cases have some)."""
    p, ref, yard, _ = reference("uniform", case, variant)
    finish("uniform", case, *R.judge_uniform(Launch(p, variant).run(), ref, yard, p, variant))


@pytest.mark.parametrize("case", R.cases(R.RANDOM_ROT), ids=lambda c: c[0])
def test_random_blocks(case, variant):
    """Every 32-row block of O, dQ, dK, dV against the twin's (bf16) or the float32 CPU
    evaluations' (f32) error on the same block; the LSE against the float32 evaluations'.
    Measured on an MI355X, worst block over the cases and variants (<= 1 passes): bf16 O 0.58,
    dQ 0.55, dK 0.61, dV 0.50, LSE 0.39 (most blocks sit at 0.500: the kernel's error is the
    twin's); f32 O 0.32, dQ 0.49, dK 0.73, dV 0.39, LSE 0.26."""
    p, ref, yard, lse32 = reference("random", case, variant)
    finish("random", case, *R.judge_random(Launch(p, variant).run(), ref, yard, lse32, p, variant))


# ------------------------------------------------------------------ parts, repeatability
CROSS = [c for c in R.cases(R.RANDOM_ROT) if not c[3]]


@pytest.mark.parametrize("case", CROSS, ids=lambda c: c[0])
def test_parts_split_the_plain_backward(case, monkeypatch):
    """parts = 1 writes dQ alone (the dK | dV buffer stays NaN), parts = 2 dK / dV alone (dQ stays
    NaN), and together they are parts = 0 bit for bit (non-causal, bf16, auto)."""
    monkeypatch.setattr(ops, "ATTN_VARIANT", 0)
    p, _, _, _ = reference("random", case, BF16)
    run = Launch(p, BF16).fwd()
    bits = lambda g: g.buf.view(torch.int16).cpu()   # noqa: E731
    q0, kv0 = run.bwd(0)
    q1, kv1 = run.bwd(1)
    q2, kv2 = run.bwd(2)
    assert torch.isnan(kv1.buf).all() and torch.isnan(q2.buf).all()
    assert torch.equal(bits(q1), bits(q0)) and torch.equal(bits(kv2), bits(kv0))


@pytest.mark.parametrize("causal,dtype", [(True, BF16), (False, F32), (True, F32)])
@pytest.mark.parametrize("parts", [1, 2])
def test_parts_refused_off_the_plain_launch(causal, dtype, parts, monkeypatch):
    monkeypatch.setattr(ops, "ATTN_VARIANT", 0)
    p = R.random_problem(B, H, 33, 33, None, causal, dtype)
    run = Launch(p, dtype).fwd()
    with pytest.raises(_lib.TT2Error):
        run.bwd(parts)


@pytest.mark.parametrize("case", R.cases(R.RANDOM_ROT), ids=lambda c: c[0])
def test_repeatable(case, variant):
    """Forward and backward run twice give bit-identical O, LSE, dQ, dK, dV (no atomics: the
    file header of attention_common.h promises it), guards included."""
    p, _, _, _ = reference("random", case, variant)
    a, b = Launch(p, variant), Launch(p, variant)
    a.run()
    b.run()
    for x, y in zip(a.raw(), b.raw()):
        assert torch.equal(x, y)
