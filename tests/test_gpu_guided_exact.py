"""tt2_attn_fwd_guided / tt2_attn_bwd_guided held to exact and per-row / per-block float64 bars (GPU).

The problems, references and judges are tests/_align_refs.py's (validated on the CPU by
tests/test_align_refs.py, whose mutants prove that these bars reject a W index off by one in n or
t or by 4 hi, Tx / Ty taken as tk / tq, kappa on rows >= Ty or on an unguided head, g formed from
the rounded p, kappa g missing from delta and a flipped sign of the W term):
  exact     the guided selector problem under the indicator guide (sigma = 2^-12: W is exactly 0
            on the diagonal and 1 elsewhere), kappa 0.5 and -2 from the device coef buffer: g, O,
            dQ, dK, dV and delta bit-equal to the float64 reference, LSE within 4 f32 ulp, g exactly
            +0 on unguided heads, rows >= Ty_b and empty rows, dK / dV exactly 0 past key_len
  random    sigma = 0.4, kappa = 3: g and delta per row, O / dQ / dK / dV per 32-row block
  diagonal  the same with 8 K[floor(n Tx / Ty)] added to Q: P sharply diagonal, g small
on every variant in bf16 and on f32, B = 2, H = 3, guide.heads in {0, 2, 3}, the six cross shapes
of _attn_refs.CROSS_TQ_TK, in the engine's layout (test_gpu_attention_exact.py's Guarded / Launch:
K / V column slices of a wide buffer at an offset, dK | dV in one fused buffer, every output
NaN-filled between NaN guards; g, LSE and delta slices between NaN guards).  Each test prints its
worst ratios (pytest -s; <= 1 passes)."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _align_refs as A  # noqa: E402
import _attn_refs as R  # noqa: E402
import test_gpu_attention_exact as E  # noqa: E402
from _attn_refs import BATCH as B, HEADS as H, F64  # noqa: E402
from test_gpu_attention_exact import BF16, F32, HD, NAN, Guarded, heads, variant  # noqa: E402,F401
from tt2 import _lib, ops  # noqa: E402

ROW_GUARD = E.LSE_GUARD


# ------------------------------------------------------------------ references, computed once
@functools.lru_cache(maxsize=None)
def exact_reference(tq, tk, kl, gd):
    return A.build_exact_guided(tq, tk, kl, gd)


@functools.lru_cache(maxsize=None)
def random_reference(kind, tq, tk, kl, gd, dtype):
    """(problem, float64 reference, block yardstick of `dtype`, the guided float32 evaluations)."""
    key_len = None if kl is None else list(kl)
    p = R.random_problem(B, H, tq, tk, key_len, False, dtype) if kind == "random" else \
        A.random_diagonal_problem(B, H, tq, tk, key_len, gd, dtype)
    f32 = A.guided_float32_evaluations(p, gd)
    return p, A.guided_ref64(p, gd), (A.GuidedTwin(gd)(p) if dtype == BF16 else f32), f32


# ------------------------------------------------------------------ one guided launch
def row_slice(n):
    """A NaN-filled f32 buffer and its [n] slice between NaN guards."""
    buf = torch.full((n + 2 * ROW_GUARD,), NAN, dtype=F32, device="cuda")
    return buf, buf[ROW_GUARD:ROW_GUARD + n]


def check_rows(buf, what, written=True):
    x = buf.cpu()
    assert torch.isnan(x[:ROW_GUARD]).all() and torch.isnan(x[-ROW_GUARD:]).all(), f"{what}: guards written"
    inside = torch.isnan(x[ROW_GUARD:-ROW_GUARD])
    assert not inside.any() if written else inside.all(), f"{what}: {'NaN left' if written else 'written'}"


class GuidedLaunch(E.Launch):
    """E.Launch's layout with the guide: g, LSE and delta between NaN guards, q_len and kappa on
    the device."""

    def __init__(self, p, gd, dtype):
        super().__init__(p, dtype)
        self.gd = gd
        self.q_len = None if gd.q_len is None else torch.tensor(gd.q_len, dtype=torch.int32).cuda()
        self.coef = torch.tensor([gd.kappa, NAN], dtype=F32).cuda()[:1]
        self.gkw = dict(key_len=self.key_len, q_len=self.q_len, sigma=gd.sigma, scale=p.scale)

    def fwd(self, guided=True, guide_heads=None):
        n = B * H * self.tq
        self.out = Guarded(B * self.tq, HD, self.dtype)
        self.lse_buf, self.lse = row_slice(n)
        self.g_buf, self.g = row_slice(n)
        args = (self.q, self.k, self.v, self.out.body, self.lse)
        lds = (self.q_ld, self.k_ld, self.v_ld, self.out.ld, B, H, self.tq, self.tk)
        if guided:
            ops.attn_fwd_guided(*args, self.g, *lds, guide_heads=self.gd.heads if guide_heads is None else guide_heads,
                                **self.gkw)
        else:
            ops.attn_fwd(*args, *lds, key_len=self.key_len, causal=False, scale=self.p.scale)
        torch.cuda.synchronize()
        self.out.check("out")
        check_rows(self.lse_buf, "lse")
        check_rows(self.g_buf, "g", written=guided)
        return self

    def bwd(self, parts=0, guided=True, kappa=None, guide_heads=None):
        tq, tk = self.tq, self.tk
        gq, gkv = Guarded(B * tq, HD, self.dtype), Guarded(B * tk, 2 * HD, self.dtype)
        dq, dk, dv = gq.body, gkv.body[:, :HD], gkv.body[:, HD:]
        self.delta_buf, self.delta = row_slice(B * H * tq)
        coef = self.coef if kappa is None else torch.tensor([kappa], dtype=F32).cuda()
        args = (self.q, self.k, self.v, self.out.body, self.do, self.lse, self.delta, dq, dk, dv)
        lds = (self.q_ld, self.k_ld, self.v_ld, self.out.ld, HD, gq.ld, gkv.ld, gkv.ld, B, H, tq, tk)
        if guided:
            ops.attn_bwd_guided(*args, self.g, coef, *lds, parts=parts,
                                guide_heads=self.gd.heads if guide_heads is None else guide_heads, **self.gkw)
        else:
            ops.attn_bwd(*args, *lds, key_len=self.key_len, causal=False, scale=self.p.scale, parts=parts)
        torch.cuda.synchronize()
        gq.check("dq", None if parts != 2 else torch.zeros(HD, dtype=torch.bool))
        gkv.check("dk | dv", None if parts != 1 else torch.zeros(2 * HD, dtype=torch.bool))
        x = self.delta_buf.cpu()
        assert torch.isnan(x[:ROW_GUARD]).all() and torch.isnan(x[-ROW_GUARD:]).all(), "delta: guards written"
        self.grads = (dq, dk, dv)
        return gq, gkv

    def results(self):
        out = super().results()
        out["g"] = self.g.cpu().to(F64).view(B, H, self.tq)
        out["delta"] = self.delta.cpu().to(F64).view(B, H, self.tq)
        return out

    def raw(self):
        return super().raw() + [self.g_buf.view(torch.int32).cpu(), self.delta_buf.view(torch.int32).cpu()]


def finish(kind, cid, fails, figs):
    print(f"\n{kind} {cid}: {R.show(figs)}")
    assert not fails, fails


# ------------------------------------------------------------------ exact
@pytest.mark.parametrize("case", A.exact_cases(), ids=lambda c: c[0])
def test_guided_selector_exact(case, variant):
    """g, O, dQ, dK, dV and delta bit-equal to the float64 reference cast to the output type; LSE
    within 4 f32 ulp; g exactly +0 on unguided heads, rows >= Ty_b and empty rows; dK / dV exactly 0
    past key_len.  Measured on an MI355X: equal on all 60 cases; the LSE's worst ratio is 0.093
    (0.37 ulp)."""
    cid, tq, tk, kl, gd = case
    p, ref = exact_reference(tq, tk, kl, gd)
    A.assert_indicator(p, gd)
    finish("exact", cid, *A.judge_guided_selector(GuidedLaunch(p, gd, variant).run(), ref, p, gd, variant))


@pytest.mark.parametrize("case", A.exact_cases(), ids=lambda c: c[0])
def test_guided_parts_compose_exactly(case, monkeypatch):
    """The fused bf16 launch: parts = 1 (dQ; the dK | dV buffer stays NaN) and parts = 2 (dK / dV;
    dQ stays NaN) are parts = 0 bit for bit, and parts = 0 is the float64 reference."""
    monkeypatch.setattr(ops, "ATTN_VARIANT", 0)
    cid, tq, tk, kl, gd = case
    p, ref = exact_reference(tq, tk, kl, gd)
    A.assert_indicator(p, gd)
    run = GuidedLaunch(p, gd, BF16).fwd()
    bits = lambda g: g.buf.view(torch.int16).cpu()   # noqa: E731
    q1, kv1 = run.bwd(1)
    delta1 = run.delta_buf.view(torch.int32).cpu()
    q2, kv2 = run.bwd(2)
    # (the dK / dV blocks compute delta + kappa g themselves and publish nothing: tt2_capi.h)
    assert torch.isnan(run.delta_buf).all(), "parts = 2 wrote the delta scratch"
    run.guards = q0, kv0 = run.bwd(0)
    assert torch.isnan(kv1.buf).all() and torch.isnan(q2.buf).all()
    assert torch.equal(bits(q1), bits(q0)) and torch.equal(bits(kv2), bits(kv0))
    assert torch.equal(delta1, run.delta_buf.view(torch.int32).cpu()), "parts = 1: delta is not the full launch's"
    finish("exact parts", cid, *A.judge_guided_selector(run.results(), ref, p, gd, BF16))


# ------------------------------------------------------------------ identities, bit for bit
@pytest.mark.parametrize("case", A.random_cases(), ids=lambda c: c[0])
def test_guided_identities(case, variant):
    """The guided forward's O / LSE are the plain call's; kappa = 0, or heads = 0, gives the plain
    backward; the unguided heads' slices of dQ / dK / dV are the plain call's; a second launch
    repeats the first -- all bit for bit, guards included."""
    cid, tq, tk, kl, gd = case
    p, _, _, _ = random_reference("random", tq, tk, kl, gd, variant)
    a, b, plain = GuidedLaunch(p, gd, variant), GuidedLaunch(p, gd, variant), GuidedLaunch(p, gd, variant)
    a.run()
    b.run()
    for x, y in zip(a.raw(), b.raw()):
        assert torch.equal(x, y), "a second launch differs"
    plain.fwd(guided=False)
    bits = torch.int16 if variant == BF16 else torch.int32
    raw = lambda g: g.buf.view(bits).cpu()   # noqa: E731
    assert torch.equal(raw(a.out), raw(plain.out)) and torch.equal(a.lse_buf.view(torch.int32).cpu(),
                                                                   plain.lse_buf.view(torch.int32).cpu())
    q0, kv0 = plain.bwd(guided=False)
    delta0 = plain.delta.cpu()
    q1, kv1 = a.bwd(kappa=0.0)
    assert torch.equal(raw(q1), raw(q0)) and torch.equal(raw(kv1), raw(kv0)), "kappa = 0 is not the plain backward"
    wrote = ~torch.isnan(delta0)       # (the plain fused launch leaves the scratch alone; where it is written, equal)
    assert torch.equal(a.delta.cpu()[wrote], delta0[wrote]) and not torch.isnan(a.delta).any()
    none = GuidedLaunch(p, gd, variant).fwd(guide_heads=0)
    assert (none.g.view(torch.int32) == 0).all(), "heads = 0: g is not +0"
    q2, kv2 = none.bwd(guide_heads=0)
    assert torch.equal(raw(q2), raw(q0)) and torch.equal(raw(kv2), raw(kv0)), "heads = 0 is not the plain backward"
    c0 = gd.heads * 64
    gq, gkv = a.guards
    assert torch.equal(raw(gq)[:, c0:], raw(q0)[:, c0:])
    assert torch.equal(raw(gkv)[:, c0:HD], raw(kv0)[:, c0:HD]) and torch.equal(raw(gkv)[:, HD + c0:], raw(kv0)[:, HD + c0:])
    live = ~A.zero_rows(p, gd) & (R.visible_counts(p) > 1)[:, None, :]     # one key: dS = 0 identically
    if live.any():
        assert not torch.equal(raw(gq)[:, :c0], raw(q0)[:, :c0]), "the guided heads are the plain call's"


# ------------------------------------------------------------------ random, per unit of work
def run_random(kind, case, dtype):
    cid, tq, tk, kl, gd = case
    p, ref, yard, f32 = random_reference(kind, tq, tk, kl, gd, dtype)
    out = GuidedLaunch(p, gd, dtype).run()
    fails, figs = A.judge_guided_random(out, ref, yard, f32, p, gd, dtype)
    figs["g_rel"] = A.g_relative_error(out["g"], ref, p, gd)
    print(f"\n{kind} {cid}: {R.show(figs)} g_rel {figs['g_rel']:.3e}")
    assert not fails, fails


@pytest.mark.parametrize("case", A.random_cases(), ids=lambda c: c[0])
def test_guided_random(case, variant):
    """g per row within max(4 x the float32 CPU evaluations' error on that row, 2 f32 ulp of
    sum_t P |W|) plus, on the v3 kernels, _align_refs.EXP2_ALLOWANCE 2^-24 sum_t P |W| for the
    hardware exp2; O, dQ, dK, dV per 32-row block against the guided twin (bf16, factor 2) or the
    guided float32 evaluations (f32, factor 4, floor 2 f32 ulp); delta per row against
    rowsum(dO O) + kappa g.  Measured on an MI355X, worst over the cases and variants (<= 1
    passes): g 0.25 (excess over the first term 2.51 units), O 0.51, dQ 0.52, dK 0.51, dV 0.50,
    LSE 0.30, delta 0.38; worst relative error of g 9.0e-5."""
    run_random("random", case, variant)


@pytest.mark.parametrize("case", A.random_cases(), ids=lambda c: c[0])
def test_guided_diagonal(case, variant):
    """The same bars where P is sharply diagonal and g small; prints the worst per-row relative
    error of g (g_rel), what 1 - exp2(e) costs near the diagonal.  Measured on an MI355X: g 0.64
    (excess 28.67 units on one row of 33x64 on the v3 kernels, the figure EXP2_ALLOWANCE is set
    from; 1.48 under the random problem's allowance of 8), O 0.52, dQ 0.60, dK 0.51, dV 0.88, LSE
    0.24, delta 0.42; g_rel 1.0 at 131x193 (rows with g near 1e-7), 6.8e-2 at 70x65, 6.6e-3 at
    33x64."""
    run_random("diagonal", case, variant)


# ------------------------------------------------------------------ refusals on the device
def _structs(run, guided_bwd):
    a = ops._attn_common(run.q, run.k, run.v, run.q_ld, run.k_ld, run.v_ld, B, H, run.tq, run.tk, run.key_len, False,
                         run.p.scale)
    out, gq, gkv = Guarded(B * run.tq, HD, run.dtype), Guarded(B * run.tq, HD, run.dtype), Guarded(B * run.tk, 2 * HD, run.dtype)
    bufs = [row_slice(B * H * run.tq) for _ in range(3)]            # g, lse, delta
    a.o_out, a.o_ld, a.lse, a.delta = out.body.data_ptr(), out.ld, bufs[1][1].data_ptr(), bufs[2][1].data_ptr()
    a.o, a.dout, a.do_ld = out.body.data_ptr(), run.do.data_ptr(), HD
    a.dq, a.dk, a.dv = gq.body.data_ptr(), gkv.body.data_ptr(), gkv.body[:, HD:].data_ptr()
    a.dq_ld, a.dk_ld, a.dv_ld = gq.ld, gkv.ld, gkv.ld
    g = _lib.AttnGuide()
    g.q_len, g.rows, g.coef, g.sigma, g.heads = ops.ptr(run.q_len), bufs[0][1].data_ptr(), run.coef.data_ptr(), 0.4, 2
    return a, g, [out.buf, gq.buf, gkv.buf] + [b[0] for b in bufs]


REFUSED = {"causal": lambda a, g: setattr(a, "causal", 1), "sigma 0": lambda a, g: setattr(g, "sigma", 0.0),
           "sigma < 0": lambda a, g: setattr(g, "sigma", -0.4), "sigma NaN": lambda a, g: setattr(g, "sigma", NAN),
           "heads > H": lambda a, g: setattr(g, "heads", H + 1), "heads < 0": lambda a, g: setattr(g, "heads", -1),
           "rows missing": lambda a, g: setattr(g, "rows", None)}


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_refused_calls_leave_the_outputs_untouched(dtype):
    p = R.random_problem(B, H, 33, 64, None, False, dtype)
    run = GuidedLaunch(p, A.Guide((33, 20), 0.4, 2, 3.0), dtype)
    L = ops.lib()
    cases = [(n, f, entry) for entry in ("tt2_attn_fwd_guided", "tt2_attn_bwd_guided") for n, f in REFUSED.items()]
    cases += [("coef missing", lambda a, g: setattr(g, "coef", None), "tt2_attn_bwd_guided"),
              ("guide missing", None, "tt2_attn_fwd_guided"), ("guide missing", None, "tt2_attn_bwd_guided")]
    for name, change, entry in cases:
        a, g, bufs = _structs(run, entry.endswith("bwd_guided"))
        if change:
            change(a, g)
        rc = getattr(L, entry)(C.byref(a), C.byref(g) if change else None, ops.stream_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.E_INVALID and entry.encode() in L.tt2_last_error(), (name, entry, rc)
        for x in bufs:
            assert torch.isnan(x).all(), (name, entry)
