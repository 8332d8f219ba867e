"""Guided-attention kernels (tt2_attn_fwd_guided / tt2_attn_bwd_guided / tt2_guided_attn_loss)
vs a float64 torch reference (GPU).

The reference is test_gpu_attention.py's ref_attn restated, plus kappa * sum(P * W) with
W[b, n, t] = 1 - exp(-(t / Tx_b - n / Ty_b)^2 / (2 sigma^2)), differentiated by autograd.

Bars: test_gpu_attention.py's (forward 2e-6 f32 / 1e-2 bf16, backward 5e-6 / 2e-2, relative
Frobenius norm).  g is a P-weighted sum like O; for f32 its bar is max(2e-6, 2 x the distance
of a plain float32 CPU evaluation of the same reference from the float64 one).  That floor
measured 7.4e-8 .. 9.0e-8 on the three cases below (W's cancellation near the diagonal), so
the bar in force is 2e-6.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tt2 import _lib, ops  # noqa: E402

D = 64
SIGMA = 0.4
KAPPA = 3.0   # large against scale / N of a real step, so the guided term weighs in every gradient


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def ref_probs(q, k, key_len, scale):
    """q [B,H,Tq,64], k [B,H,Tk,64]; masked probs exactly 0; empty rows -> 0."""
    B, H, Tq, _ = q.shape
    Tk = k.shape[2]
    s = (q @ k.transpose(-1, -2)) * scale
    allowed = torch.ones(B, 1, Tq, Tk, dtype=torch.bool)
    if key_len is not None:
        allowed &= torch.arange(Tk)[None, None, None, :] < key_len.view(B, 1, 1, 1)
    s = s.masked_fill(~allowed, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.exp(s - mx) * allowed
    den = e.sum(-1, keepdim=True)
    return e / torch.where(den > 0, den, torch.ones_like(den))


def guide_weight(B, H, Tq, Tk, key_len, q_len, gheads, dtype):
    """W * validity [B, H, Tq, Tk]: 0 on heads >= gheads, rows n >= Ty_b, keys t >= Tx_b."""
    tx = torch.full((B,), Tk) if key_len is None else key_len.clamp(max=Tk)
    ty = torch.full((B,), Tq) if q_len is None else q_len.clamp(max=Tq)
    t = torch.arange(Tk, dtype=dtype)[None, None, :]
    n = torch.arange(Tq, dtype=dtype)[None, :, None]
    txf, tyf = tx.to(dtype).clamp(min=1).view(B, 1, 1), ty.to(dtype).clamp(min=1).view(B, 1, 1)
    w = 1.0 - torch.exp(-((t / txf - n / tyf) ** 2) / (2 * SIGMA * SIGMA))
    valid = (torch.arange(Tk)[None, None, :] < tx.view(B, 1, 1)) & (torch.arange(Tq)[None, :, None] < ty.view(B, 1, 1))
    w = (w * valid)[:, None].expand(B, H, Tq, Tk).clone()
    w[:, gheads:] = 0
    return w


def ref_all(q, k, v, key_len, q_len, gheads, scale):
    p = ref_probs(q, k, key_len, scale)
    B, H, Tq, Tk = p.shape
    g = (p * guide_weight(B, H, Tq, Tk, key_len, q_len, gheads, q.dtype)).sum(-1)
    return p @ v, g


CASES = [
    # B, H, Tq, Tk, key_len, q_len, guided heads
    (3, 3, 131, 133, [133, 70, 0], [131, 40, 17], 2),
    (2, 2, 70, 37, [37, 20], [70, 0], 2),
    (1, 8, 64, 128, None, None, 8),
]


class Problem:
    """One case's device tensors and float64 reference (built once per (case, dtype))."""

    def __init__(self, case, dtype):
        B, H, Tq, Tk, kl, ql, gh = case
        self.case, self.dtype = case, dtype
        self.scale = 1.0 / math.sqrt(D)
        HD = self.HD = H * D
        g = torch.Generator().manual_seed(B * 100 + Tq + Tk)
        q = torch.randn(B * Tq, HD, generator=g)
        kv = torch.randn(B * Tk, 2 * HD, generator=g)
        dout = torch.randn(B * Tq, HD, generator=g)
        self.q_d, self.kv_d, self.dout_d = q.to(dtype).cuda(), kv.to(dtype).cuda(), dout.to(dtype).cuda()
        self.key_len = None if kl is None else torch.tensor(kl, dtype=torch.int32)
        self.q_len = None if ql is None else torch.tensor(ql, dtype=torch.int32)
        self.klen_d = None if kl is None else self.key_len.cuda()
        self.qlen_d = None if ql is None else self.q_len.cuda()

        def heads(x, T):
            return x.to(dtype).double().view(B, T, H, D).transpose(1, 2)

        self.qr = heads(q, Tq).clone().requires_grad_(True)
        self.kr = heads(kv[:, :HD], Tk).clone().requires_grad_(True)
        self.vr = heads(kv[:, HD:], Tk).clone().requires_grad_(True)
        o, self.g_ref = ref_all(self.qr, self.kr, self.vr, self.key_len, self.q_len, gh, self.scale)
        self.o_ref = o.transpose(1, 2).reshape(B * Tq, HD).detach()
        ((o * heads(dout, Tq)).sum() + KAPPA * self.g_ref.sum()).backward()
        flat = lambda x, T: x.transpose(1, 2).reshape(B * T, HD)  # noqa: E731
        self.dq_ref, self.dk_ref, self.dv_ref = flat(self.qr.grad, Tq), flat(self.kr.grad, Tk), flat(self.vr.grad, Tk)
        self.g_ref = self.g_ref.detach().reshape(B * H, Tq)
        # the float32 CPU evaluation's own distance from float64 (the f32 bar's floor)
        with torch.no_grad():
            _, g32 = ref_all(self.qr.float(), self.kr.float(), self.vr.float(), self.key_len, self.q_len, gh,
                             self.scale)
        self.g_floor = rel(g32.reshape(B * H, Tq), self.g_ref)

    def fwd(self, guided=True, gheads=None):
        B, H, Tq, Tk, _, _, gh = self.case
        HD = self.HD
        out = torch.zeros(B * Tq, HD, dtype=self.dtype, device="cuda")
        lse = torch.zeros(B * H, Tq, dtype=torch.float32, device="cuda")
        rows = torch.full((B * H, Tq), 7.0, dtype=torch.float32, device="cuda")
        k_t, v_t = self.kv_d[:, :HD], self.kv_d[:, HD:]
        if guided:
            ops.attn_fwd_guided(self.q_d, k_t, v_t, out, lse, rows, HD, 2 * HD, 2 * HD, HD, B, H, Tq, Tk, self.klen_d,
                                q_len=self.qlen_d, sigma=SIGMA, guide_heads=gh if gheads is None else gheads,
                                scale=self.scale)
        else:
            ops.attn_fwd(self.q_d, k_t, v_t, out, lse, HD, 2 * HD, 2 * HD, HD, B, H, Tq, Tk, self.klen_d, False,
                         self.scale)
        return out, lse, rows

    def bwd(self, out, lse, rows=None, kappa=KAPPA, gheads=None, parts=0):
        B, H, Tq, Tk, _, _, gh = self.case
        HD = self.HD
        dq = torch.zeros(B * Tq, HD, dtype=self.dtype, device="cuda")
        dkv = torch.zeros(B * Tk, 2 * HD, dtype=self.dtype, device="cuda")
        delta = torch.zeros(B * H, Tq, dtype=torch.float32, device="cuda")
        k_t, v_t = self.kv_d[:, :HD], self.kv_d[:, HD:]
        lds = (HD, 2 * HD, 2 * HD, HD, HD, HD, 2 * HD, 2 * HD)
        if rows is not None:
            coef = torch.tensor([kappa], dtype=torch.float32, device="cuda")
            ops.attn_bwd_guided(self.q_d, k_t, v_t, out, self.dout_d, lse, delta, dq, dkv[:, :HD], dkv[:, HD:], rows,
                                coef, *lds, B, H, Tq, Tk, self.klen_d, q_len=self.qlen_d, sigma=SIGMA,
                                guide_heads=gh if gheads is None else gheads, scale=self.scale, parts=parts)
        else:
            ops.attn_bwd(self.q_d, k_t, v_t, out, self.dout_d, lse, delta, dq, dkv[:, :HD], dkv[:, HD:], *lds,
                         B, H, Tq, Tk, self.klen_d, False, self.scale, parts=parts)
        return dq, dkv


_problems = {}


def problem(case, dtype) -> Problem:
    key = (CASES.index(case), dtype)
    if key not in _problems:
        _problems[key] = Problem(case, dtype)
    return _problems[key]


@pytest.fixture(params=[0, 1, 2, 3], ids=["auto", "v1", "v3w2", "v3w4"])
def attn_variant(request):
    old = ops.ATTN_VARIANT
    ops.ATTN_VARIANT = request.param
    yield request.param
    ops.ATTN_VARIANT = old


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=["ragged3x3", "empty_q2x2", "full1x8"])
def test_guided_fwd_bwd(dtype, case, attn_variant):
    B, H, Tq, Tk, kl, ql, gh = case
    HD = H * D
    P = problem(case, dtype)
    out, lse, rows = P.fwd()
    # ---- forward: g against the reference, exact zeros, O / lse bit-identical to the plain call
    tol_g = max(2e-6, 2 * P.g_floor) if dtype == torch.float32 else 1e-2
    err_g = rel(rows, P.g_ref)
    print(f"g rel {err_g:.3e} (bar {tol_g:.1e}, f32 reference floor {P.g_floor:.2e})")
    assert err_g < tol_g
    r = rows.view(B, H, Tq)
    assert r[:, gh:].abs().max().item() == 0 if gh < H else True
    for b in range(B):
        ty = Tq if ql is None else ql[b]
        tx = Tk if kl is None else kl[b]
        if ty < Tq:
            assert r[b, :, ty:].abs().max().item() == 0
        if tx == 0:
            assert r[b].abs().max().item() == 0
    out0, lse0, _ = P.fwd(guided=False)
    assert torch.equal(out, out0) and torch.equal(lse, lse0)
    assert rel(out, P.o_ref) < (2e-6 if dtype == torch.float32 else 1e-2)
    out2, lse2, rows2 = P.fwd()
    assert torch.equal(rows, rows2) and torch.equal(out, out2) and torch.equal(lse, lse2)
    # ---- backward against the reference
    dq, dkv = P.bwd(out, lse, rows)
    tol_b = 5e-6 if dtype == torch.float32 else 2e-2
    errs = rel(dq, P.dq_ref), rel(dkv[:, :HD], P.dk_ref), rel(dkv[:, HD:], P.dv_ref)
    print("dq dk dv rel", " ".join(f"{e:.3e}" for e in errs), f"(bar {tol_b:.1e})")
    assert max(errs) < tol_b
    if kl is not None:
        for b, L in enumerate(kl):   # keys past the length: exactly zero gradient
            if L < Tk:
                assert dkv.view(B, Tk, 2 * HD)[b, L:].abs().max().item() == 0
    dq_b, dkv_b = P.bwd(out, lse, rows)
    assert torch.equal(dq, dq_b) and torch.equal(dkv, dkv_b)
    # ---- kappa = 0 and heads = 0: the plain backward bit for bit
    dq0, dkv0 = P.bwd(out, lse)
    for kw in (dict(kappa=0.0), dict(gheads=0)):
        rws = rows if "kappa" in kw else P.fwd(gheads=0)[2]
        dq1, dkv1 = P.bwd(out, lse, rws, **kw)
        assert torch.equal(dq1, dq0) and torch.equal(dkv1, dkv0), kw
    # ---- the unguided heads' slices are the plain call's
    if gh < H:
        c0 = gh * D
        assert torch.equal(dq[:, c0:], dq0[:, c0:])
        assert torch.equal(dkv[:, c0:HD], dkv0[:, c0:HD]) and torch.equal(dkv[:, HD + c0:], dkv0[:, HD + c0:])
        assert not torch.equal(dq[:, :c0], dq0[:, :c0])   # ... and the guided ones are not


@pytest.mark.parametrize("case", CASES[:2], ids=["ragged3x3", "empty_q2x2"])
def test_guided_parts_compose(case):
    """parts 1 (dQ) and 2 (dK / dV) of the fused bf16 launch together equal parts 0."""
    B, H, Tq, Tk, kl, ql, gh = case
    P = problem(case, torch.bfloat16)
    out, lse, rows = P.fwd()
    dq, dkv = P.bwd(out, lse, rows)
    dq1, dkv1 = P.bwd(out, lse, rows, parts=1)
    dq2, dkv2 = P.bwd(out, lse, rows, parts=2)
    assert torch.equal(dq1, dq) and torch.equal(dkv2, dkv)
    assert dkv1.abs().max().item() == 0 and dq2.abs().max().item() == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_guided_causal_refused(dtype):
    B, H, T = 1, 2, 64
    HD = H * D
    x = torch.zeros(B * T, 3 * HD, dtype=dtype, device="cuda")
    out = torch.zeros(B * T, HD, dtype=dtype, device="cuda")
    lse = torch.zeros(B * H, T, dtype=torch.float32, device="cuda")
    rows = torch.zeros(B * H, T, dtype=torch.float32, device="cuda")
    coef = torch.zeros(1, dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.TT2Error, match=r"\(-1\).*non-causal"):   # TT2_E_INVALID
        ops.attn_fwd_guided(x, x[:, HD:], x[:, 2 * HD:], out, lse, rows, 3 * HD, 3 * HD, 3 * HD, HD, B, H, T, T,
                            causal=True)
    with pytest.raises(_lib.TT2Error, match=r"\(-1\).*non-causal"):
        ops.attn_bwd_guided(x, x[:, HD:], x[:, 2 * HD:], out, out, lse, lse.clone(), out.clone(), out.clone(),
                            out.clone(), rows, coef, 3 * HD, 3 * HD, 3 * HD, HD, HD, HD, HD, HD, B, H, T, T,
                            causal=True)
    with pytest.raises(_lib.TT2Error, match="rows"):   # a short buffer is caught before the launch
        ops.attn_fwd_guided(x, x[:, HD:], x[:, 2 * HD:], out, lse, rows[:1], 3 * HD, 3 * HD, 3 * HD, HD, B, H, T, T)


def test_guided_loss_reduction():
    """term = scale * sum(guided rows) / N, kappa = scale * grad_scale / N, loss_out[0] += term;
    N = 0 (no valid frame) gives term = kappa = 0 and leaves loss_out alone."""
    B, H, Tq, Tk, gh = 3, 3, 131, 133, 2
    g = torch.Generator().manual_seed(5)
    rows = [torch.rand(B * H, Tq, generator=g).cuda() for _ in range(3)]
    for r in rows:
        r.view(B, H, Tq)[:, gh:] = 0   # as the forward leaves the unguided heads
    kl = torch.tensor([133, 70, 0], dtype=torch.int32)
    ql = torch.tensor([131, 40, 17], dtype=torch.int32)
    n = 3 * gh * float((kl.double() * ql.double()).sum())
    want = 10.0 * sum(r.double().sum().item() for r in rows) / n
    term = torch.full((1,), 9.0, device="cuda")
    coef = torch.full((1,), 9.0, device="cuda")
    loss = torch.tensor([2.0, 1.0, 1.0, 1.0], device="cuda")
    seen = []
    for _ in range(2):   # run to run identical
        loss.copy_(torch.tensor([2.0, 1.0, 1.0, 1.0]))
        ops.guided_attn_loss(rows, term, coef, B, H, Tq, Tk, key_len=kl.cuda(), q_len=ql.cuda(), guide_heads=gh,
                             scale=10.0, grad_scale=0.5, loss_out=loss)
        got = (term.item(), coef.item(), loss.tolist())
        assert abs(got[0] - want) < 2e-6 * want
        assert abs(got[1] - 10.0 * 0.5 / n) < 1e-6 * 10.0 * 0.5 / n
        assert abs(got[2][0] - 2.0 - got[0]) < 1e-6 and got[2][1:] == [1.0, 1.0, 1.0]
        seen.append(got)
    assert seen[0] == seen[1]
    # odd row count (scalar loads) agrees with the same data
    ops.guided_attn_loss([r[:, :Tq - 1].contiguous() * 0 + 1 for r in rows[:1]], term, coef, B, H, Tq - 1, Tk,
                         guide_heads=H, scale=1.0)
    assert abs(term.item() - 1.0 / Tk) < 1e-6 / Tk   # mean of ones over Tk keys per row
    # N = 0
    zero = torch.zeros(B, dtype=torch.int32, device="cuda")
    loss.copy_(torch.tensor([2.0, 1.0, 1.0, 1.0]))
    ops.guided_attn_loss(rows, term, coef, B, H, Tq, Tk, key_len=kl.cuda(), q_len=zero, guide_heads=gh, scale=10.0,
                         loss_out=loss)
    assert term.item() == 0.0 and coef.item() == 0.0 and loss.tolist() == [2.0, 1.0, 1.0, 1.0]
