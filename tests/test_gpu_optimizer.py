"""Fused Adam + global-norm clip + Noam LR vs an independent
implementation: torch.optim.Adam / AdamW + torch.nn.utils.clip_grad_norm_ + LambdaLR(Noam)
in float64 on the CPU, three steps over a random flat buffer (the third with a gradient
norm below the clip, so no clipping).  Parameters, both moments and the bf16 shadow must
agree to 1e-6 relative (the parameter update itself to 1e-5)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _misc_refs as R  # noqa: E402
from tt2 import ops  # noqa: E402


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def noam(step, d_model, warmup):
    return d_model ** -0.5 * min(step ** -0.5, step * warmup ** -1.5)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_clip_noam_matches_torch(wd):
    n = 65536 + 48                 # flat slots are 16-aligned; exercises the float4 body only
    d_model, warmup, clip, lr = 512, 4.0, 1.0, 1.0
    g = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * s for s in (0.5, 2.0, 1e-4)]   # norms ~128, ~512, ~0.03

    ref = torch.nn.Parameter(p0.double().clone())
    opt_cls = torch.optim.AdamW if wd > 0 else torch.optim.Adam
    opt = opt_cls([ref], lr=lr, betas=(0.9, 0.98), eps=1e-9, weight_decay=wd)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: noam(e + 1, d_model, warmup))

    p = p0.cuda()
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    for gr in grads:
        ref.grad = gr.double().clone()
        torch.nn.utils.clip_grad_norm_([ref], clip)
        opt.step()
        sched.step()
        ops.adam_step(p, gr.cuda(), m, v, shadow, step, n, lr, beta1=0.9, beta2=0.98, eps=1e-9, weight_decay=wd,
                      clip_norm=clip, warmup=warmup, noam=True, d_model=d_model)
        ops.step_bump(step)
        st = opt.state[ref]
        assert rel(p, ref.detach()) < 1e-6
        assert rel(p - p0.cuda(), ref.detach() - p0.double()) < 1e-5
        assert rel(m, st["exp_avg"]) < 1e-6
        assert rel(v, st["exp_avg_sq"]) < 1e-6
        assert torch.equal(shadow, p.bfloat16())
    assert step.item() == 3


# ---------------------------------------------------------------------------------------------
# Scalar tail (n % 4 != 0), grid-stride wrap, caller-supplied norm partials and the gate, against
# tests/_misc_refs.py::ref_adam (validated against torch.optim on the CPU by tests/test_misc_refs.py)
def _f32(x):
    return torch.tensor(x, dtype=torch.float32).item()


# the C ABI takes its hyperparameters as floats: the reference gets the values the kernel is
# given (1 - float(0.98) is 1e-6 off 0.02, which a few tail elements cannot average away)
HYPER = dict(beta1=_f32(0.9), beta2=_f32(0.98), eps=_f32(1e-9), clip_norm=1.0, warmup=4.0, noam=True, d_model=512)
WD = _f32(0.01)
N_WRAP = 8192 * 256 * 4 + 4 * 300 + 3     # the float4 body wraps the 8192-block grid and the tail is live


def _segments(n):
    """(name, slice): the scalar tail (last n % 4), the last full float4, the rest -- compared one
    by one, so a wrong tail is not swamped by the body."""
    n4 = n // 4 * 4
    segs = [("tail", slice(n4, n)), ("last float4", slice(max(n4 - 4, 0), n4)), ("rest", slice(0, max(n4 - 4, 0)))]
    return [(k, s) for k, s in segs if s.stop > s.start]


def _state(n, seed):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g) * 0.05       # weight-sized, so a tail element's own update is resolved
    return g, p0


def _check_segments(n, p, m, v, shadow, p0, rp, rm, rv, what):
    pc, mc, vc = p.cpu(), m.cpu(), v.cpu()
    for name, s in _segments(n):
        w = f"{what}: {name}"
        assert rel(pc[s], rp[s]) < 1e-6, w
        assert rel(pc[s] - p0[s], rp[s] - p0[s].double()) < 1e-5, w
        assert rel(mc[s], rm[s]) < 1e-6, w
        assert rel(vc[s], rv[s]) < 1e-6, w
    assert torch.equal(shadow, p.bfloat16()), what


@pytest.mark.parametrize("wd", [0.0, WD], ids=["adam", "adamw"])
@pytest.mark.parametrize("n", [1, 3, 5, 65536 + 48 + 3])
def test_adam_scalar_tail(n, wd):
    """Three steps (the third unclipped) at sizes with a live scalar tail, down to no float4 at all."""
    lr = 1.0
    g, p0 = _state(n, n)
    grads = [torch.randn(n, generator=g) * s for s in (0.5, 2.0, 1e-4)]
    grads[2] *= min(1.0, 0.5 / grads[2].norm().item())     # below the clip at any n
    p, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    rp, rm, rv = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for i, gr in enumerate(grads):
        rp, rm, rv = R.ref_adam(rp, gr, rm, rv, i + 1, lr, weight_decay=wd, **HYPER)
        ops.adam_step(p, gr.cuda(), m, v, shadow, step, n, lr, weight_decay=wd, **HYPER)
        ops.step_bump(step)
        _check_segments(n, p, m, v, shadow, p0, rp, rm, rv, f"n={n} step {i + 1}")
    assert step.item() == 3


def test_adam_grid_stride_wrap_with_tail():
    """One step over more float4s than 8192 x 256 threads, with a 3-element tail."""
    n, lr, wd = N_WRAP, 1.0, WD
    g, p0 = _state(n, 3)
    gr = torch.randn(n, generator=g) * 0.5
    p, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    rp, rm, rv = R.ref_adam(p0, gr, torch.zeros(n), torch.zeros(n), 1, lr, weight_decay=wd, **HYPER)
    ops.adam_step(p, gr.cuda(), m, v, shadow, step, n, lr, weight_decay=wd, **HYPER)
    _check_segments(n, p, m, v, shadow, p0, rp, rm, rv, "wrap")
    # no element left as it was: every float4 of the wrapped range and the tail were visited
    assert (m != 0).sum().item() == (gr != 0).sum().item()


@pytest.mark.parametrize("nparts", [1, 7, 1024])
def test_adam_with_norm_parts(nparts):
    """The clip norm from ops.sumsq_parts instead of the step's own pass: the existing tolerances
    per segment, and per element within 4 x the float32 reference's error (2 ulp floor; worst
    ratio printed; measured on the MI355X: p 0.40, m 0.21, v 0.19).  Integer-valued gradients make
    the squared norm itself exact."""
    n, lr, wd = 65536 + 48 + 3, 1.0, WD
    g, p0 = _state(n, nparts)
    gr = torch.randint(-2, 3, (n,), generator=g).float()
    assert 4.0 * n < R.EXACT_LIMIT
    # a running state with v bounded away from 0: every update is of the same order, so the f32
    # reference's worst error is not that of one or two outliers whose m / sqrt(v) is 1000 x the rest
    # (with v0 down to 0 the ratio of p hung on those elements' roundings: 0.55 to 1.34 by nparts)
    m0, v0 = torch.randn(n, generator=g) * 0.01, (0.5 + torch.rand(n, generator=g)) * 1e-4
    p, m, v = p0.cuda(), m0.cuda(), v0.cuda()
    shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    step = torch.full((1,), 2, dtype=torch.int32, device="cuda")
    parts = torch.empty(nparts, device="cuda")
    ops.sumsq_parts(gr.cuda(), parts, nparts)
    ops.adam_step(p, gr.cuda(), m, v, shadow, step, n, lr, weight_decay=wd, norm_parts=parts, **HYPER)
    rp, rm, rv = R.ref_adam(p0, gr, m0, v0, 3, lr, weight_decay=wd, **HYPER)
    _check_segments(n, p, m, v, shadow, p0, rp, rm, rv, f"norm_parts {nparts}")
    sp, sm, sv = R.ref_adam(p0, gr, m0, v0, 3, lr, weight_decay=wd, dtype=torch.float32, **HYPER)
    ratios = {"p": R.worst_ratio(p, rp, sp), "m": R.worst_ratio(m, rm, sm), "v": R.worst_ratio(v, rv, sv)}
    print(f"adam norm_parts={nparts}: p {R.describe(p, rp, sp)}, m {R.describe(m, rm, sm)}, v {R.describe(v, rv, sv)}")
    assert max(ratios.values()) <= 1.0, ratios


def test_adam_gate():
    """gate = 0: nothing moves; gate = 1: the ungated update bit for bit; adam_gate arms, a consume
    bumps the step once and clears the gate, a second consume changes nothing."""
    n, lr, wd = 1027, 1.0, WD
    g, p0 = _state(n, 17)
    gr = (torch.randn(n, generator=g) * 0.5).cuda()
    m0, v0 = (torch.randn(n, generator=g) * 0.01).cuda(), (torch.rand(n, generator=g) * 1e-4).cuda()

    def run(gate):
        p, m, v = p0.cuda(), m0.clone(), v0.clone()
        shadow = torch.full((n,), 3.0, dtype=torch.bfloat16, device="cuda")
        step = torch.full((1,), 4, dtype=torch.int32, device="cuda")
        ops.adam_step(p, gr, m, v, shadow, step, n, lr, weight_decay=wd, gate=gate, **HYPER)
        assert step.item() == 4                   # the step kernel never bumps the counter itself
        return p, m, v, shadow

    plain = run(None)
    closed = run(torch.zeros(1, dtype=torch.int32, device="cuda"))
    for got, init in zip(closed, (p0.cuda(), m0, v0, torch.full((n,), 3.0, dtype=torch.bfloat16, device="cuda"))):
        assert torch.equal(got, init)
    opened = run(torch.ones(1, dtype=torch.int32, device="cuda"))
    for a, b in zip(opened, plain):
        assert torch.equal(a, b)
    assert not torch.equal(plain[0], p0.cuda())

    gate = torch.zeros(1, dtype=torch.int32, device="cuda")
    step = torch.full((1,), 4, dtype=torch.int32, device="cuda")
    ops.adam_gate(gate, step)                     # consume with nothing pending
    assert (gate.item(), step.item()) == (0, 4)
    ops.adam_gate(gate, step, arm=True)
    assert (gate.item(), step.item()) == (1, 4)
    armed = run(gate)                             # an armed gate lets the update through
    for a, b in zip(armed, plain):
        assert torch.equal(a, b)
    ops.adam_gate(gate, step)
    assert (gate.item(), step.item()) == (0, 5)
    ops.adam_gate(gate, step)
    assert (gate.item(), step.item()) == (0, 5)
    ops.adam_gate(gate, None, arm=True)           # step may be NULL
    ops.adam_gate(gate, None)
    assert gate.item() == 0
