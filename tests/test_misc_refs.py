"""The float64 references of tests/_misc_refs.py against independent implementations (torch
autograd, torch.optim, the oracle's tts_loss), on the CPU: the references are trusted before
tests/test_gpu_misc_kernels.py holds a kernel against them."""
import pytest
import torch
import torch.nn.functional as F

import _misc_refs as R
from tt2_oracle import dropout_keep, tts_loss

F64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("pad_idx", [0, 7])
def test_embedding_refs_match_torch_embedding(pad_idx):
    g = gen(1)
    M, C, V = 300, 36, 80
    ids = torch.randint(0, V, (M,), generator=g)
    table = torch.randn(V, C, generator=g, dtype=F64).requires_grad_(True)
    dout = torch.randn(M, C, generator=g, dtype=F64)
    out = F.embedding(ids, table, padding_idx=pad_idx)
    assert torch.equal(R.ref_embedding_fwd(ids, table.detach(), V), out.detach())
    out.backward(dout)
    ref = R.ref_embedding_bwd(ids, dout, V, pad_idx)
    assert torch.allclose(ref, table.grad, rtol=0, atol=1e-12)
    assert not ref[pad_idx].any()
    # the in-order float32 sum is the float64 sum to f32 accuracy, and equals it on exact inputs
    o32 = R.ref_embedding_bwd_f32_ordered(ids, dout.float(), V, pad_idx)
    assert torch.allclose(o32.double(), ref, rtol=0, atol=1e-5)
    di = torch.randint(-2, 3, (M, C), generator=g).float()
    assert torch.equal(R.ref_embedding_bwd_f32_ordered(ids, di, V, pad_idx).double(),
                       R.ref_embedding_bwd(ids, di, V, pad_idx))


def test_embedding_refs_out_of_range_ids():
    g = gen(2)
    V, C = 80, 8
    ids = torch.tensor([0, V - 1, -1, V, 5, 5, 1000, -7])
    table = torch.randn(V, C, generator=g)
    out = R.ref_embedding_fwd(ids, table, V)
    assert torch.equal(out[[0, 1, 4]], table[[0, V - 1, 5]])
    assert not out[[2, 3, 6, 7]].any()
    dout = torch.randn(8, C, generator=g)
    for f in (R.ref_embedding_bwd, R.ref_embedding_bwd_f32_ordered):
        dt = f(ids, dout, V, 0).double()
        assert not dt[0].any()                                    # pad_idx
        assert torch.allclose(dt[5], (dout[4].double() + dout[5].double()), atol=1e-6)
        assert torch.allclose(dt[V - 1], dout[1].double(), atol=1e-6)
        assert dt.abs().sum(1).count_nonzero() == 2               # nothing from the out-of-range ids


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_posenc_bwd_ref_matches_autograd(p):
    g = gen(3)
    B, T, C = 3, 37, 40
    M = B * T
    x = torch.randn(M, C, generator=g, dtype=F64).requires_grad_(True)
    alpha = torch.tensor(1.7, dtype=F64, requires_grad=True)
    pe = torch.randn(T + 5, C, generator=g, dtype=F64)
    dout = torch.randn(M, C, generator=g, dtype=F64)
    keep = torch.from_numpy(dropout_keep(5, 9, M * C, p)).view(M, C) if p > 0 else None
    rows = torch.arange(M) % T
    out = x + alpha * pe[rows]
    if p > 0:
        out = out * keep / (1 - p)
    out.backward(dout)
    dx, dalpha = R.ref_posenc_bwd(dout, pe, T, keep, 1 / (1 - p))
    assert torch.allclose(dx, x.grad, rtol=1e-14, atol=0)
    assert torch.allclose(dalpha, alpha.grad, rtol=1e-12, atol=0)


def _loss_inputs(g, B, T, NM, hld):
    M = B * T
    heads = torch.randn(M, hld, generator=g, dtype=F64) * 3
    heads[:, NM + 1:] = float("nan")                 # the unused columns must not matter
    after = torch.randn(M, NM, generator=g, dtype=F64)
    target = torch.randn(B, T, NM, generator=g, dtype=F64)
    return heads, after, target


@pytest.mark.parametrize("lens", [[40, 17, 1, 7], [40, 17, 0, 7], [0, 0, 0, 0], [55, 17, 0, 7], [-3, 40, 2, 0]])
@pytest.mark.parametrize("separate", [False, True])
def test_tts_loss_ref_matches_oracle(lens, separate):
    """In-range lengths, and the oracle's own reading of 0, > T and negative ones: the valid
    frames are t < mel_len, the stop label sits at mel_len - 1, the mean is over the valid
    frames (all padded: every term and gradient is zero)."""
    g = gen(4)
    B, T, NM, hld = 4, 40, 8, 11
    heads, after, target = _loss_inputs(g, B, T, NM, hld)
    ml = torch.tensor(lens)
    before = heads[:, :NM].clone().requires_grad_(True)
    stop = heads[:, NM].clone().requires_grad_(True)
    aft = after.clone().requires_grad_(True)
    gs = 0.5
    total, d = tts_loss(before.view(B, T, NM), aft.view(B, T, NM), stop.view(B, T), target, ml, pos_weight=5.0)
    (total * gs).backward()
    loss, g_heads, g_after = R.ref_tts_loss(heads, after, target, ml, NM, 5.0, gs, separate)
    exp = torch.stack([total, d["mel_before"], d["mel_after"], d["stop"]]).detach()
    assert torch.allclose(loss, exp, rtol=1e-12, atol=1e-15)
    assert torch.allclose(g_after, aft.grad, rtol=1e-12, atol=1e-18)
    mel = before.grad if separate else before.grad + aft.grad
    assert torch.allclose(g_heads[:, :NM], mel, rtol=1e-12, atol=1e-18)
    assert torch.allclose(g_heads[:, NM], stop.grad, rtol=1e-10, atol=1e-18)
    assert not g_heads[:, NM + 1:].any()
    assert torch.isfinite(loss).all() and torch.isfinite(g_heads).all()
    if sum(max(0, min(T, n)) for n in lens) == 0:
        assert not loss.any() and not g_heads.any() and not g_after.any()


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_ref_matches_torch_optim(wd):
    def noam(step, d_model, warmup):
        return d_model ** -0.5 * min(step ** -0.5, step * warmup ** -1.5)

    n, d_model, warmup, clip, lr = 1027, 512, 4.0, 1.0, 1.0
    g = gen(11)
    p0 = torch.randn(n, generator=g, dtype=F64)
    grads = [torch.randn(n, generator=g, dtype=F64) * s for s in (0.5, 2.0, 1e-4)]   # the last is not clipped
    ref = torch.nn.Parameter(p0.clone())
    opt_cls = torch.optim.AdamW if wd > 0 else torch.optim.Adam
    opt = opt_cls([ref], lr=lr, betas=(0.9, 0.98), eps=1e-9, weight_decay=wd)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: noam(e + 1, d_model, warmup))
    p, m, v = p0, torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for i, gr in enumerate(grads):
        ref.grad = gr.clone()
        torch.nn.utils.clip_grad_norm_([ref], clip)
        opt.step()
        sched.step()
        p, m, v = R.ref_adam(p, gr, m, v, i + 1, lr, weight_decay=wd, clip_norm=clip, warmup=warmup,
                             d_model=d_model)
        st = opt.state[ref]
        assert torch.allclose(p, ref.detach(), rtol=1e-12, atol=1e-14)
        assert torch.allclose(m, st["exp_avg"], rtol=1e-12, atol=1e-18)
        assert torch.allclose(v, st["exp_avg_sq"], rtol=1e-12, atol=1e-24)
    # the float32 evaluation (the yardstick of the non-exact checks) stays at f32 accuracy
    p32, m32, v32 = R.ref_adam(p0, grads[0], torch.zeros(n), torch.zeros(n), 1, lr, weight_decay=wd,
                               clip_norm=clip, warmup=warmup, d_model=d_model, dtype=torch.float32)
    assert p32.dtype == torch.float32
    p64, _, _ = R.ref_adam(p0, grads[0], torch.zeros(n), torch.zeros(n), 1, lr, weight_decay=wd, clip_norm=clip,
                           warmup=warmup, d_model=d_model)
    assert (p32.double() - p64).abs().max() < 1e-6


def test_small_refs():
    g = gen(5)
    mel = torch.randn(2, 5, 3, generator=g)
    s = R.ref_shift_right(mel)
    assert not s[0].any() and not s[5].any()
    assert torch.equal(s[1:5], mel[0, :4]) and torch.equal(s[6:], mel[1, :4])
    x = torch.randint(-2, 3, (33, 7), generator=g).float()
    d0 = torch.randint(-4, 5, (7,), generator=g).float()
    assert torch.equal(R.ref_colsum(x, 0.5, d0), 0.5 * d0.double() + x.double().sum(0))
    assert torch.equal(R.ref_colsum(x, 0, torch.full((7,), float("nan"))), x.double().sum(0))
    assert R.ref_sumsq(x) == (x.double() ** 2).sum()


def test_yardstick():
    """ulp() is the format's spacing, and worst_ratio() is 1 exactly at the allowed error."""
    one = torch.tensor([1.0, 1.5, 2.0, 0.75, 0.0], dtype=F64)
    assert torch.equal(R.ulp(one, torch.float32), torch.tensor([2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24,
                                                                 2.0 ** -149], dtype=F64))
    assert R.ulp(torch.tensor([1.0], dtype=F64), torch.bfloat16).item() == 2.0 ** -7
    assert R.ulp(torch.tensor([1.0], dtype=F64), torch.float16).item() == 2.0 ** -10
    ref = torch.tensor([1.0, 100.0], dtype=F64)
    d = lambda a, b: ref + torch.tensor([a, b], dtype=F64)   # noqa: E731
    assert R.worst_ratio(d(2.0 ** -22, 0.0), ref, ref) == 1.0                       # the 2 ulp floor, per element
    assert R.worst_ratio(d(0.0, 2.0 ** -22), ref, ref) < 0.02
    ref32 = d(0.0, 1e-4)                                                            # E32 = 1e-4 for the tensor
    assert abs(R.worst_ratio(d(0.0, 4e-4), ref, ref32) - 1.0) < 1e-9                # 4 x the f32 error
    assert abs(R.worst_ratio(d(4e-4, 0.0), ref, ref32) - 1.0) < 1e-9
    assert R.worst_ratio(d(0.0, 8e-4), ref, ref32) > 1.9
    assert R.worst_ratio(torch.tensor([float("nan"), 100.0]), ref, ref32) == float("inf")
