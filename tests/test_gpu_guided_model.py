"""Guided-attention loss through the engine and the model API (GPU): B = 2, 37 phonemes,
70 frames, ragged lengths.  The oracle's guided loss is computed here from the attention
probabilities TransformerTTSOracle.forward(..., return_attn=True) returns ("dec_cross"):

    L_ga = scale * sum_{l, h < heads, n < Ty_b, t < Tx_b} P * W / (|layers| * heads * sum_b Tx_b Ty_b),
    W = 1 - exp(-(t / Tx_b - n / Ty_b)^2 / (2 sigma^2)).

Bars: f32 mode as test_gpu_fullsize.py (each gradient within max(1e-3, 2 x the f32 oracle's own
distance from the float64 oracle), the guided term and the total likewise); bf16 mode as test_gpu_bf16_parity.py (1.5 x
the autocast oracle's own deviation + 2e-3, the two pos.alpha scalar sums 8 x, that file's
criterion unchanged), with the same guided loss on both sides.  The autograd path and the fused
path run the same kernels and differ only in how d(loss)/d(outputs) is staged in f32 (summed
by torch vs folded in the loss kernel): 1e-5 per parameter, test_gpu_autograd.py's bound for
the same pair of paths."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from tt2.config import TTSConfig  # noqa: E402
from tt2.model import TransformerTTS  # noqa: E402
from tt2_oracle import OracleConfig, TransformerTTSOracle, init_deterministic  # noqa: E402

B, TX, TY = 2, 37, 70
GUIDE = dict(sigma=0.4, scale=10.0, heads=2, layers=None)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def batch(seed=1, tls=(37, 20), mls=(70, 41)):
    g = torch.Generator().manual_seed(seed)
    text = torch.randint(1, 80, (B, TX), generator=g)
    tl, ml = torch.tensor(tls), torch.tensor(mls)
    mel = torch.randn(B, TY, 80, generator=g)
    for b in range(B):
        text[b, tl[b]:] = 0
        mel[b, ml[b]:] = 0
    return text, tl, mel, ml


def guided_loss_oracle(pc, tl, ml, sigma=0.4, scale=10.0, heads=2, layers=None):
    layers = range(len(pc)) if layers is None else layers
    dt = pc[0].dtype
    t = torch.arange(TX, dtype=dt)[None, None, :]
    n = torch.arange(TY, dtype=dt)[None, :, None]
    txf, tyf = tl.to(dt).view(B, 1, 1), ml.to(dt).view(B, 1, 1)
    w = 1.0 - torch.exp(-((t / txf - n / tyf) ** 2) / (2 * sigma * sigma))
    w = w * ((torch.arange(TX)[None, None, :] < tl.view(B, 1, 1)) & (torch.arange(TY)[None, :, None] < ml.view(B, 1, 1)))
    total = sum((pc[l][:, :heads] * w[:, None]).sum() for l in layers)
    return scale * total / (len(layers) * heads * (tl * ml).sum())


def run_oracle(oracle, bt, dtype=torch.float32, autocast=False, seed=7, **guide):
    text, tl, mel, ml = bt
    o = copy.deepcopy(oracle).to(dtype)
    o.set_seed(seed)
    m = mel.to(dtype)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        out = o(text, tl, m, ml, return_attn=True)
        base, _ = o.loss(out[:3], m, ml)
        ga = guided_loss_oracle(out[3]["dec_cross"], tl, ml, **guide)
    (base.float() + ga.float()).backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().float() for k, p in
             o.named_parameters()}
    return (base + ga).detach().float(), ga.detach().float(), grads


def gpu_model(oracle, dtype, seed=7, guide=GUIDE):
    m = TransformerTTS(TTSConfig(), dtype=dtype).train()
    m.load_state_dict(oracle.state_dict())
    m.set_seed(seed)
    if guide is not None:
        m.guided_attention(**guide)
    return m


@pytest.fixture(scope="module")
def oracle():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    return init_deterministic(TransformerTTSOracle(OracleConfig()), 21).train()


def fused_grads(m, bt):
    text, tl, mel, ml = bt
    m(text, tl.int(), mel, ml.int())
    total, parts = m.loss()
    m.backward()
    torch.cuda.synchronize()
    return total, parts, m.grads_state_dict()


def test_guided_f32_parity(oracle):
    bt = batch()
    t64, ga64, g64 = run_oracle(oracle, bt, torch.float64)
    t32, ga32, g32 = run_oracle(oracle, bt, torch.float32)
    with torch.no_grad():
        total, parts, gm = fused_grads(gpu_model(oracle, torch.float32), bt)
    print(f"guided term gpu {parts['guided_attn'].item():.7f} oracle f64 {ga64.item():.7f}; total {total.item():.6f} "
          f"vs {t64.item():.6f}")
    assert abs(parts["guided_attn"].item() - ga64.item()) <= max(1e-3, 2 * abs(ga32.item() - ga64.item())) * ga64.item()
    assert abs(total.item() - t64.item()) <= max(1e-3, 2 * abs(t32.item() - t64.item())) * t64.item()
    assert ga64.item() > 0.1   # the term is a real share of the loss at the default scale
    gnorm = torch.sqrt(sum((g.double() ** 2).sum() for g in g64.values()))
    bad, report = [], []
    for k, ref in g64.items():
        if ref.double().norm() < 1e-6 * gnorm:   # conv biases in front of training-mode BatchNorm
            assert gm[k].double().norm() < 1e-5 * gnorm, k
            continue
        e, noise = rel(gm[k], ref), rel(g32[k], ref)
        report.append((e, noise, k))
        if e > max(1e-3, 2 * noise):
            bad.append((k, e, noise))
    report.sort(reverse=True)
    print("worst engine-vs-f64 / f32 noise:", [(f"{a:.2e}", f"{b:.2e}", k) for a, b, k in report[:4]])
    assert not bad, bad
    # the guided term reaches the gradients: without it they differ
    with torch.no_grad():
        _, parts0, g0 = fused_grads(gpu_model(oracle, torch.float32, guide=None), bt)
    assert "guided_attn" not in parts0
    k = "decoder.layers.0.cross_attn.in_proj_weight"   # ... by more than the bar above allows
    assert rel(g0[k], g64[k]) > max(1e-3, 2 * rel(g32[k], g64[k]))


def test_guided_bf16_within_autocast_deviation(oracle):
    RATIO, FLOOR, SCALAR_RATIO = 1.5, 2e-3, 8.0   # test_gpu_bf16_parity.py
    bt = batch(seed=2)
    t_ref, ga_ref, g_ref = run_oracle(oracle, bt)
    t_ac, ga_ac, g_ac = run_oracle(oracle, bt, autocast=True)
    with torch.no_grad():
        total, parts, gm = fused_grads(gpu_model(oracle, torch.bfloat16), bt)
    rows = {"loss.total": (rel(total, t_ref), rel(t_ac, t_ref)),
            "loss.guided": (rel(parts["guided_attn"], ga_ref), rel(ga_ac, ga_ref))}
    for k, r in g_ref.items():
        if r.abs().max() == 0:
            assert gm[k].abs().max().item() < 1e-6, k
            continue
        rows["grad." + k] = (rel(gm[k], r), rel(g_ac[k], r))
    bad = [(k, a, b) for k, (a, b) in rows.items()
           if a > (SCALAR_RATIO if k.endswith("pos.alpha") else RATIO) * b + FLOOR]
    worst = max(rows.items(), key=lambda kv: kv[1][0] / (kv[1][1] + 1e-12))
    print(f"{len(rows)} quantities; loss rows {rows['loss.total']}, {rows['loss.guided']}; worst gpu/autocast: {worst}")
    assert not bad, bad[:8]


def test_guided_autograd_path_matches_fused(oracle):
    bt = batch(seed=3)
    text, tl, mel, ml = bt
    fused = gpu_model(oracle, torch.float32)
    with torch.no_grad():
        total_f, parts_f, _ = fused_grads(fused, bt)
    gf = fused.engine.grads.clone()
    m = gpu_model(oracle, torch.float32)
    out = m(text, tl.int(), mel, ml.int())
    assert out[3] is not None and out[3].requires_grad and out[3].dim() == 0
    total, parts = m.loss(out, mel.cuda(), ml.cuda())
    assert torch.equal(parts["guided_attn"], parts_f["guided_attn"])
    assert abs(total.item() - total_f.item()) < 1e-5 * total_f.item()
    total.backward()
    e = m.engine
    for name in e.lay.slots:
        p = m.slots[name.replace(".", "__")]
        ref = e.lay.view(gf, name)
        if ref.abs().max().item() == 0:
            continue
        assert rel(p.grad, ref) < 1e-5, name
    # the fourth output is differentiable on its own, and scales with the incoming gradient
    m2 = gpu_model(oracle, torch.float32)
    m2(text, tl.int(), mel, ml.int())[3].mul(2.0).backward()
    ga2 = m2.slots["dec0__cq__w"].grad.clone()
    m3 = gpu_model(oracle, torch.float32)
    m3(text, tl.int(), mel, ml.int())[3].backward()
    assert ga2.abs().max().item() > 0 and rel(ga2, 2.0 * m3.slots["dec0__cq__w"].grad) < 1e-6
    # off: the fourth output stays None
    assert gpu_model(oracle, torch.float32, guide=None)(text, tl.int(), mel, ml.int())[3] is None


def _train_model(guide=GUIDE, overlap=True, seed=5):
    torch.manual_seed(0)
    m = TransformerTTS(TTSConfig(), dtype=torch.bfloat16, seed=seed)
    with torch.no_grad():
        g = torch.Generator(device="cuda").manual_seed(0)
        for name, (off, shape, n) in m.engine.lay.slots.items():
            if len(shape) >= 2:
                m.engine.P(name).copy_(torch.randn(shape, generator=g, device="cuda") * 0.02)
        m.engine.sync_shadow()
    m.configure_optimizer(lr=1e-3, warmup=10.0)
    m.engine.wgrad_overlap = overlap
    if guide is not None:
        m.guided_attention(**guide)
    return m.train()


def _cuda(bt):
    text, tl, mel, ml = bt
    return text.cuda(), tl.int().cuda(), mel.cuda(), ml.int().cuda()


def test_guided_captured_step_follows_lengths():
    """One graph, two batches of different lengths: kappa and N come from the device lengths."""
    b1, b2 = _cuda(batch(seed=4)), _cuda(batch(seed=5, tls=(30, 37), mls=(55, 70)))
    a, b = _train_model(), _train_model()
    for m in (a, b):
        m.train_step(*b1)
    run = b.capture_train_step(B, TX, TY)
    for bt in (b1, b2, b1):
        la, lb = a.train_step(*bt).clone(), run(*bt).clone()
        assert torch.isfinite(la).all() and torch.equal(la, lb)
        assert torch.equal(a._last["ga_term"], b._last["ga_term"]) and a._last["ga_term"].item() > 0
    torch.cuda.synchronize()
    assert torch.equal(a.engine.params, b.engine.params)
    # the switch changed: the captured step must be taken again
    b.guided_attention(on=False)
    with pytest.raises(RuntimeError, match="capture_train_step again"):
        run(*b1)


def _grads(m, bt):
    e = m.engine
    m._sync_shadow()
    A = m._stage(*bt)
    e.forward(A)
    e.loss(A)
    e.backward(A)
    torch.cuda.synchronize()
    return e.grads.clone(), A["loss"].clone()


def test_guided_overlapped_backward_bitwise():
    bt = _cuda(batch(seed=6))
    g_in, l_in = _grads(_train_model(overlap=False), bt)
    g_ov, l_ov = _grads(_train_model(overlap=True), bt)
    assert torch.equal(g_in, g_ov) and torch.equal(l_in, l_ov)


def test_guided_off_and_scale_zero_restore_plain_step(tmp_path):
    bt = _cuda(batch(seed=7))
    plain, toggled, zero = _train_model(guide=None), _train_model(), _train_model(guide=dict(GUIDE, scale=0.0))
    toggled.train_step(*bt)
    plain.train_step(*bt)
    toggled.engine.params.copy_(plain.engine.params)   # same state again, guidance now off
    toggled.engine.exp_avg.copy_(plain.engine.exp_avg)
    toggled.engine.exp_avg_sq.copy_(plain.engine.exp_avg_sq)
    toggled.engine.sync_shadow()
    toggled.guided_attention(on=False)
    lp, lt = plain.train_step(*bt).clone(), toggled.train_step(*bt).clone()
    assert torch.equal(lp, lt) and torch.equal(plain.engine.grads, toggled.engine.grads)
    assert torch.equal(plain.engine.params, toggled.engine.params)
    # scale = 0: kappa = 0, every gradient is the plain step's
    g0, l0 = _grads(_train_model(guide=None), bt)
    gz, lz = _grads(zero, bt)
    assert torch.equal(g0, gz) and torch.equal(l0, lz)
    # a checkpoint written with guidance on loads into a model with it off
    on = _train_model()
    on.train_step(*bt)
    path = str(tmp_path / "guided.pt")
    on.save_checkpoint(path)
    off = _train_model(guide=None)
    off.load_checkpoint(path)
    assert torch.equal(on.engine.params, off.engine.params) and off.engine.guide is None
