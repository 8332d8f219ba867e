"""tt2.upsample on the GPU: gaussian_upsample through autograd in h, durations, delta and sigma against
float64 (the reference of tests/_upsample_refs.py with the chain rule over centers and the sigma
mapping, itself held to torch float64 autograd of the composed form here), [B, Tx] inputs,
forward_sum.best_path's durations straight in, the hard limit (a large delta reproduces
length_regulate's bits), forward and backward replayed from one captured graph after durations and
lengths changed in place, and the host-read sizing.

The bars of the autograd test: per tensor, the L2 error against float64 over max(4 x the error of the
yardstick of _upsample_refs (the numpy float32 evaluation for f32, the bf16-rounding twin for bf16)
pushed through the same chain rule, 2 ulp of the tensor's scale pushed through it), <= 1 passes.  The
per-row bars are those of tests/test_gpu_upsample_kernels.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _upsample_refs as R  # noqa: E402
from tt2 import forward_sum, ops, regulate, upsample  # noqa: E402

DEV = "cuda"
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}


def composed(h, d, text_len, mel_len, n_out, delta=None, sigma=None, offset=0.0):
    """ESPnet's GaussianUpsampling (arange, cumsum, a broadcast square, masked_fill, softmax, matmul),
    or Non-Attentive Tacotron's weights with sigma; frames at and past mel_len are zero."""
    B, Tx = d.shape
    valid = torch.arange(Tx, device=d.device)[None] < text_len[:, None]
    d = d * valid
    c = torch.cumsum(d, 1) - d / 2
    x = torch.arange(n_out, device=d.device, dtype=d.dtype) + offset
    q = (x[None, :, None] - c[:, None, :]) ** 2
    if sigma is None:
        e = -(delta[:, None, :] if torch.is_tensor(delta) else delta) * q
    else:
        e = -torch.log(sigma)[:, None, :] - q / (2 * sigma[:, None, :] ** 2)
    e = e.masked_fill(~valid[:, None, :], float("-inf"))
    y = torch.softmax(e, -1) @ h
    return y * (torch.arange(n_out, device=d.device)[None] < mel_len[:, None])[:, :, None]


def chain(g, p, d, sig, form):
    """dcenter / dprec / dbias [B, Tx] (float64 numpy) -> (d durations, d delta-or-sigma)."""
    dc = g["dcenter"]
    dd = np.cumsum(dc[:, ::-1], axis=1)[:, ::-1] - dc / 2
    ds = g["dprec"] if form == "delta" else -g["dprec"] / sig ** 3 - g["dbias"] / sig
    return dd, ds


@pytest.mark.parametrize("form", ["delta", "sigma"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_autograd_against_float64(dtype, form):
    n_out, tx, dim = 65, 33, 80
    rng = np.random.default_rng(7)
    B = 4
    text_len = np.array([33, 17, 33, 5])
    d = rng.uniform(0.5, 3.5, size=(B, tx)).astype(np.float32).astype(np.float64)
    sig = rng.uniform(0.5, 2.0, size=(B, tx)).astype(np.float32).astype(np.float64)       # delta or sigma
    if form == "delta":
        sig = sig * 0.2
    h = R._round_in(rng.normal(size=(B, tx, dim)), dtype)
    dy = R._round_in(rng.normal(size=(B, n_out, dim)), dtype)
    mel_len = np.array([65, 40, 33, 68])
    offset = 0.0 if form == "delta" else 1.0

    # the module
    ht = torch.tensor(h, device=DEV).to(TDT[dtype]).requires_grad_(True)
    dt = torch.tensor(d, dtype=torch.float32, device=DEV, requires_grad=True)
    st = torch.tensor(sig, dtype=torch.float32, device=DEV, requires_grad=True)
    kw = dict(delta=st) if form == "delta" else dict(sigma=st)
    res = upsample.gaussian_upsample(ht, dt, torch.tensor(text_len, device=DEV), torch.tensor(mel_len, device=DEV),
                                     max_frames=n_out, offset=offset, **kw)
    assert res.frames.tolist() == [65, 40, 33, 65] and res.out.dtype == TDT[dtype]
    res.out.backward(torch.tensor(dy, device=DEV).to(TDT[dtype]))
    got = {"y": res.out, "dh": ht.grad, "dd": dt.grad, "ds": st.grad}
    got = {k: v.detach().double().cpu().numpy() for k, v in got.items()}

    # float64 torch autograd of the composed form
    h64, d64, s64 = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (h, d, sig))
    kw = dict(delta=s64) if form == "delta" else dict(sigma=s64)
    y64 = composed(h64, d64, torch.tensor(text_len), torch.tensor(mel_len), n_out, offset=offset, **kw)
    y64.backward(torch.tensor(dy))
    want = {"y": y64.detach().numpy(), "dh": h64.grad.numpy(), "dd": d64.grad.numpy(), "ds": s64.grad.numpy()}

    # the kernel-level problem the module hands down: centres in f32 as upsample.centers forms them
    valid = np.arange(tx)[None] < text_len[:, None]
    # (the same torch calls on the same device, so the same bits)
    c32 = upsample.centers(dt.detach(), torch.tensor(text_len, device=DEV)).double().cpu().numpy()
    s_safe = np.where(valid, sig, 1.0)
    s_dev = torch.tensor(s_safe, dtype=torch.float32, device=DEV)
    prec = s_safe if form == "delta" else (0.5 / (s_dev * s_dev)).double().cpu().numpy()
    bias = None if form == "delta" else (-torch.log(s_dev)).double().cpu().numpy()
    p = {"h": h, "dy": dy, "center": c32, "prec": R._f32(prec), "bias": None if bias is None else R._f32(bias),
         "offset": offset, "q_len": list(mel_len), "key_len": list(text_len), "dtype": dtype}
    ref, yard, sc = R.evaluate(p), R.yardstick(p), R.scales(p)

    def tensors(g):
        dd, ds = chain(g, p, d, s_safe, form)
        return {"y": g["y"], "dh": g["dh"], "dd": dd * valid, "ds": ds * valid}
    ref_t = tensors(ref)
    # the reference is torch's float64 autograd up to the f32 rounding of centres, prec and bias
    for k in ref_t:
        assert np.linalg.norm(ref_t[k] - want[k]) <= 1e-4 * np.linalg.norm(want[k]), k
    floor = {"y": sc["y"], "dh": sc["dh"]}                # the magnitudes of what is summed, through the same chain
    floor["dd"] = np.cumsum(sc["dcenter"][:, ::-1], axis=1)[:, ::-1] * valid
    floor["ds"] = (sc["dprec"] if form == "delta" else sc["dprec"] / s_safe ** 3 + sc["dbias"] / s_safe) * valid
    for k in ("y", "dh", "dd", "ds"):
        err = np.linalg.norm(got[k] - ref_t[k])
        ey = max(np.linalg.norm(tensors(y)[k] - ref_t[k]) for y in yard)
        ulp = 2.0 ** -8 if dtype == "bf16" and k in ("y", "dh") else 2.0 ** -23
        allowed = max(4 * ey, 2 * ulp * np.linalg.norm(floor[k]))
        print(f"{form} {dtype} {k}: error {err:.3e}, allowed {allowed:.3e}, ratio {err / allowed:.3f}")
        assert err <= allowed, (k, err, allowed)
    assert not got["dd"][~valid].any() and not got["ds"][~valid].any() and not got["y"][1, 40:].any()


def test_flat_input_and_module():
    rng = np.random.default_rng(3)
    d = torch.tensor(rng.integers(0, 5, size=(3, 12)), device=DEV)
    v = torch.tensor(rng.normal(size=(3, 12)), dtype=torch.float32, device=DEV)
    flat = upsample.gaussian_upsample(v, d, max_frames=40)
    full = upsample.gaussian_upsample(v.unsqueeze(2), d, max_frames=40)
    assert flat.out.shape == (3, 40) and torch.equal(flat.out, full.out.squeeze(2)) and torch.equal(flat.frames, full.frames)
    mod = upsample.GaussianUpsampling(delta=0.1)(v, d, max_frames=40)
    assert torch.equal(mod.out, flat.out) and mod.frames.dtype == torch.int32
    assert flat.frames.tolist() == [min(int(s), 40) for s in d.sum(1)]
    with pytest.raises(ValueError, match="not both"):
        upsample.gaussian_upsample(v, d, delta=0.2, sigma=torch.ones(3, 12, device=DEV))


def test_best_path_durations_go_straight_in():
    torch.manual_seed(0)
    B, ty, tx, D = 3, 50, 12, 16
    scores = torch.randn(B, ty, tx, device=DEV)
    text_len = torch.tensor([12, 7, 10], device=DEV)
    mel_len = torch.tensor([50, 31, 44], device=DEV)
    hard = forward_sum.best_path(scores, text_len, mel_len)
    h = torch.randn(B, tx, D, device=DEV, requires_grad=True)
    up = upsample.gaussian_upsample(h, hard.durations, text_len)          # sized by one host read
    assert up.out.shape == (B, 50, D) and up.frames.tolist() == mel_len.tolist()
    want = composed(h.detach().double(), hard.durations.double(), text_len, mel_len, 50, delta=0.1)
    assert (up.out.double() - want).abs().max().item() < 1e-5
    up.out.sum().backward()
    assert h.grad is not None and not h.grad[1, 7:].any()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_large_delta_is_the_hard_regulator(dtype):
    """Equal durations k, offset 0.5, delta = 200: the nearest other centre is k frames further than
    the frame's own, its weight exp(-200 k (k - 1) ...) underflows to 0, W is one-hot and the output is
    length_regulate's, bit for bit."""
    for k in (1, 2, 3):
        B, tx, D = 2, 21, 40
        h = torch.randn(B, tx, D, device=DEV).to(TDT[dtype])
        d = torch.full((B, tx), k, dtype=torch.int32, device=DEV)
        text_len = torch.tensor([21, 9], device=DEV)
        hard = regulate.length_regulate(h, d, text_len)
        soft = upsample.gaussian_upsample(h, d, text_len, delta=200.0, offset=0.5)
        assert torch.equal(hard.frames, soft.frames) and hard.out.shape == soft.out.shape
        assert torch.equal(hard.out.view(torch.int16 if dtype == "bf16" else torch.int32),
                           soft.out.view(torch.int16 if dtype == "bf16" else torch.int32))


def test_forward_and_backward_replay_in_one_graph():
    """centers, tt2_gauss_upsample_fwd and _bwd into preallocated tensors, captured once; the replay
    follows durations and lengths that were overwritten in place."""
    rng = np.random.default_rng(21)
    B, tx, n_out, D = 3, 20, 90, 24
    h = torch.tensor(rng.normal(size=(B, tx, D)), dtype=torch.float32, device=DEV)
    dy = torch.tensor(rng.normal(size=(B, n_out, D)), dtype=torch.float32, device=DEV)
    dur = torch.zeros(B, tx, dtype=torch.float32, device=DEV)
    text_len = torch.zeros(B, dtype=torch.int32, device=DEV)
    mel_len = torch.zeros(B, dtype=torch.int32, device=DEV)
    prec = torch.full((B, tx), 0.1, device=DEV)
    y, lse = torch.empty(B, n_out, D, device=DEV), torch.empty(B, n_out, device=DEV)
    dh, dc, dp = torch.empty(B, tx, D, device=DEV), torch.empty(B, tx, device=DEV), torch.empty(B, tx, device=DEV)

    def step():
        c = upsample.centers(dur, text_len)
        ops.gauss_upsample_fwd(h, c, prec, y, lse, q_len=mel_len, key_len=text_len)
        ops.gauss_upsample_bwd(h, c, prec, y, lse, dy, dh=dh, dcenter=dc, dprec=dp, q_len=mel_len, key_len=text_len)

    def load(seed):
        r = np.random.default_rng(seed)
        d = r.integers(0, 8, size=(B, tx))
        tl = r.integers(1, tx + 1, size=B)
        ml = np.minimum((d * (np.arange(tx)[None] < tl[:, None])).sum(1), n_out)
        dur.copy_(torch.tensor(d, dtype=torch.float32))
        text_len.copy_(torch.tensor(tl, dtype=torch.int32))
        mel_len.copy_(torch.tensor(ml, dtype=torch.int32))

    load(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for seed in (1, 2, 1):
        load(seed)
        for t in (y, lse, dh, dc, dp):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in (y, lse, dh, dc, dp)]
        step()                                         # the same calls, eagerly
        torch.cuda.synchronize()
        for a, b in zip(replayed, (y, lse, dh, dc, dp)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        want = composed(h.double(), dur.double(), text_len, mel_len, n_out, delta=0.1)
        assert (y.double() - want).abs().max().item() < 1e-5


def test_host_read_sizing():
    rng = np.random.default_rng(5)
    d = torch.tensor(rng.integers(0, 6, size=(4, 15)), device=DEV)
    text_len = torch.tensor([15, 3, 9, 1], device=DEV)
    h = torch.tensor(rng.normal(size=(4, 15, 8)), dtype=torch.float32, device=DEV)
    total = (d * (torch.arange(15, device=DEV)[None] < text_len[:, None])).sum(1)
    auto = upsample.gaussian_upsample(h, d, text_len)
    assert auto.out.shape[1] == int(total.max()) and auto.frames.tolist() == total.tolist()
    fixed = upsample.gaussian_upsample(h, d, text_len, max_frames=auto.out.shape[1])
    assert torch.equal(auto.out, fixed.out) and torch.equal(auto.frames, fixed.frames)
    cut = upsample.gaussian_upsample(h, d, text_len, max_frames=7)
    assert cut.out.shape[1] == 7 and cut.frames.tolist() == [min(int(t), 7) for t in total]
    assert torch.equal(cut.out[0], fixed.out[0, :7])
    mel_len = torch.tensor([10, 2, 0, 30], device=DEV)
    by_len = upsample.gaussian_upsample(h, d, text_len, mel_len=mel_len)
    assert by_len.out.shape[1] == 30 and by_len.frames.tolist() == [10, 2, 0, 30]
    assert not by_len.out[0, 10:].any() and not by_len.out[2].any()
    empty = upsample.gaussian_upsample(h[:0], d[:0])
    assert empty.out.shape == (0, 0, 8) and empty.frames.shape == (0,)
    # floating durations: the frame count is the rounded sum
    f = upsample.gaussian_upsample(h, d.float() + 0.2, text_len)
    assert f.frames.tolist() == torch.round(((d.float() + 0.2) * (torch.arange(15, device=DEV)[None] < text_len[:, None])).sum(1)).int().tolist()
