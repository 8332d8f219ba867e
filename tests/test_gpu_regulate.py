"""tt2.regulate on the GPU: length_regulate and segment_sum through autograd in f32 and bf16 against
the numpy references of tests/_regulate_refs.py (bit for bit; never against torch's atomic
index_add_), [B, Tx] inputs, plan reuse, max_frames=None against max_frames given, round_durations
feeding LengthRegulator, and the three ops-level calls captured in one graph and replayed after the
durations were overwritten in place."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _regulate_refs as R  # noqa: E402
from tt2 import ops, regulate  # noqa: E402

TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}


def to_dev(x, dtype):
    """numpy float32 / bf16 bits -> a cuda tensor of the same bits."""
    if dtype == "f32":
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int16)).cuda().view(torch.bfloat16).clone()


def to_np(t):
    t = t.detach().contiguous().cpu()
    return t.numpy() if t.dtype != torch.bfloat16 else t.view(torch.int16).numpy().view(np.uint16)


def same(got, want):
    return R.reject({"x": to_np(got)}, {"x": np.ascontiguousarray(want)}) == []


@pytest.fixture(scope="module")
def prob():
    """One batch shared by the tests below (left unchanged): B = 4, Tx = 40, durations with zeros and a
    negative, text_len above, inside, at 0; 137 frames at most."""
    rng = np.random.default_rng(11)
    B, tx = 4, 40
    d = rng.integers(0, 8, size=(B, tx)) * (rng.random((B, tx)) < 0.7)
    d[0, 3] = -4
    d[1, 7] = 30
    key_len = [40, 25, 43, 0]
    n_max = max(int(np.maximum(d[b, :R.clamp(k, 0, tx)], 0).sum()) for b, k in enumerate(key_len))
    return dict(B=B, tx=tx, d=d, key_len=key_len, n_max=n_max, rng_seed=12)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("dim", [None, 1, 6, 64])
def test_length_regulate_forward_and_backward(prob, dim, dtype):
    rng = np.random.default_rng(prob["rng_seed"])
    B, tx, n_out = prob["B"], prob["tx"], prob["n_max"] - 9                    # utterance 1 is cut
    p = R.plan_ref(prob["d"], prob["key_len"], tx, n_out)
    assert (p["total"] > p["frames"]).any() and (p["frames"] < n_out).any()
    D = dim or 1
    h_np = (R._from_f32(rng.normal(size=(B, tx, D)), dtype))
    dy_np = R._from_f32(rng.normal(size=(B, n_out, D)) * 2.0 ** rng.integers(-8, 9, size=(B, n_out, D)), dtype)
    shape = (lambda x: x[:, :, 0]) if dim is None else (lambda x: x)
    h = to_dev(shape(h_np), dtype).requires_grad_()
    out = regulate.length_regulate(h, torch.from_numpy(prob["d"]).cuda(), torch.tensor(prob["key_len"]).cuda(), max_frames=n_out)
    assert out.out.dtype == TORCH[dtype] and out.out.shape == shape(np.zeros((B, n_out, D))).shape
    assert same(out.out, shape(R.fwd_ref(h_np, p["index"], tx)))
    assert same(out.index, p["index"]) and same(out.frames, p["frames"])
    assert not out.index.requires_grad and out.out.requires_grad
    out.out.backward(to_dev(shape(dy_np), dtype))
    assert h.grad.dtype == TORCH[dtype] and same(h.grad, shape(R.bwd_model(dy_np, p["ends"], n_out)))
    # .sum().backward(): the gradient arrives expanded; every phoneme's gradient is its duration
    h2 = to_dev(shape(h_np), dtype).requires_grad_()
    regulate.length_regulate(h2, torch.from_numpy(prob["d"]).cuda(), torch.tensor(prob["key_len"]).cuda(),
                             max_frames=n_out).out.float().sum().backward()
    dur = np.diff(p["ends"], axis=1, prepend=0).astype(np.float32)
    assert np.array_equal(h2.grad.float().cpu().numpy(), shape(np.repeat(dur[:, :, None], D, axis=2)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("dim", [None, 5])
def test_segment_sum_forward_and_backward(prob, dim, dtype):
    rng = np.random.default_rng(prob["rng_seed"] + 1)
    B, tx, n_out = prob["B"], prob["tx"], prob["n_max"]
    p = R.plan_ref(prob["d"], prob["key_len"], tx, n_out)
    D = dim or 1
    v_np = R._from_f32(rng.normal(size=(B, n_out, D)) * 2.0 ** rng.integers(-8, 9, size=(B, n_out, D)), dtype)
    ds_np = R._from_f32(rng.normal(size=(B, tx, D)), dtype)
    shape = (lambda x: x[:, :, 0]) if dim is None else (lambda x: x)
    plan = regulate.plan(torch.from_numpy(prob["d"]).cuda(), torch.tensor(prob["key_len"]).cuda(), max_frames=n_out)
    v = to_dev(shape(v_np), dtype).requires_grad_()
    s = regulate.segment_sum(v, plan)
    assert s.shape == shape(np.zeros((B, tx, D))).shape and same(s, shape(R.bwd_model(v_np, p["ends"], n_out)))
    s.backward(to_dev(shape(ds_np), dtype))
    assert same(v.grad, shape(R.fwd_ref(ds_np, p["index"], tx)))


def test_plan_reuse_and_sizing(prob):
    """One plan serves hidden states, pitch and energy; max_frames=None sizes the output to the
    longest utterance with one host read and gives what max_frames= gives."""
    B, tx = prob["B"], prob["tx"]
    d = torch.from_numpy(prob["d"]).cuda()
    lens = torch.tensor(prob["key_len"], dtype=torch.int32).cuda()
    auto = regulate.plan(d, lens)
    assert auto.index.shape == (B, prob["n_max"]) and int(auto.frames.max()) == prob["n_max"]
    given = regulate.plan(d.to(torch.int32), lens.long(), max_frames=prob["n_max"])
    for a, g in zip(auto, given):
        assert torch.equal(a, g)
    want = R.plan_ref(prob["d"], prob["key_len"], tx, prob["n_max"])
    assert R.reject({k: to_np(getattr(auto, k)) for k in want}, want) == []
    assert torch.equal(auto.total, auto.frames)
    h = torch.randn(B, tx, 16, device="cuda")
    pitch = torch.randn(B, tx, device="cuda")
    a = regulate.length_regulate(h, plan=auto)
    b = regulate.length_regulate(pitch, plan=auto)
    assert a.index is auto.index and b.frames is auto.frames
    assert torch.equal(a.out, regulate.length_regulate(h, d, lens).out)
    assert torch.equal(b.out, regulate.length_regulate(pitch, d, lens, max_frames=prob["n_max"]).out)
    # against the textbook form
    for u in range(B):
        k = min(max(prob["key_len"][u], 0), tx)
        rep = torch.repeat_interleave(pitch[u, :k], torch.from_numpy(np.maximum(prob["d"][u, :k], 0)).cuda())
        assert torch.equal(b.out[u, :len(rep)], rep) and not b.out[u, len(rep):].any()
    # a column slice of a wider activation buffer goes in as it is
    wide = torch.randn(B, tx, 48, device="cuda", dtype=torch.bfloat16)
    assert torch.equal(regulate.length_regulate(wide[:, :, 8:24], plan=auto).out,
                       regulate.length_regulate(wide[:, :, 8:24].contiguous(), plan=auto).out)
    # plain means per phoneme: segment_sum(v) / d
    steps = torch.randint(-8, 9, (B, tx), device="cuda").float()          # small integers: every sum is exact
    dur = torch.diff(auto.ends, dim=1, prepend=torch.zeros(B, 1, dtype=torch.int32, device="cuda"))
    mean = regulate.segment_sum(regulate.length_regulate(steps, plan=auto).out, auto) / dur.clamp(min=1)
    assert torch.equal(mean[dur > 0], steps[dur > 0]) and not mean[dur == 0].any()
    empty = regulate.plan(torch.zeros(0, 5, dtype=torch.int32, device="cuda"))
    assert empty.index.shape == (0, 0) and empty.ends.shape == (0, 5)


def test_round_durations_feeds_the_module(prob):
    B, tx = prob["B"], prob["tx"]
    lens = torch.tensor(prob["key_len"]).cuda()
    log_d = torch.log(torch.from_numpy(np.maximum(prob["d"], 0)).float().cuda() + 1.0)
    d = regulate.round_durations(log_d, lens)
    want_d = np.where(np.arange(tx)[None, :] < np.array(prob["key_len"])[:, None], np.maximum(prob["d"], 0), 0)
    assert d.dtype == torch.int32 and np.array_equal(d.cpu().numpy(), want_d)
    h = torch.randn(B, tx, 32, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    mod = regulate.LengthRegulator()
    out = mod(h, d, text_len=lens)
    p = R.plan_ref(want_d, None, tx, prob["n_max"])
    assert same(out.index, p["index"]) and same(out.out, R.fwd_ref(to_np(h), p["index"], tx))
    slow = mod(h, regulate.round_durations(log_d, lens, alpha=2.0), lens)
    assert torch.equal(slow.frames, 2 * out.frames)


def test_the_three_calls_replay_in_one_graph():
    """plan, fwd and bwd into preallocated tensors, captured once; the replay follows durations that
    were overwritten in place."""
    rng = np.random.default_rng(21)
    B, tx, n_out, D = 3, 20, 90, 24
    d1 = rng.integers(0, 7, size=(B, tx))
    d2 = rng.integers(0, 9, size=(B, tx))[:, ::-1].copy()
    key_len = [20, 13, 20]
    h_np = rng.normal(size=(B, tx, D)).astype(np.float32)
    dy_np = rng.normal(size=(B, n_out, D)).astype(np.float32)
    dur = torch.from_numpy(d1).to(torch.int32).cuda()
    lens = torch.tensor(key_len, dtype=torch.int32).cuda()
    h, dy = torch.from_numpy(h_np).cuda(), torch.from_numpy(dy_np).cuda()
    ends = torch.empty(B, tx, dtype=torch.int32, device="cuda")
    index = torch.empty(B, n_out, dtype=torch.int32, device="cuda")
    frames, total = (torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(2))
    y, dh = torch.empty(B, n_out, D, device="cuda"), torch.empty(B, tx, D, device="cuda")

    def step():
        ops.regulate_plan(dur, n_out, key_len=lens, ends=ends, index=index, frames=frames, total=total)
        ops.regulate_fwd(h, index, y)
        ops.regulate_bwd(dy, ends, dh)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for d in (d1, d2, d1):
        dur.copy_(torch.from_numpy(d).to(torch.int32))
        y.fill_(float("nan"))
        dh.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        p = R.plan_ref(d, key_len, tx, n_out)
        got = {"ends": to_np(ends), "index": to_np(index), "frames": to_np(frames), "total": to_np(total)}
        assert R.reject(got, p) == []
        assert same(y, R.fwd_ref(h_np, p["index"], tx)) and same(dh, R.bwd_model(dy_np, p["ends"], n_out))
    assert not np.array_equal(R.plan_ref(d1, key_len, tx, n_out)["index"], R.plan_ref(d2, key_len, tx, n_out)["index"])
