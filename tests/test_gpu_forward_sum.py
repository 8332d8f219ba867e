"""tt2.forward_sum (GPU): forward_sum_loss through autograd against the float64 reference of
tests/_fsum_refs.py with a non-trivial incoming gradient and all three reductions, [B, 1, Ty, Tx]
input and a column slice of a wider buffer, posterior, best_path into regulate.plan, the
beta-binomial prior, and forward + backward + path captured in one graph and replayed after scores
and lengths were overwritten in place.  The bars are _fsum_refs' (judge_soft, judge_reduced,
judge_path)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _fsum_refs as F  # noqa: E402
from tt2 import forward_sum as FS, regulate  # noqa: E402

SHAPE = (70, 33)


@pytest.fixture(scope="module")
def prob():
    return F.problem("random", *SHAPE)


def dev(p):
    return (torch.from_numpy(p["scores"]).cuda(), torch.from_numpy(p["key_len"]).cuda(), torch.from_numpy(p["q_len"]).cuda())


def weights(p, reduction):
    """d reduced / d loss_b, so that the weighted sum below has the gradient grad_loss on loss_b / w_b"""
    tx = np.array([Tx for _, _, Tx in F.utterances(p)], np.float64)
    return np.ones(4) if reduction != "mean" else 1.0 / (np.maximum(tx, 1.0) * 4)


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("layout", ["plain", "b1yx", "slice"])
def test_autograd_against_float64(prob, reduction, layout):
    p = prob
    s, tl, ml = dev(p)
    if layout == "b1yx":
        s = s[:, None].clone()
    elif layout == "slice":
        wide = torch.full((4, SHAPE[0], SHAPE[1] + 9), float("nan"), device="cuda")
        wide[:, :, 4:4 + SHAPE[1]] = s
        s = wide[:, :, 4:4 + SHAPE[1]]
    s.requires_grad_(True)
    out = FS.forward_sum_loss(s, tl, ml, reduction=reduction)
    up = torch.from_numpy(p["grad_loss"]).cuda()
    scale = -1.25
    (out * up).sum().backward() if reduction == "none" else (out * scale).backward()
    assert not F.judge_reduced(p, reduction, out.detach().cpu().numpy() if reduction == "none" else out.item())
    g = (p["grad_loss"] if reduction == "none" else scale * weights(p, reduction)).astype(np.float32)
    loss = FS.forward_sum_loss(s.detach(), tl, ml, reduction="none").cpu().numpy()
    gamma = FS.posterior(s.detach(), tl, ml).gamma.cpu().numpy()
    ds = s.grad.reshape(4, *SHAPE).cpu().numpy()
    fails, worst = F.judge_soft(p, loss, gamma, ds, grad_loss=g)
    assert not fails, fails
    assert s.grad.shape == s.shape and out.requires_grad


def test_posterior_rows_sum_to_one_and_loss_matches(prob):
    s, tl, ml = dev(prob)
    r = FS.posterior(s, tl, ml)
    assert isinstance(r, FS.ForwardSum) and r.gamma.shape == s.shape and r.loss.shape == (4,)
    loss = FS.forward_sum_loss(s, tl, ml, reduction="none")
    assert torch.equal(r.loss, loss)
    rows = r.gamma.double().sum(2).cpu().numpy()
    for b, Ty, Tx in F.utterances(prob):
        live = Ty if Tx else 0
        assert np.abs(rows[b, :live] - 1).max(initial=0) <= 4 * 2.0 ** -24 * Tx
        assert (rows[b, live:] == 0).all()


def test_best_path_feeds_the_length_regulator(prob):
    s, tl, ml = dev(prob)
    h = FS.best_path(s, tl, ml)
    assert isinstance(h, FS.HardAlignment) and h.durations.dtype == torch.int32 and h.path.dtype == torch.int32
    assert h.durations.shape == (4, SHAPE[1]) and h.path.shape == (4, SHAPE[0]) and h.logp.shape == (4,)
    assert not F.judge_path(prob, h.path.cpu().numpy(), h.durations.cpu().numpy(), h.logp.cpu().numpy())
    plan = regulate.plan(h.durations, tl, max_frames=SHAPE[0])
    assert torch.equal(plan.index, h.path)


def test_the_prior_adds_to_the_scores(prob):
    s, tl, ml = dev(prob)
    prior = FS.beta_binomial_prior(tl, ml, SHAPE[1], SHAPE[0])
    assert prior.shape == s.shape and prior.is_cuda
    q = dict(prob, scores=(s + prior).cpu().numpy())
    q.pop("_refs", None)
    loss = FS.forward_sum_loss(s + prior, tl, ml, reduction="none")
    assert not F.judge_reduced(q, "none", loss.cpu().numpy())
    mod = FS.ForwardSumLoss()
    assert not list(mod.parameters())
    assert not F.judge_reduced(q, "mean", mod(s + prior, tl, ml).item())


def test_refusals():
    s = torch.zeros(2, 5, 3, device="cuda")
    for bad in (lambda: FS.forward_sum_loss(s.double()), lambda: FS.forward_sum_loss(s.cpu()),
                lambda: FS.forward_sum_loss(s, reduction="avg"), lambda: FS.forward_sum_loss(s[0]),
                lambda: FS.forward_sum_loss(s, torch.zeros(3, dtype=torch.int32, device="cuda")),
                lambda: FS.forward_sum_loss(torch.zeros(1, 2, 513, device="cuda")),
                lambda: FS.best_path(torch.zeros(1, 4097, 2, device="cuda")), lambda: FS.posterior(s.half())):
        with pytest.raises(ValueError):
            bad()
    assert FS.forward_sum_loss(torch.zeros(0, 5, 3, device="cuda")).item() == 0


def test_forward_backward_and_path_replay_from_one_graph():
    p, q = F.problem("random", *SHAPE), F.problem("sharp", *SHAPE, seed=1)
    q["q_len"], q["key_len"] = p["q_len"][[1, 0, 3, 2]].copy(), p["key_len"][[1, 0, 3, 2]].copy()
    s, tl, ml = dev(p)
    up = torch.from_numpy(p["grad_loss"]).cuda()
    s.requires_grad_(True)

    def step():
        s.grad = None
        loss = FS.forward_sum_loss(s, tl, ml, reduction="none")
        (loss * up).sum().backward()
        h = FS.best_path(s, tl, ml)
        g = FS.posterior(s, tl, ml).gamma
        return loss.detach(), s.grad, h, g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                    # sizes the workspace and autograd's buffers before the capture
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grad, h, gamma = step()
    for prob_ in (q, p):
        with torch.no_grad():
            s.copy_(torch.from_numpy(prob_["scores"]).cuda())
            tl.copy_(torch.from_numpy(prob_["key_len"]).cuda())
            ml.copy_(torch.from_numpy(prob_["q_len"]).cuda())
        graph.replay()
        torch.cuda.synchronize()
        fails, _ = F.judge_soft(prob_, loss.cpu().numpy(), gamma.cpu().numpy(), grad.cpu().numpy())
        assert not fails, fails
        assert not F.judge_path(prob_, h.path.cpu().numpy(), h.durations.cpu().numpy(), h.logp.cpu().numpy(),
                                exact=False)
