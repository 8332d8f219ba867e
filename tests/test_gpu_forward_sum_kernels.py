"""Forward-sum kernels (tt2_forward_sum_fwd / _bwd / _path) against the references and judges of
tests/_fsum_refs.py (GPU), by direct C-ABI calls on hand-built buffers.  tests/test_fsum_refs.py pins
the reference and shows that the judges reject every mutant, the plain float32 recurrence included.

Setup: B = 4 with a different case per row (q_len / key_len above the size, inside it, 0 and
negative), NaN in every score row >= Ty_b and every score column >= Tx_b, every buffer a strided
region of a flat NaN- (or -77-) poisoned buffer between guard bands with pad columns of a different
width per buffer, and the score base 4 bytes off 16-byte alignment.  After a call every input is
unchanged and every byte outside an output tensor is unchanged.

Problems: "exact" (0 on a planted path, -128 elsewhere: exp(-128) is 0 in f32, so every output is
defined bit for bit), "const" (the hypergeometric closed form), "random" and "sharp" (judged row by
row against float64 with the bar max(4 x the float32 renormalised reference's error, 2 f32 ulp)),
"integer" (full of ties, every path sum exact: the path must equal the reference's).

Measured (MI355X), the worst error / bar ratios over all shapes are in DESIGN.md 5.14.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _fsum_refs as F  # noqa: E402
from tt2 import _lib  # noqa: E402

GUARD = 64
SENT = -77
# + the shapes whose move bits go to the workspace: more than 256 frames at the 512-key capacity,
# more than 1536 at the 256-key one (F.SHAPES holds each capacity with the bits in LDS)
PATH_SHAPES = F.SHAPES + [(300, 260), (1540, 130)]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype.itemsize == 4 else np.uint16)


class Buf:
    """A strided tensor inside a flat poisoned buffer with guard bands."""

    def __init__(self, shape, dtype, strides, shift=0, data=None):
        self.shape, self.dtype, self.strides, self.off = tuple(shape), np.dtype(dtype), tuple(strides), GUARD + shift
        n = 0 if 0 in self.shape else 1 + sum((s - 1) * st for s, st in zip(self.shape, self.strides))
        self.before = np.full(self.off + n + GUARD, SENT if self.dtype == np.int32 else np.nan, dtype=self.dtype)
        if data is not None:
            self.region(self.before)[...] = np.asarray(data).astype(self.dtype, copy=False).reshape(self.shape)
        self.dev = torch.from_numpy(self.before.view(np.int32).copy()).cuda()

    def region(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.off:], self.shape, tuple(s * 4 for s in self.strides))

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.off * 4

    def fetch(self):
        return self.dev.cpu().numpy().view(self.dtype)

    def unchanged(self):
        return np.array_equal(bits(self.fetch()), bits(self.before))

    def result(self):
        """The tensor after the call; asserts that nothing outside it was written."""
        after = self.fetch().copy()
        out = self.region(after).copy()
        self.region(after)[...] = self.region(self.before)
        assert np.array_equal(bits(after), bits(self.before)), "written outside the tensor (pad columns or guard bands)"
        return out


def call(name, a, expect=0):
    L = _lib.lib()
    rc = getattr(L, name)(ctypes.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (name, rc, L.tt2_last_error())
    if expect:
        assert L.tt2_last_error().startswith(name.encode() + b":")


def poisoned_scores(p):
    s = p["scores"].copy()
    for b, Ty, Tx in F.utterances(p):
        s[b, Ty:] = np.nan
        s[b, :, Tx:] = np.nan
    return s


class Run:
    """The buffers of one problem and the three calls on them."""

    def __init__(self, p, scores=None, lens=True, grad=True, hurt=()):
        B, tq, tk = p["scores"].shape
        self.hurt = hurt                      # utterances whose scores are not finite
        self.p, self.B, self.tq, self.tk = p, B, tq, tk
        s_ld, a_ld, d_ld, g_ld = tk + 3, tk + 1, tk + 5, tk + 2
        self.scores = Buf((B, tq, tk), np.float32, (tq * s_ld + 5, s_ld, 1), shift=1,
                          data=poisoned_scores(p) if scores is None else scores)
        self.q_len = Buf((B,), np.int32, (1,), data=p["q_len"]) if lens else None
        self.key_len = Buf((B,), np.int32, (1,), shift=1, data=p["key_len"]) if lens else None
        self.grad = Buf((B,), np.float32, (1,), shift=2, data=p["grad_loss"]) if grad else None
        self.loss = Buf((B,), np.float32, (1,), shift=3)
        self.lse = Buf((B, tq), np.float32, (tq, 1))
        self.alpha = Buf((B, tq, tk), np.float32, (tq * a_ld, a_ld, 1))
        self.dscores = Buf((B, tq, tk), np.float32, (tq * d_ld + 7, d_ld, 1), shift=2)
        self.gamma = Buf((B, tq, tk), np.float32, (tq * g_ld + 2, g_ld, 1), shift=3)
        self.path = Buf((B, tq), np.int32, (tq, 1), shift=1)
        self.durations = Buf((B, tk), np.int32, (tk, 1), shift=2)
        self.logp = Buf((B,), np.float32, (1,))
        L = _lib.lib()
        need = max(L.tt2_forward_sum_bwd_workspace_size(B, tq, tk), L.tt2_forward_sum_path_workspace_size(B, tq, tk), 16)
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def args(self, **override):
        a = _lib.ForwardSumArgs()
        a.scores = self.scores.ptr
        a.q_len = self.q_len.ptr if self.q_len else None
        a.key_len = self.key_len.ptr if self.key_len else None
        a.grad_loss = self.grad.ptr if self.grad else None
        a.loss, a.lse, a.alpha, a.dscores, a.gamma = self.loss.ptr, self.lse.ptr, self.alpha.ptr, self.dscores.ptr, self.gamma.ptr
        a.path, a.durations, a.logp = self.path.ptr, self.durations.ptr, self.logp.ptr
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), self.ws.numel()
        a.s_ld, a.s_bs = self.scores.strides[1], self.scores.strides[0]
        a.a_ld = self.alpha.strides[1]
        a.d_ld, a.d_bs = self.dscores.strides[1], self.dscores.strides[0]
        a.g_ld, a.g_bs = self.gamma.strides[1], self.gamma.strides[0]
        a.batch, a.tq, a.tk = self.B, self.tq, self.tk
        for k, v in override.items():
            setattr(a, k, v)
        return a

    def inputs_unchanged(self):
        return all(b is None or b.unchanged() for b in (self.scores, self.q_len, self.key_len, self.grad))

    def soft(self, **override):
        """fwd then bwd -> loss, lse, gamma, dscores"""
        call("tt2_forward_sum_fwd", self.args(**override))
        call("tt2_forward_sum_bwd", self.args(**override))
        assert self.inputs_unchanged(), "an input was written"
        alpha = self.alpha.result()
        for b, Ty, Tx in F.utterances(self.p):     # alpha is written for n < Ty, t < Te and nowhere else
            Te = min(Ty, Tx)
            if b in self.hurt:
                continue
            assert np.isnan(alpha[b, Ty:]).all() and np.isnan(alpha[b, :, Te:]).all() and not np.isnan(alpha[b, :Ty, :Te]).any()
        return self.loss.result(), self.lse.result(), self.gamma.result(), self.dscores.result()

    def hard(self, **override):
        call("tt2_forward_sum_path", self.args(**override))
        assert self.inputs_unchanged(), "an input was written"
        return self.path.result(), self.durations.result(), self.logp.result()


@pytest.mark.parametrize("tq,tk", F.SHAPES)
def test_exact_problem_bit_for_bit(tq, tk):
    p = F.problem("exact", tq, tk)
    r = Run(p)
    loss, lse, gamma, ds = r.soft()
    path, dur, logp = r.hard()
    assert F.plus_zero(loss) and F.plus_zero(logp) and (ds == 0).all()      # (grad_loss < 0 makes some of them -0)
    assert not F.judge_soft(p, loss, gamma, ds)[0]                             # the padding is +0
    want = np.zeros((4, tq, tk), np.float32)
    for b, Ty, Tx in F.utterances(p):
        assert F.plus_zero(lse[b])
        if p["paths"][b] is None:
            assert (path[b] == -1).all() and (dur[b] == 0).all()
            continue
        want[b, np.arange(Ty), p["paths"][b]] = 1.0
        assert np.array_equal(path[b, :Ty], p["paths"][b]) and (path[b, Ty:] == -1).all()
        assert np.array_equal(dur[b], np.bincount(p["paths"][b], minlength=tk))
    assert np.array_equal(bits(gamma), bits(want))


@pytest.mark.parametrize("tq,tk", [(5, 5), (37, 7), (33, 64), (65, 65), (257, 129), (70, 512), (1030, 130)])
def test_constant_scores_against_the_closed_form(tq, tk):
    p = F.problem("const", tq, tk)
    loss, _, gamma, ds = Run(p).soft()
    fails, worst = F.judge_soft(p, loss, gamma, ds)
    print("const", (tq, tk), "worst error / bar:", worst)
    assert not fails, fails
    for b, Ty, Tx in F.utterances(p):
        if Ty >= Tx > 0:
            want, g = F.closed_form(Ty, Tx)
            r64, r32 = F.references(p)[b]
            assert abs(float(loss[b]) - want) <= max(F.MARGIN * abs(r32["loss"] - r64["loss"]), 2 * F.ulp32(want)) + 1e-12 * want
            assert np.abs(gamma[b, :Ty, :Tx] - g).max() <= max(F.MARGIN * np.abs(r32["gamma"] - r64["gamma"]).max(), 2 * F.ulp32(1.0)) + 1e-12


@pytest.mark.parametrize("tq,tk", F.SHAPES)
@pytest.mark.parametrize("kind", ["random", "sharp"])
def test_random_problems_row_by_row_against_float64(kind, tq, tk):
    p = F.problem(kind, tq, tk)
    loss, lse, gamma, ds = Run(p).soft()
    fails, worst = F.judge_soft(p, loss, gamma, ds)
    print(kind, (tq, tk), "worst error / bar:", {k: round(v, 3) for k, v in worst.items()})
    assert not fails, fails
    for b, Ty, Tx in F.utterances(p):
        want = F.references(p)[b][0]["lse"]
        # the log's argument is a float32 sum (up to 4 half-ulps relative), then one rounded add
        assert np.abs(lse[b, :Ty] - want).max() <= 2 * F.ulp32(np.abs(want).max()) + 4 * 2.0 ** -24 if Ty and Tx else True
        assert F.plus_zero(lse[b, Ty:])


@pytest.mark.parametrize("tq,tk", PATH_SHAPES)
@pytest.mark.parametrize("kind", ["random", "sharp", "integer"])
def test_best_path(kind, tq, tk):
    p = F.problem(kind, tq, tk)
    path, dur, logp = Run(p).hard()
    fails = F.judge_path(p, path, dur, logp, exact=kind != "random")
    assert not fails, fails


def test_no_lengths_and_no_grad_loss_mean_full_size_and_one():
    p = F.problem("random", 37, 7)
    q = dict(p, q_len=np.full(4, 37, np.int32), key_len=np.full(4, 7, np.int32), grad_loss=np.ones(4, np.float32))
    q.pop("_refs", None)
    r = Run(q, lens=False, grad=False)
    loss, _, gamma, ds = r.soft()
    fails, _ = F.judge_soft(q, loss, gamma, ds)
    assert not fails, fails
    assert not F.judge_path(q, *r.hard())


@pytest.mark.parametrize("tq,tk", [(65, 65), (257, 129)])
def test_repeatable_position_independent_and_isolated(tq, tk):
    p = F.problem("random", tq, tk)

    def everything(r):
        return [bits(x) for x in r.soft() + r.hard()]

    first = everything(Run(p))
    again = everything(Run(p))
    assert all(np.array_equal(a, b) for a, b in zip(first, again)), "not repeatable"
    # the utterances in another order
    perm = np.array([1, 3, 0, 2])
    q = dict(p, scores=p["scores"][perm], q_len=p["q_len"][perm], key_len=p["key_len"][perm], grad_loss=p["grad_loss"][perm])
    q.pop("_refs", None)
    moved = everything(Run(q))
    assert all(np.array_equal(a[perm], b) for a, b in zip(first, moved)), "depends on the batch position"
    # NaN and inf inside utterance 0 leave the others as they were
    s = poisoned_scores(p)
    s[0, 0, 0], s[0, min(3, tq - 1), 1] = np.nan, np.inf
    hurt = everything(Run(p, scores=s, hurt=(0,)))
    assert all(np.array_equal(a[1:], b[1:]) for a, b in zip(first, hurt)), "a NaN crossed utterances"


def test_loss_only_call_and_gamma_only_call():
    p = F.problem("random", 257, 129)
    r = Run(p)
    loss, lse, gamma, ds = r.soft()
    r2 = Run(p)
    call("tt2_forward_sum_fwd", r2.args(alpha=None))
    assert np.array_equal(bits(r2.loss.result()), bits(loss)) and np.array_equal(bits(r2.lse.result()), bits(lse))
    assert r2.alpha.unchanged()
    r3 = Run(p)
    call("tt2_forward_sum_fwd", r3.args())
    call("tt2_forward_sum_bwd", r3.args(dscores=None))
    assert np.array_equal(bits(r3.gamma.result()), bits(gamma)) and r3.dscores.unchanged()
    r4 = Run(p)
    call("tt2_forward_sum_fwd", r4.args())
    call("tt2_forward_sum_bwd", r4.args(gamma=None))
    assert np.array_equal(bits(r4.dscores.result()), bits(ds)) and r4.gamma.unchanged()


def test_refused_calls_leave_the_poison_untouched():
    p = F.problem("random", 37, 7)
    r = Run(p)
    outs = (r.loss, r.lse, r.alpha, r.dscores, r.gamma, r.path, r.durations, r.logp)
    for name, kw in (("tt2_forward_sum_fwd", dict(s_ld=6)), ("tt2_forward_sum_fwd", dict(a_ld=6)),
                     ("tt2_forward_sum_fwd", dict(loss=None)), ("tt2_forward_sum_fwd", dict(tk=513)),
                     ("tt2_forward_sum_bwd", dict(d_ld=6)), ("tt2_forward_sum_bwd", dict(g_ld=6)),
                     ("tt2_forward_sum_bwd", dict(workspace_bytes=8)), ("tt2_forward_sum_bwd", dict(alpha=None)),
                     ("tt2_forward_sum_bwd", dict(dscores=None, gamma=None)), ("tt2_forward_sum_bwd", dict(tq=4097)),
                     ("tt2_forward_sum_path", dict(path=None)), ("tt2_forward_sum_path", dict(batch=-1)),
                     ("tt2_forward_sum_path", dict(scores=None))):
        call(name, r.args(**kw), expect=_lib.E_INVALID)
        assert all(o.unchanged() for o in outs), (name, kw)
    big = Run(F.problem("random", 300, 260))
    call("tt2_forward_sum_path", big.args(workspace_bytes=64), expect=_lib.E_INVALID)
    call("tt2_forward_sum_path", big.args(workspace=big.ws.data_ptr() + 4), expect=_lib.E_INVALID)
    assert big.path.unchanged() and big.durations.unchanged() and big.logp.unchanged()


def test_zero_sizes():
    L = _lib.lib()
    for tq, tk in ((0, 5), (5, 0), (0, 0)):
        p = dict(scores=np.zeros((4, tq, tk), np.float32), q_len=np.array([3, 5, 0, -1], np.int32),
                 key_len=np.array([5, 2, 1, 0], np.int32), grad_loss=np.ones(4, np.float32), tq=tq, tk=tk)
        r = Run(p)
        call("tt2_forward_sum_fwd", r.args())
        call("tt2_forward_sum_bwd", r.args())
        call("tt2_forward_sum_path", r.args())
        assert F.plus_zero(r.loss.result()) and F.plus_zero(r.logp.result()) and F.plus_zero(r.lse.result())
        assert (r.path.result() == -1).all() and (r.durations.result() == 0).all()
    r = Run(F.problem("random", 5, 5))
    for name in ("tt2_forward_sum_fwd", "tt2_forward_sum_bwd", "tt2_forward_sum_path"):
        call(name, r.args(batch=0))
    assert all(o.unchanged() for o in (r.loss, r.lse, r.alpha, r.dscores, r.gamma, r.path, r.durations, r.logp))
    assert L.tt2_forward_sum_bwd_workspace_size(0, 5, 5) == 0
