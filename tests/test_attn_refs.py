"""tests/_attn_refs.py against independent implementations (torch's scaled_dot_product_attention,
autograd, logsumexp), its exact-problem builders at every shape of the GPU test, and the proof
that its bars bite: seven deliberately wrong copies of the twin, each of which the judges that
tests/test_gpu_attention_exact.py applies to the kernels must reject (CPU only)."""
import math

import pytest
import torch
import torch.nn.functional as F

import _attn_refs as R
from _attn_refs import BATCH, HEADS, F64, Twin
from _misc_refs import EXACT_LIMIT

BF16 = torch.bfloat16


# ------------------------------------------------------------------ reference and twin
@pytest.mark.parametrize("causal", [False, True])
def test_ref64_is_sdpa_and_autograd(causal):
    p = R.random_problem(2, 3, 37, 37 if causal else 70, None, causal, torch.float32, seed=1)
    ref = R.ref64(p)
    q, k, v = (t.clone().requires_grad_(True) for t in (p.q, p.k, p.v))
    o = F.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=p.scale)
    (o * p.do).sum().backward()
    s = (p.q @ p.k.transpose(-1, -2)) * p.scale
    if causal:
        s = s.masked_fill(~torch.ones(37, 37, dtype=torch.bool).tril(), -math.inf)
    for got, want in ((ref["o"], o.detach()), (ref["dq"], q.grad), (ref["dk"], k.grad), (ref["dv"], v.grad),
                      (ref["lse"], torch.logsumexp(s, -1) / math.log(2))):
        assert (got - want).abs().max().item() < 1e-12 * max(want.abs().max().item(), 1)


def test_ref64_key_len_and_empty_rows():
    """The header's conventions: key j < min(tk, max(key_len, 0)); empty row: O = 0, LSE = +inf,
    and no gradient flows through it."""
    p = R.random_problem(3, 2, 9, 12, [17, 5, -3], False, torch.float32)
    ref = R.ref64(p)
    cut = R.Problem(p.q[1:2], p.k[1:2, :, :5], p.v[1:2, :, :5], p.do[1:2], None, False, p.scale)
    rc = R.ref64(cut)
    assert torch.allclose(ref["o"][1:2], rc["o"], rtol=0, atol=1e-14)
    assert torch.allclose(ref["dk"][1:2, :, :5], rc["dk"], rtol=0, atol=1e-13)
    assert ref["dk"][1, :, 5:].abs().max() == 0 and ref["dv"][1, :, 5:].abs().max() == 0
    assert ref["o"][2].abs().max() == 0 and torch.isposinf(ref["lse"][2]).all()
    assert all(ref[n][2].abs().max() == 0 for n in R.GRADS)
    full = R.ref64(R.Problem(p.q[:1], p.k[:1], p.v[:1], p.do[:1], None, False, p.scale))
    assert torch.equal(ref["o"][:1], full["o"])


@pytest.mark.parametrize("causal", [False, True])
def test_unrounded_twin_is_the_reference(causal):
    """The twin's explicit backward from the saved LSE is autograd's, when nothing is rounded."""
    p = R.random_problem(2, 3, 70, 70 if causal else 41, [75, 23], causal, BF16, seed=2)
    ref, tw = R.ref64(p), Twin(F64, None)(p)
    for n in ("o", "lse") + R.GRADS:
        fin = torch.isfinite(ref[n])
        assert torch.equal(fin, torch.isfinite(tw[n]))
        assert (tw[n][fin] - ref[n][fin]).abs().max().item() < 1e-12


@pytest.mark.parametrize("case", R.cases(R.RANDOM_ROT), ids=lambda c: c[0])
def test_twin_errors_are_bf16_sized(case):
    """Guards against a twin that is accidentally the reference: wherever the reference is not
    zero, the worst block of the rounded twin is off by bf16 rounding noise (a relative 2^-9 per
    element is 1.1e-3 rms) up to what cancellation in dS adds, and never by nothing."""
    _, tq, tk, causal, kl = case
    p = R.random_problem(BATCH, HEADS, tq, tk, kl, causal, BF16)
    ref, tw = R.ref64(p), Twin()(p)
    many = min(R.visible_counts(p).max().item(), tq) > 1     # a single key: O = V, dV = dO, dS = 0, all exact
    for n in ("o",) + R.GRADS:
        e = R.block_errors(tw[n], ref[n])
        assert torch.isfinite(e).all()
        if many:
            assert 2e-4 < e.max().item() < 0.1, (n, e.max().item())


# ------------------------------------------------------------------ exact-problem builders
@pytest.mark.parametrize("case", R.cases(R.SELECTOR_ROT) + [
    ("issue-131x197", 131, 197, False, [202, 70]), ("issue-causal-131", 131, 131, True, [136, 70])], ids=lambda c: c[0])
def test_selector_problem_is_exact(case):
    """The float64 reference is bf16-representable, equals the closed form (O = V[t] or the mean of
    two), and a float32 evaluation with the twin's roundings returns it bit for bit."""
    _, tq, tk, causal, kl = case
    p = R.selector_problem(BATCH, HEADS, tq, tk, kl, causal)
    ref = R.ref64(p)
    R.assert_exact_problem(ref, case[0])
    t32 = Twin(torch.float32, BF16)(p)
    for n in ("o",) + R.GRADS:
        assert torch.equal(t32[n], ref[n].to(torch.float32).to(F64)), n
    assert R.lse_ratio(t32["lse"], ref["lse"]) <= 1
    # P is one 1 or two 1/2 per live row: l is 1 or 2, so LSE - max score is 0 or 1
    dots = (p.q * p.q).sum(-1)                      # 8192 one-hot, 3 * 8192 pair (q.k = 12288 each), 0 empty
    qlive = R.live_rows(p)[0].expand(BATCH, HEADS, tq)
    c = torch.tensor(p.scale * R.LOG2E, dtype=F64)
    want = torch.where(dots == 8192, 8192 * c, 12288 * c + 1)
    assert set(dots.unique().tolist()) <= {0.0, 8192.0, 24576.0}
    assert torch.equal(dots > 0, qlive)
    assert (ref["lse"][qlive] - want[qlive]).abs().max().item() < 1e-9 if qlive.any() else True
    assert torch.isposinf(ref["lse"][~qlive]).all() and ref["o"][~qlive].abs().sum() == 0
    if not causal and kl is None:               # every residue mod 32 has a second visible key
        frac = (dots == 24576).double().mean().item()
        assert 0.2 < frac < 0.6, frac                # about half the rows are pairs


def test_selector_codes_are_unique():
    k = R.selector_codes(1024)
    assert torch.unique(k, dim=0).shape[0] == 1024
    g = k @ k.T
    assert (g.diagonal() == 8192).all() and (g - torch.diag(g.diagonal())).max() == 4096


@pytest.mark.parametrize("case", R.cases(R.UNIFORM_ROT), ids=lambda c: c[0])
def test_uniform_problem_closed_form(case):
    _, tq, tk, causal, kl = case
    p = R.uniform_problem(BATCH, HEADS, tq, tk, kl, causal)
    ref = R.ref64(p)
    assert torch.equal(ref["lse"], R.log2_count_lse(p))
    assert (ref["o"] - R.uniform_o(p)).abs().max().item() < 1e-14
    assert (p.v.abs().sum(2).max() < EXACT_LIMIT) and ref["dk"].abs().max() == 0     # integer sums are exact in f32
    # rows with a power-of-two count: the backward is exact too, so a float32 evaluation returns the
    # float64 twin's dQ bit for bit, with the bf16 roundings and without any
    n = R.visible_counts(p)
    rows = ((n > 0) & ((n & (n - 1)) == 0))[:, None, :].expand(BATCH, HEADS, tq)
    for rnd in (BF16, None):
        assert torch.equal(Twin(torch.float32, rnd)(p)["dq"][rows], Twin(F64, rnd)(p)["dq"][rows])
    assert torch.equal(Twin(F64, None)(p)["dq"][rows], ref["dq"][rows])


# ------------------------------------------------------------------ checkers
def test_checkers():
    ref = torch.tensor([1.0, 2.0, -3.0, math.inf, 0.0])
    out = torch.tensor([1.0 + 2.0 ** -7, 2.0, -3.0 - 2.0 ** -5, math.inf, 0.0])
    assert R.ulp_distance(out, ref, BF16).tolist() == [1.0, 0.0, 2.0, 0.0, 0.0]
    assert R.ulp_distance(torch.tensor([math.nan, 1.0]), torch.tensor([1.0, math.inf]), BF16).tolist() == [math.inf] * 2
    r = torch.zeros(1, 2, 40, 64, dtype=F64)
    r[0, 0] = 1.0
    o = r.clone()
    o[0, 0, 35] = 1.1                               # one bad row of head 0, in its second block
    e = R.block_errors(o, r)
    assert e.shape == (1, 2, 2) and e[0, 0, 0] == 0 and abs(e[0, 0, 1].item() - 0.1 / math.sqrt(8)) < 1e-12 and (e[0, 1] == 0).all()
    o[0, 1, 3, 5] = 1e-30                           # anything where the reference is all zero
    assert R.block_errors(o, r)[0, 1, 0] == math.inf
    o[0, 1, 3, 5] = math.nan
    assert R.block_errors(o, r)[0, 1, 0] == math.inf
    yard = r * (1 + 1e-3)
    assert R.worst_ratio(yard, r, yard) == pytest.approx(0.5) and R.worst_ratio(r * (1 + 3e-3), r, yard) > 1
    assert R.worst_ratio(o, r, yard) == math.inf
    y2 = r * (1 + 3e-3)                             # a list of yardsticks: the worst of them per block
    assert R.worst_ratio(r * (1 + 5e-3), r, [yard, y2]) < 1 < R.worst_ratio(r * (1 + 7e-3), r, [yard, y2])
    assert R.lse_ratio(torch.tensor([1.0, math.inf]), torch.tensor([1.0, math.inf], dtype=F64)) == 0
    assert R.lse_ratio(torch.tensor([1.0, 5.0]), torch.tensor([1.0, math.inf], dtype=F64)) == math.inf
    assert R.lse_ratio(torch.tensor([1.0 + 2.0 ** -20]), torch.tensor([1.0], dtype=F64)) > 1


# ------------------------------------------------------------------ mutants
class KeyLimitOffByOne(Twin):          # j <= limit for j < limit
    def visible(self, p):
        B, H, Tq, Tk = p.shape
        kl = None if p.key_len is None else [min(max(x, 0), Tk) + 1 for x in p.key_len]
        return R.visible(B, Tq, Tk, kl, p.causal)


class CausalStrict(Twin):              # j < t for j <= t
    def visible(self, p):
        B, H, Tq, Tk = p.shape
        vis = R.visible(B, Tq, Tk, p.key_len, False)
        return vis & (torch.arange(Tk)[None, :] < torch.arange(Tq)[:, None]) if p.causal else vis


class SkipLastTile(Twin):              # one 32-row block of one (batch, head) never walks its last 64-key tile
    def visible(self, p):
        B, H, Tq, Tk = p.shape
        vis = super().visible(p).expand(B, H, Tq, Tk).clone()
        if Tk > 64:
            vis[0, 1, 32:64, 64 * ((Tk - 1) // 64):] = False
        return vis


class NoRescale(Twin):                 # l is not multiplied by exp2(m_old - m_new) when the running maximum rises
    def stats(self, x):
        m = torch.full_like(x[..., :1], -R.INF)
        l = torch.zeros_like(m)
        for k0 in range(0, x.shape[-1], 64):
            t = x[..., k0:k0 + 64]
            m = torch.maximum(m, t.amax(-1, keepdim=True))
            l = l + torch.exp2(t - torch.where(torch.isfinite(m), m, torch.zeros_like(m))).sum(-1, keepdim=True)
        return torch.where(torch.isfinite(m), m, torch.zeros_like(m)), l


class HeadsSwapped(Twin):              # heads 0 and 1 of batch 1 land in each other's output columns
    def saved(self, o_acc, o, lse):
        o = o.clone()
        o[1, [0, 1]] = o[1, [1, 0]]
        return o, o, lse


class UnroundedDs(Twin):               # dS kept in f32 for dQ / dK, and delta from the unrounded O
    def round_ds(self, ds):
        return ds

    def saved(self, o_acc, o, lse):
        return o_acc, o, lse


class LseExtraKey(Twin):               # the saved LSE counts one key too many (l + 1)
    def lse(self, m, l):
        return super().lse(m, torch.where(l > 0, l + 1, l))


MUTANTS = [KeyLimitOffByOne, CausalStrict, SkipLastTile, NoRescale, HeadsSwapped, UnroundedDs, LseExtraKey]
# two shapes of the GPU test with a short key_len: three key tiles and a causal mask between them
MUTANT_SHAPES = [(131, 193, False, [198, 97]), (129, 129, True, [134, 65])]
_cache = {}


def _problems():
    """[(problem name, Problem, ref64, twin, float32 evaluation's LSE)], built once."""
    if not _cache:
        rows = []
        for tq, tk, causal, kl in MUTANT_SHAPES:
            for name, p in (("selector", R.selector_problem(BATCH, HEADS, tq, tk, kl, causal)),
                            ("uniform", R.uniform_problem(BATCH, HEADS, tq, tk, kl, causal)),
                            ("random", R.random_problem(BATCH, HEADS, tq, tk, kl, causal, BF16))):
                rows.append((name, p, R.ref64(p), Twin()(p), Twin(torch.float32, None)(p)["lse"]))
        _cache["rows"] = rows
    return _cache["rows"]


def _judge(name, out, p, ref, tw, lse32):
    if name == "selector":
        return R.judge_selector(out, ref, p, BF16)
    if name == "uniform":
        return R.judge_uniform(out, ref, tw, p, BF16)
    return R.judge_random(out, ref, tw, lse32, p, BF16)


def test_the_twin_itself_passes_every_judge():
    for name, p, ref, tw, lse32 in _problems():
        fails, figs = _judge(name, tw, p, ref, tw, lse32)
        assert not fails, (name, fails)


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: m.__name__)
def test_mutant_is_rejected(mutant):
    """Each wrong copy of the twin misses a bar on at least one of the three problems.  Printed
    (pytest -s): the problems that reject it, and whether the whole-tensor bars of
    tests/test_gpu_attention.py (rel < 1e-2 forward, < 2e-2 backward, random inputs) accept it.

    Measured (B = 2, H = 3; 131 x 193 non-causal and 129 x 129 causal, key_len [T + 5, T / 2]):
      KeyLimitOffByOne  rejected by uniform and random, both shapes              old bar rejects
      CausalStrict      rejected by selector, uniform and random, causal shape   old bar rejects
      SkipLastTile      rejected by uniform and random, non-causal shape         old bar rejects
      NoRescale         rejected by selector and random, both shapes             old bar rejects
      HeadsSwapped      rejected by all three, both shapes                       old bar rejects
      LseExtraKey       rejected by all three, both shapes                       old bar rejects
      UnroundedDs       rejected by uniform, causal shape                        old bar accepts
    (at these shapes one 32-row block is a thirtieth of the tensor and half the rows have the short
    key_len, so the whole-tensor bars see the first six too.)
    UnroundedDs rounds less than the kernels do, so under the block bars, which bound the error
    from above, it passes: its worst ratios are 0.43 (dQ) and 0.46 (dK) on the random problem
    against the twin's own 0.50.  What rejects it is the exact part of the uniform problem: on the
    rows whose count of visible keys is a power of two dQ must be the twin's bit for bit
    (uniform_problem), and a dS that was not rounded to bf16 gives another."""
    rejected, old_accepts = [], True
    for name, p, ref, tw, lse32 in _problems():
        out = mutant()(p)
        fails, _ = _judge(name, out, p, ref, tw, lse32)
        if fails:
            rejected.append(f"{name}-{'causal' if p.causal else 'cross'}")
        if name == "random":
            old_accepts &= R.old_global_bar(out, ref)
    print(f"\n{mutant.__name__:18s} rejected by: {', '.join(rejected) or 'nothing':60s} "
          f"old global bar: {'accepts' if old_accepts else 'rejects'}")
    assert rejected
