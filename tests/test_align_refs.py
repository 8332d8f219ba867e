"""tests/_align_refs.py against independent implementations (autograd over a softmax written out
with a looped W, the plain twin, plain float64 formulas), its exact problems at every shape of the
GPU tests, and the proof that its judges bite: deliberately wrong copies (mutants) of the guided
twin and of the numpy models, each of which the judges that tests/test_gpu_guided_exact.py and
tests/test_gpu_align_exact.py apply to the kernels must reject.  How many of them the whole-tensor
bars of tests/test_gpu_guided_attention.py accept is printed (pytest -s): at kappa = 3 they accept
5 of the 30 bf16 mutant runs (the W index mutants confined to one wave's rows at 131 x 193, and g
from the rounded p) and none of the 14 f32 ones (CPU only)."""
import math

import numpy as np
import pytest
import torch

import _align_refs as A
import _attn_refs as R
from _align_refs import F32, Guide, GuidedTwin
from _attn_refs import BATCH, HEADS, F64, Twin

BF16 = torch.bfloat16


# ------------------------------------------------------------------ reference and twin
def test_guided_ref64_is_autograd_over_a_looped_weight():
    gd = Guide((9, 4), 0.4, 1, 3.0)
    p = R.random_problem(2, 2, 9, 7, [12, 5], False, F32, seed=3)
    ref = A.guided_ref64(p, gd)
    q, k, v = (t.clone().requires_grad_(True) for t in (p.q, p.k, p.v))
    total, g_want = 0.0, torch.zeros(2, 2, 9, dtype=F64)
    for b, (tx, ty) in enumerate(((7, 9), (5, 4))):
        for h in range(2):
            prob = torch.softmax((q[b, h] @ k[b, h, :tx].T) * p.scale, -1)
            total = total + ((prob @ v[b, h, :tx]) * p.do[b, h]).sum()
            if h < gd.heads:
                w = torch.tensor([[1 - math.exp(-(t / tx - n / ty) ** 2 / (2 * 0.4 ** 2)) if n < ty else 0.0
                                   for t in range(tx)] for n in range(9)], dtype=F64)
                g = (prob * w).sum(-1)
                total = total + gd.kappa * g.sum()
                g_want[b, h] = g.detach()
    total.backward()
    for got, want in ((ref["g"], g_want), (ref["dq"], q.grad), (ref["dk"], k.grad), (ref["dv"], v.grad)):
        assert (got - want).abs().max().item() < 1e-12
    assert (ref["g"][:, 1] == 0).all() and (ref["g"][1, :, 4:] == 0).all() and ref["g"][0, 0].min() > 0
    assert (ref["delta"] - ((p.do * ref["o"]).sum(-1) + 3.0 * g_want)).abs().max().item() < 1e-12


def test_kappa_zero_and_no_heads_are_the_plain_reference_and_twin():
    p = R.random_problem(2, 3, 70, 41, [75, 23], False, BF16, seed=2)
    base, t0 = R.ref64(p), Twin()(p)
    for gd in (Guide((60, 70), 0.4, 2, 0.0), Guide(None, 0.4, 0, 3.0)):
        ref, tw = A.guided_ref64(p, gd), GuidedTwin(gd)(p)
        for n in ("o", "lse") + R.GRADS:
            assert torch.equal(tw[n], t0[n]), n                  # bit for bit
            fin = torch.isfinite(base[n])
            assert (ref[n][fin] - base[n][fin]).abs().max().item() < 1e-12
    assert (A.guided_ref64(p, Guide(None, 0.4, 0, 3.0))["g"] == 0).all()


def test_unrounded_guided_twin_is_the_reference():
    """The explicit backward dS = P (dP + kappa W - (delta + kappa g)) is autograd's."""
    gd = Guide((75, 40), 0.4, 2, 3.0)
    p = R.random_problem(2, 3, 70, 41, [45, 23], False, BF16, seed=2)
    ref, tw = A.guided_ref64(p, gd), GuidedTwin(gd, F64, None)(p)
    for n in ("o", "lse", "g", "delta") + R.GRADS:
        fin = torch.isfinite(ref[n])
        assert (tw[n][fin] - ref[n][fin]).abs().max().item() < 1e-12, n
    assert (ref["dq"] - R.ref64(p)["dq"]).abs().max().item() > 1e-3      # the guided term weighs in


# ------------------------------------------------------------------ the indicator guide
def test_indicator_predicate_holds_on_the_lengths_in_use():
    """Tx = Ty up to 284 (at 285 the nearest off-diagonal exponent is -148.99, above the -150 the
    predicate asks for: refused below) and the power-of-two ratios of the GPU test's kind."""
    pairs = [(t, t) for t in range(1, 285)] + [(64, 128), (70, 140), (33, 132), (37, 74), (96, 192), (50, 200), (133, 266)]
    margin = math.inf
    for tx, ty in pairs:
        p = R.Problem(torch.zeros(1, 1, ty, 64, dtype=F64), torch.zeros(1, 1, tx, 64, dtype=F64), None, None, None, False, 0.125)
        margin = min(margin, A.assert_indicator(p, Guide(None, A.INDICATOR_SIGMA, 1, 1.0)))
    print(f"\nsmallest off-diagonal exponent: {-150 - margin:.1f}")
    assert margin > 0


@pytest.mark.parametrize("tx,ty,sigma", [(64, 64, 0.4), (285, 285, A.INDICATOR_SIGMA),
                                           (300, 300, 2.0 ** -7)])
def test_indicator_predicate_refuses_other_guides(tx, ty, sigma):
    p = R.Problem(torch.zeros(1, 1, ty, 64, dtype=F64), torch.zeros(1, 1, tx, 64, dtype=F64), None, None, None, False, 0.125)
    with pytest.raises(AssertionError):
        A.assert_indicator(p, Guide(None, sigma, 1, 1.0))


@pytest.mark.parametrize("case", A.exact_cases(), ids=lambda c: c[0])
def test_guided_selector_problem_is_exact(case):
    """The float64 reference is representable (O and gradients bf16, g in {0, 1/2, 1}, delta f32),
    a float32 evaluation with the kernels' roundings returns it bit for bit, at least a quarter of
    the guided rows sit on their diagonal key, and the reference passes its own judge."""
    _, tq, tk, kl, gd = case
    p, ref = A.build_exact_guided(tq, tk, kl, gd)
    t32 = GuidedTwin(gd, F32, BF16)(p)
    for dtype in (BF16, F32):
        out = {n: (x if n == "lse" else x.to(dtype if n in ("o",) + R.GRADS else F32).to(F64)) for n, x in t32.items()}
        fails, _ = A.judge_guided_selector(out, ref, p, gd, dtype)
        assert not fails, fails
    if gd.heads and tq >= 33:
        share = A.diagonal_share(p, gd, ref)
        assert share >= 0.25, share
        assert set(ref["g"].to(F32).unique().tolist()) == {0.0, 0.5, 1.0}
    tx, ty = A.lengths(p, gd)
    assert (ty < tq).any() or tq == 1
    assert (tx < tk).any() or tk == 1


def test_default_selector_problem_is_unchanged():
    a, b = R.selector_problem(2, 3, 70, 65, [65, 35], False), R.selector_problem(2, 3, 70, 65, [65, 35], False, diag=None)
    assert torch.equal(a.q, b.q) and torch.equal(a.v, b.v)
    c = R.selector_problem(2, 3, 70, 65, [65, 35], False, diag=([65, 70], 0.9))
    assert not torch.equal(a.q, c.q) and torch.equal(a.v, c.v) and torch.equal(a.do, c.do)


# ------------------------------------------------------------------ mutants of the guided twin
def mutant(**methods):
    return type("Mutant", (GuidedTwin,), methods)


def _rows_without(limit_rows, limit_heads):
    def rows(self, p):
        B, H, Tq, Tk = p.shape
        tx, ty = A.lengths(p, self.guide)
        r = (tx[:, None] > 0) & ((torch.arange(Tq)[None, :] < ty[:, None]) | (not limit_rows))
        hd = (torch.arange(H) < self.guide.heads) | (not limit_heads)
        return (r[:, None, :] & hd[None, :, None])[..., None]
    return rows


def _local(p):
    """One wave's work: rows 32 .. 63 of head 0 of the last utterance ([B, H, Tq, 1])."""
    B, H, Tq, Tk = p.shape
    m = torch.zeros(B, H, Tq, 1, dtype=torch.bool)
    m[B - 1, 0, 32:64] = True
    return m


def _weight(wrong, local):
    def weight(self, p):
        w, bad = A.guide_weight(p, self.guide, self.dtype), A.guide_weight(p, self.guide, self.dtype, wrong)
        return torch.where(_local(p), bad, w.expand(*p.shape)) if local else bad
    return weight


def _everywhere_or_local(fn, local):
    """fn(self, kap, x) on the local rows (or everywhere), the honest kap * x elsewhere."""
    def term(self, kap, x):
        return torch.where(self._mask, fn(kap, x), kap * x) if local else fn(kap, x)
    return term


class _Masked(GuidedTwin):
    def __call__(self, p):
        self._mask = _local(p)
        return super().__call__(p)


GUIDED_MUTANTS = {}
for _loc in (False, True):
    _tag = " (one wave's rows)" if _loc else ""
    GUIDED_MUTANTS.update({
        "W off by one in n" + _tag: mutant(weight=_weight("n+1", _loc)),
        "W off by one in t" + _tag: mutant(weight=_weight("t+1", _loc)),
        "W off by 4 hi" + _tag: mutant(weight=_weight("4hi", _loc)),
        "Tx / Ty taken as tk / tq" + _tag: mutant(weight=_weight("full", _loc)),
        "kappa g missing from delta" + _tag: type("Mutant", (_Masked,), dict(delta_term=_everywhere_or_local(lambda kap, g: 0 * g, _loc))),
        "sign of the W term" + _tag: type("Mutant", (_Masked,), dict(w_term=_everywhere_or_local(lambda kap, w: -kap * w, _loc))),
    })
GUIDED_MUTANTS.update({
    "kappa on rows >= Ty": mutant(kappa_rows=_rows_without(False, True)),
    "kappa on an unguided head": mutant(kappa_rows=_rows_without(True, False)),
    "g from the rounded p": mutant(g_probs=lambda self, pf: self.r(pf)),
})
EXACT_ONLY_BLIND = {"g from the rounded p"}      # P is 1 or 1/2 there: rounding it changes nothing


def _as_kernel(out, dtype):
    return {n: (x if n in ("lse", "g", "delta") else x.to(dtype).to(F64)) for n, x in out.items()}


def test_guided_judges_reject_every_mutant_and_old_bars_accept_some():
    """Each mutant runs as a float32 'kernel' with the bf16 roundings.  The exact judge must reject
    it on the selector problem (but for the one it cannot see), the per-row / per-block judge on
    the random problem; the honest twin passes both.  The old whole-tensor bars are counted."""
    ex = [c for c in A.exact_cases() if c[0] in ("129x128-h2-k0.5", "70x65-h2-k-2")]
    rnd = [c for c in A.random_cases() if c[1:3] in ((70, 65), (131, 193))]
    assert len(ex) == 2 and len(rnd) == 2
    exact = [(A.build_exact_guided(tq, tk, kl, gd), gd) for _, tq, tk, kl, gd in ex]
    rand = []
    for _, tq, tk, kl, gd in rnd:
        assert 0 < gd.heads < HEADS and gd.q_len is not None and min(gd.q_len) < tq
        p = R.random_problem(BATCH, HEADS, tq, tk, None if kl is None else list(kl), False, BF16)
        rand.append((p, gd, A.guided_ref64(p, gd), GuidedTwin(gd)(p), A.guided_float32_evaluations(p, gd)))
    old_accepts, n_old = 0, 0
    for name, cls in [("honest", GuidedTwin)] + list(GUIDED_MUTANTS.items()):
        by_exact = [bool(A.judge_guided_selector(_as_kernel(cls(gd, F32, BF16)(p), BF16), ref, p, gd, BF16)[0])
                    for (p, ref), gd in exact]
        by_random, old = [], []
        for p, gd, ref, yard, yard32 in rand:
            out = _as_kernel(cls(gd, F32, BF16)(p), BF16)
            by_random.append(bool(A.judge_guided_random(out, ref, yard, yard32, p, gd, BF16)[0]))
            old.append(A.old_guided_bars(out, ref, BF16))
        print(f"\n{name:46s} rejected by exact {by_exact}, by random {by_random}; old bars accept {old}")
        if name == "honest":
            assert not any(by_exact) and not any(by_random) and all(old)
            continue
        assert all(by_random), name
        assert all(by_exact) or name in EXACT_ONLY_BLIND, name
        old_accepts += sum(old)
        n_old += len(old)
    print(f"old whole-tensor bars accept {old_accepts} of {n_old} mutant runs")
    assert old_accepts >= 1


def test_f32_judge_rejects_the_mutants_too():
    """The same on float32 inputs with the float32 yardsticks (no rounding: 'g from the rounded p'
    does not exist there)."""
    _, tq, tk, kl, gd = [c for c in A.random_cases() if c[1:3] == (70, 65)][0]
    p = R.random_problem(BATCH, HEADS, tq, tk, None if kl is None else list(kl), False, F32)
    ref, yard32 = A.guided_ref64(p, gd), A.guided_float32_evaluations(p, gd)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(99))
    inv = torch.argsort(perm)
    old_accepts = 0
    for name, cls in [("honest", GuidedTwin)] + list(GUIDED_MUTANTS.items()):
        if name == "g from the rounded p":
            continue
        out = cls(gd, F32, None)(R.Problem(p.q[..., perm], p.k[..., perm], p.v[..., perm], p.do[..., perm], p.key_len, False, p.scale))
        out = {n: (x if x.dim() == 3 else x[..., inv]) for n, x in out.items()}     # an order no yardstick has
        fails, figs = A.judge_guided_random(out, ref, yard32, yard32, p, gd, F32)
        print(f"\n{name:46s} {R.show(figs)}")
        assert bool(fails) == (name != "honest"), (name, fails)
        old_accepts += name != "honest" and A.old_guided_bars(out, ref, F32)
    print(f"old f32 bars accept {old_accepts} of {len(GUIDED_MUTANTS) - 1} mutants")


def test_random_and_diagonal_cases_are_what_the_gpu_test_needs():
    """A guided head, an unguided head and a row >= Ty exist somewhere among the random cases; the
    diagonal problem's g is small."""
    cases = A.random_cases()
    assert {c[4].heads for c in cases} == set(A.GUIDE_HEADS)
    _, tq, tk, kl, gd = [c for c in cases if c[1:3] == (131, 193)][0]
    p = A.random_diagonal_problem(BATCH, HEADS, tq, tk, None if kl is None else list(kl), gd, BF16)
    plain = R.random_problem(BATCH, HEADS, tq, tk, None if kl is None else list(kl), False, BF16)
    g, g0 = A.guided_ref64(p, gd)["g"], A.guided_ref64(plain, gd)["g"]
    live = ~A.zero_rows(p, gd)
    assert g[live].median() < 0.05 * g0[live].median(), (g[live].median(), g0[live].median())


# ------------------------------------------------------------------ tt2_guided_attn_loss
def test_loss_model_is_the_header_formula():
    for c in A.LOSS_CASES:
        rows = A.loss_rows(c)
        term, coef, loss = A.loss_model(c, rows)
        kl = [c["tk"]] * c["B"] if c["key_len"] is None else c["key_len"]
        ql = [c["tq"]] * c["B"] if c["q_len"] is None else c["q_len"]
        n = c["L"] * c["gh"] * sum(min(max(a, 0), c["tk"]) * min(max(b, 0), c["tq"]) for a, b in zip(kl, ql))
        total = rows[:, :, :c["gh"]].sum().item()
        assert torch.isnan(rows[:, :, c["gh"]:]).all()
        if n == 0:
            assert term == 0 and coef == 0 and (loss is None or loss == np.float32(c["loss0"]))
            continue
        assert abs(term - c["scale"] * total / n) <= 1e-7 * abs(term) and abs(coef - c["scale"] * c["grad_scale"] / n) <= 1e-7 * coef
        assert c["loss0"] is None or loss == np.float32(np.float32(c["loss0"]) + term)
    names = {c["name"]: c for c in A.LOSS_CASES}
    assert names["pairs18-below"]["L"] * names["pairs18-below"]["B"] == 18
    assert names["pairs18-below"]["gh"] * names["pairs18-below"]["tq"] < 256 < names["pairs18-above"]["gh"] * names["pairs18-above"]["tq"]
    assert names["odd-tq"]["tq"] % 2 == 1 and names["misaligned"]["offset"] == 1
    # pair 17 (index 16, the first of the 16 waves' second trip) skipped: another term
    for name in ("pairs18-below", "pairs18-above"):
        c = names[name]
        rows = A.loss_rows(c)
        assert A.loss_model(c, rows, drop_pair=16)[0] != A.loss_model(c, rows)[0]


# ------------------------------------------------------------------ tt2_attn_align
ALIGN_SHAPES = [(tq, tk, R.key_len_options(tk)[i % 4]) for i, (tq, tk) in enumerate(R.CROSS_TQ_TK)]


def _b4(kl):
    """key_len of B = 4 from a B = 2 option."""
    return None if kl is None else list(kl) + list(kl)[::-1]


def test_align_exact_problem_and_tie_mutants():
    """pmax = 2^-m is what a float32 evaluation of the model gives; each tie mutant is rejected on
    some shape; ties exist across the 32-key halves, the lane halves and the 64-key tiles."""
    rejected = {"highest": 0, "halves": 0}
    crossing = {"64-key tiles": False, "lane halves": False, "32-key halves": False}
    for tq, tk, kl in ALIGN_SHAPES:
        q_len = A.align_q_len(tq)
        p, lse = A.align_exact_problem(4, HEADS, tq, tk, _b4(kl))
        want_p, want_a = A.align_exact_expected(p, lse, q_len)
        s = A.masked_scores(p)
        x = (s.amax(-1).clamp_min(0).numpy().astype(np.float32) * A.kernel_c(p.scale)) - lse.numpy().astype(np.float32)
        with np.errstate(over="ignore"):
            model = torch.from_numpy(np.exp2(x).astype(np.float64))
        ok = want_a >= 0
        assert torch.equal(model[ok], want_p[ok]) and (want_p[~ok] == 0).all()
        assert set(want_p[ok].unique().tolist()) <= {1.0, 0.5, 0.25, 0.125}
        assert not A.judge_align_exact(want_p, want_a, want_p, want_a)
        for rule in rejected:
            mp, ma = A.align_exact_expected(p, lse, q_len, rule)
            rejected[rule] += bool(A.judge_align_exact(mp, ma, want_p, want_a))
        if tk > 1:
            top = (s == s.amax(-1, keepdim=True)) & torch.isfinite(s)
            t = torch.arange(tk)
            first = torch.where(top, t, torch.full_like(top, tk, dtype=torch.long)).amin(-1, keepdim=True)
            other = top & (t != first)
            crossing["64-key tiles"] |= bool((other & (t // 64 != first // 64)).any())
            crossing["lane halves"] |= bool((other & ((t >> 2) & 1 != (first >> 2) & 1)).any())
            crossing["32-key halves"] |= bool((other & (t // 32 != first // 32) & (t // 64 == first // 64)).any())
    assert all(crossing.values()), crossing
    print(f"\ntie mutants rejected on {rejected} of {len(ALIGN_SHAPES)} shapes")
    assert all(v >= 3 for v in rejected.values())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_align_random_seeds_meet_the_gap_cap(dtype):
    """The float64 reference alone: rows under the top-2 gap are <= 0.5 % of the valid rows, the
    reference passes its own judge (printed: where a held-out float32 evaluation sits, which shows
    how tight the per-row bar is), and a relative 1e-5 on every row fails it."""
    for tq, tk, kl in ALIGN_SHAPES:
        p = R.random_problem(4, HEADS, tq, tk, _b4(kl), False, dtype)
        ref = A.align_random_reference(p, A.align_q_len(tq))
        under = int((ref["gap"][ref["valid"]] < A.GAP).sum())
        assert under <= 0.005 * int(ref["valid"].sum()), (tq, tk, under)
        amax = torch.where(ref["valid"], ref["top2"][..., 0], torch.full_like(ref["top2"][..., 0], -1))
        assert not A.judge_align_random(ref["pmax"], amax, ref)[0]
        held = dict(ref, evals=ref["evals"][:6] + ref["evals"][8:])          # without one order's two
        worst = max(A.judge_align_random(pm, amax, held)[1]["pmax"] for pm in ref["evals"][6:8])
        print(f"\n{tq}x{tk} {dtype}: a held-out float32 evaluation sits at {worst:.3f} of the bar")
        assert worst <= 1
        if ref["valid"].any() and tk > 1:
            fails, _ = A.judge_align_random(ref["pmax"] * (1 + 1e-5), amax, ref)
            assert fails


# ------------------------------------------------------------------ tt2_align_durations
def test_durations_model_against_plain_formulas_and_its_mutants():
    caught = {m: [] for m in ("chunk", "pair", "inv_tq", "past_len", "high_tie")}
    for c in A.DUR_CASES:
        pmax, amax = A.durations_inputs(c)
        want = A.durations_model(c, pmax, amax)
        L, B, H, tq, tk = (c[k] for k in ("L", "B", "H", "tq", "tk"))
        ty = R.key_limits(B, tq, c["q_len"]).tolist()
        for b in range(B):
            mean = pmax[:, b, :, :ty[b]].mean(-1) if ty[b] else torch.zeros(L, H, dtype=F64)
            assert np.allclose(want["focus"][:, b], mean.numpy(), rtol=2e-7, atol=0)
            sl, sh = want["sel"][b]
            assert want["focus"][sl, b, sh] == want["focus"][:, b].max() or c["head"] is not None
            klim = tk if c["key_len"] is None else min(tk, c["key_len"][b])
            assert want["durations"][b, max(klim, 0):].sum() == 0
            a = amax[sl, b, sh, :ty[b]]
            assert want["durations"][b].sum() == int(((a >= 0) & (a < klim)).sum())
            assert not torch.isnan(pmax[:, b, :, :ty[b]]).any() and (ty[b] == tq or torch.isnan(pmax[:, b, :, ty[b]:]).all())
        assert not A.judge_durations(want, want)
        for m in caught:
            if A.judge_durations(A.durations_model(c, pmax, amax, m), want):
                caught[m].append(c["name"])
    print(f"\ndurations mutants caught on: {caught}")
    assert all(caught.values()), caught
    assert "keys4100" in caught["chunk"] and "rows1030" in caught["inv_tq"] and "pairs17" in caught["pair"]
    names = {c["name"]: c for c in A.DUR_CASES}
    assert names["pairs1024"]["L"] * names["pairs1024"]["H"] == 1024 and names["pairs17"]["L"] * names["pairs17"]["H"] == 17
