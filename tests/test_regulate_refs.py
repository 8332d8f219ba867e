"""CPU: the references of the length regulator (tests/_regulate_refs.py) against brute force -- the
plan and the forward against np.repeat per utterance, the backward against float64 torch autograd of
a gather, the plan's index against the MonotonicAlignment.path convention -- then the premises of the
GPU tests' problem sets (exact problems are exact, mixed problems are order-sensitive), the bar
against every mutant on those sets, and round_durations against hand-computed values."""
import numpy as np
import pytest
import torch

import _regulate_refs as R


def test_plan_and_forward_equal_repeat_per_utterance():
    rng = np.random.default_rng(0)
    for tx in (0, 1, 2, 5, 17):
        for n_out in (0, 1, 9, 40):
            for trial in range(6):
                B = 3
                d = rng.integers(-2, 6, size=(B, tx))
                key_len = [None, rng.integers(-2, tx + 3, size=B).tolist()][trial % 2]
                p = R.plan_ref(d, key_len, tx, n_out)
                index, frames, total = R.plan_brute(d, key_len, tx, n_out)
                assert np.array_equal(p["index"], index) and p["frames"].tolist() == frames and p["total"].tolist() == total
                h = rng.normal(size=(B, tx, 3)).astype(np.float32)
                y = R.fwd_ref(h, p["index"], tx)
                for b in range(B):
                    txb = tx if key_len is None else R.clamp(key_len[b], 0, tx)
                    rep = np.repeat(h[b, :txb], np.maximum(d[b, :txb], 0), axis=0)[:n_out]
                    assert np.array_equal(y[b, :len(rep)], rep) and not y[b, len(rep):].any()
                    # ends: the clamped running sum, constant from Tx_b - 1 on
                    want = np.minimum(np.cumsum(np.maximum(np.where(np.arange(tx) < txb, d[b], 0), 0)), n_out)
                    assert np.array_equal(p["ends"][b], want)


def test_plan_known_answers():
    p = R.plan_ref([[2, 0, 3, 0]], None, 4, 7)
    assert p["ends"].tolist() == [[2, 2, 5, 5]] and p["index"].tolist() == [[0, 0, 2, 2, 2, -1, -1]]
    assert p["frames"].tolist() == [5] and p["total"].tolist() == [5]
    p = R.plan_ref([[2, 0, 3, 0]], None, 4, 4)                       # cut at n_out: total > frames
    assert p["ends"].tolist() == [[2, 2, 4, 4]] and p["index"].tolist() == [[0, 0, 2, 2]]
    assert p["frames"].tolist() == [4] and p["total"].tolist() == [5]
    p = R.plan_ref([[R.INT32_MAX, -4, R.INT32_MAX]], None, 3, 5)      # nothing wraps
    assert p["ends"].tolist() == [[5, 5, 5]] and p["total"].tolist() == [R.INT32_MAX] and p["index"].tolist() == [[0] * 5]
    p = R.plan_ref([[1, 1, R.HUGE]], [2], 3, 5)                      # key_len: the third entry is not read
    assert p["ends"].tolist() == [[1, 2, 2]] and p["index"].tolist() == [[0, 1, -1, -1, -1]]
    p = R.plan_ref([[3, 3]], [-1], 2, 2)
    assert p["ends"].tolist() == [[0, 0]] and p["index"].tolist() == [[-1, -1]] and p["total"].tolist() == [0]
    p = R.plan_ref([[], []], None, 0, 2)
    assert p["ends"].shape == (2, 0) and p["index"].tolist() == [[-1, -1]] * 2 and p["frames"].tolist() == [0, 0]


def test_index_is_the_monotonic_path_convention():
    """MonotonicAlignment.path[b, n] is the phoneme of frame n, nondecreasing, -1 past the utterance;
    durations are its histogram.  The plan of that histogram gives the path back."""
    path = np.array([0, 0, 0, 1, 3, 3, 4, 4, 4, 4, 7, -1, -1, -1])
    tx = 9
    durations = np.bincount(path[path >= 0], minlength=tx)
    p = R.plan_ref([durations], None, tx, len(path))
    assert p["index"][0].tolist() == path.tolist() and p["frames"].tolist() == [11]


def test_bf16_rounding_is_torchs():
    rng = np.random.default_rng(3)
    x = (rng.normal(size=4096) * 2.0 ** rng.integers(-20, 20, size=4096)).astype(np.float32)
    x[:6] = [0.0, -0.0, np.inf, -np.inf, 1.00390625, 1.01171875]      # two exact ties: to even
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.f32_to_bf16(x), want)
    assert R.f32_to_bf16(np.float32([1.00390625, 1.01171875])).tolist() == [0x3F80, 0x3F82]
    assert np.array_equal(R.bf16_to_f32(want), torch.from_numpy(want.view(np.int16)).view(torch.bfloat16).float().numpy())


def test_backward_equals_float64_autograd_of_a_gather():
    rng = np.random.default_rng(1)
    B, tx, n_out, D = 3, 7, 30, 4
    d = rng.integers(0, 7, size=(B, tx))
    p = R.plan_ref(d, [7, 5, 9], tx, n_out)
    dy = rng.normal(size=(B, n_out, D)).astype(np.float32)
    h = torch.zeros(B, tx, D, dtype=torch.float64, requires_grad=True)
    idx = torch.from_numpy(p["index"].astype(np.int64))
    y = torch.gather(h, 1, idx.clamp(min=0)[:, :, None].expand(B, n_out, D)) * (idx >= 0)[:, :, None]
    y.backward(torch.from_numpy(dy).double())
    want = h.grad.numpy()
    assert np.array_equal(R.bwd_f64(dy, p["ends"], n_out), want) or np.allclose(R.bwd_f64(dy, p["ends"], n_out), want, rtol=1e-14, atol=0)
    got = R.bwd_model(dy, p["ends"], n_out)
    assert got.dtype == np.float32 and np.allclose(got, want, rtol=0, atol=7 * 2.0 ** -24 * np.abs(dy).sum(axis=1).max())
    # integers: exact, in f32 and through bf16
    dyi = rng.integers(-3, 4, size=(B, n_out, D)).astype(np.float32)
    wi = R.bwd_f64(dyi, p["ends"], n_out)
    assert np.array_equal(R.bwd_model(dyi, p["ends"], n_out), wi)
    assert np.array_equal(R.bf16_to_f32(R.bwd_model(R.f32_to_bf16(dyi), p["ends"], n_out)), wi)
    # an empty segment is +0, not -0, and -0 rows sum to +0 from the +0 start
    z = np.full((1, 4, 1), -0.0, dtype=np.float32)
    out = R.bwd_model(z, np.array([[0, 3, 3]], dtype=np.int32), 4)
    assert R.bits(out).ravel().tolist() == [0, 0, 0]
    # ends outside [0, n_out] are clamped
    out = R.bwd_model(np.ones((1, 4, 1), dtype=np.float32), np.array([[-3, 2, 9]], dtype=np.int32), 4)
    assert out.ravel().tolist() == [0, 2, 2]


@pytest.fixture(scope="module")
def layouts():
    return {name: R.layout(name) for name in R.LAYOUTS}


def test_the_layouts_cover_the_cases(layouts):
    L = layouts["long"]
    assert 1030 in L["durations"][0] and L["plan"]["frames"].tolist() == [1053, 48, 1100, 0]
    assert L["plan"]["total"][2] > L["plan"]["frames"][2]            # cut at n_out
    assert (L["plan"]["index"][0] == -1).sum() == 47
    L = layouts["many"]
    fr = L["plan"]["frames"].tolist()
    assert fr[2] == L["n_out"] and fr[3] == 0 and 0 < fr[1] < fr[0] < L["n_out"]
    assert L["tx"] > 256 and L["n_out"] > 1024                       # more than one work group at dim = 1
    for L in layouts.values():
        for b, k in enumerate(L["key_len"]):
            assert (L["durations"][b, R.clamp(k, 0, L["tx"]):] == R.HUGE).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_problem_premises(layouts, dtype):
    """Exact problems are exact; mixed problems tell ascending from descending from pairwise sums; h
    carries -0, a denormal and both infinities in rows that are copied and NaN in rows that are not."""
    for name, L in layouts.items():
        for dim in R.DIMS:
            ends, n_out = L["plan"]["ends"], L["n_out"]
            dy = R.bwd_exact_problem(L, dim, dtype)
            assert R.is_exact(dy, ends, n_out, dtype), (name, dim)
            want = R.bwd_f64(dy, ends, n_out)
            assert np.array_equal(R._as_f32(R.bwd_model(dy, ends, n_out)).astype(np.float64), want)
            mixed = R.bwd_mixed_problem(L, dim, dtype)
            assert R.order_sensitive(mixed, ends, n_out), (name, dim)
            assert not R.is_exact(mixed, ends, n_out, dtype)
            for b in range(4):                                        # NaN at and past frames, none before
                fr = L["plan"]["frames"][b]
                for x in (dy, mixed):
                    v = R._as_f32(x)[b]
                    assert np.isnan(v[fr:]).all() and not np.isnan(v[:fr]).any()
            h = R.fwd_problem(L, dim, dtype)
            y = R._as_f32(R.fwd_ref(h, L["plan"]["index"], L["tx"]))
            assert not np.isnan(y).any()
            col0 = R.bits(R.fwd_ref(h, L["plan"]["index"], L["tx"]))[:, :, 0]
            for s in R.bits(R.SPECIALS[dtype])[:4]:
                assert (col0 == s).any(), (name, dim, hex(int(s)))
            assert np.isnan(R._as_f32(h)).any()
    assert not R.is_exact(np.full((1, 3, 1), 0.5, dtype=np.float32), np.array([[3]], dtype=np.int32), 3, "f32")
    assert not R.is_exact(np.ones((1, 300, 1), dtype=np.float32), np.array([[300]], dtype=np.int32), 300, "bf16")


_PLAN_CASES = []       # (problem, reference), computed once and left unchanged


def _plan_cases():
    if not _PLAN_CASES:
        for tx in R.PLAN_TX:
            for n_out in R.PLAN_NOUT:
                for p in R.plan_problems(tx, n_out):
                    _PLAN_CASES.append((p, R.plan_ref(p["durations"], p["key_len"], tx, n_out)))
    return _PLAN_CASES


def _plan_rejections(mut):
    return sum(bool(R.reject(R.plan_ref(p["durations"], p["key_len"], p["tx"], p["n_out"], mut=mut), want))
               for p, want in _plan_cases())


@pytest.mark.parametrize("mut", R.PLAN_MUTANTS)
def test_the_bar_rejects_every_plan_mutant(mut):
    assert _plan_rejections(mut) > 0, mut


def test_the_bar_accepts_the_reference_and_the_plan_problems_cover_the_cases():
    assert _plan_rejections(None) == 0
    seen = set()
    for tx in R.PLAN_TX:
        for n_out in R.PLAN_NOUT:
            probs = R.plan_problems(tx, n_out)
            assert len(probs) == 5 and probs[-1]["key_len"] is None
            rows = R.plan_rows(tx, n_out)
            if tx >= 2:
                d, k = rows["huge"]
                assert (d[:k] == R.INT32_MAX).sum() >= 2
                assert R.plan_ref([d], [k], tx, n_out)["total"].tolist() == [R.INT32_MAX]
            if tx >= 8:
                for name, want in (("exact", n_out), ("below", max(n_out - 1, 0)), ("above", n_out + 1)):
                    d, k = rows[name]
                    assert R.plan_ref([d], [k], tx, n_out + 9)["total"].tolist() == [want], (tx, n_out, name)
                d, _ = rows["below"]
                assert not d[:tx // 4].any() and not d[tx - tx // 4:].any()
                assert (rows["above"][0] < 0).any() and (rows["exact"][0] == 0).any()
                d, _ = rows["seams"]
                assert all(d[i] > 0 for i in range(0, tx, 64)) and d[1:min(63, tx - 1)].sum() == 0
            ks = {n: rows[n][1] for n in rows}
            assert ks["exact"] > tx and ks["klen0"] == 0 and ks["kneg"] < 0 and ks["mid"] == tx // 2
            seen.add((tx, n_out))
    assert len(seen) == 40


@pytest.mark.parametrize("mut", R.BWD_MUTANTS)
def test_the_bar_rejects_every_backward_mutant(layouts, mut):
    """On the mixed problems of the GPU test (the exact ones cannot tell the order of a sum)."""
    rejected = 0
    with np.errstate(invalid="ignore"):
        for name, L in layouts.items():
            for dim, dtype in ((3, "f32"), (8, "bf16")):
                dy = R.bwd_mixed_problem(L, dim, dtype)
                want = {"dh": R.bwd_model(dy, L["plan"]["ends"], L["n_out"])}
                got = {"dh": R.bwd_model(dy, L["plan"]["ends"], L["n_out"], mut=mut, key_len=L["key_len"])}
                rejected += bool(R.reject(got, want))
                assert R.reject({"dh": R.bwd_model(dy, L["plan"]["ends"], L["n_out"], mut="none at all")}, want) == []
    assert rejected > 0, mut


def test_mutant_list_is_the_one_announced():
    assert len(R.MUTANTS) == 12 and len(set(R.MUTANTS)) == 12


def test_round_durations_known_values():
    """d = clamp(round_half_even(alpha * max(exp(x) - 1, 0)), min_frames, 2^31 - 1), 0 past text_len.
    exp(log(v + 1)) - 1 gives a small integer v back only to within an f32 ulp, which is enough to round
    to v but not to sit on a tie; the ties are therefore built from an x whose exp(x) - 1 is exactly 1
    and half-integer alphas, whose products are exact."""
    from tt2.regulate import round_durations
    v = torch.tensor([[0.0, 1.0, 2.0, 3.0, 5.0, 7.0, 10.0, 0.2]])
    x = torch.log(v + 1.0)
    assert torch.equal(torch.round(torch.exp(x) - 1.0), torch.round(v))           # the premise
    got = round_durations(x)
    assert got.dtype == torch.int32 and got.tolist() == [[0, 1, 2, 3, 5, 7, 10, 0]]
    # alpha scales before rounding: 2 v, then rounded
    assert round_durations(x, alpha=2.0).tolist() == [[0, 2, 4, 6, 10, 14, 20, 0]]
    # ties to even: an x whose exp(x) - 1 is exactly 1 in f32 (one of the neighbours of log 2), then
    # alpha = 0.5, 1.5, 2.5, 3.5 are exact products on the tie
    near = torch.tensor(np.float32(np.log(2.0))).repeat(17)
    for i in range(17):
        for _ in range(abs(i - 8)):
            near[i] = torch.nextafter(near[i], torch.tensor(float("inf") if i > 8 else float("-inf")))
    hit = near[(torch.exp(near) - 1.0) == 1.0]
    assert len(hit) > 0
    x1 = hit[:1].reshape(1, 1)
    assert [round_durations(x1, alpha=a).item() for a in (0.5, 1.5, 2.5, 3.5, 4.5)] == [0, 2, 2, 4, 4]
    # negative and tiny predictions are 0 frames; min_frames lifts them, but not past text_len
    x2 = torch.tensor([[-5.0, 0.0, 1e-3, 2.0], [3.0, -1.0, 0.7, 0.7]])
    assert round_durations(x2).tolist() == [[0, 0, 0, 6], [19, 0, 1, 1]]
    assert round_durations(x2, min_frames=1).tolist() == [[1, 1, 1, 6], [19, 1, 1, 1]]
    assert round_durations(x2, text_len=torch.tensor([3, 1]), min_frames=1).tolist() == [[1, 1, 1, 0], [19, 0, 0, 0]]
    assert round_durations(x2, text_len=torch.tensor([9, -2])).tolist() == [[0, 0, 0, 6], [0, 0, 0, 0]]
    # overflow, infinity and NaN
    x3 = torch.tensor([[30.0, float("inf"), float("nan"), float("-inf")]])
    assert round_durations(x3).tolist() == [[R.INT32_MAX, R.INT32_MAX, 0, 0]]
    assert round_durations(x3, min_frames=2).tolist() == [[R.INT32_MAX, R.INT32_MAX, 2, 2]]
    assert round_durations(x2.double()).tolist() == [[0, 0, 0, 6], [19, 0, 1, 1]]
    for bad in (dict(alpha=-1.0), dict(alpha=float("nan")), dict(min_frames=-1)):
        with pytest.raises(ValueError):
            round_durations(x2, **bad)
    with pytest.raises(ValueError):
        round_durations(torch.zeros(3))
    with pytest.raises(ValueError):
        round_durations(torch.zeros(2, 3, dtype=torch.int32))
