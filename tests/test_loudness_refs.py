"""CPU: the float64 references of tests/_loudness_refs.py are held against each other, against the
standard's numbers and against hand-computed gate cases before the GPU files rely on them; the
chunked model of the kernel's scheme is bit-equal to the unchunked reference on the integer
problems at every chunking; every mutant is told apart by a problem that the GPU file runs."""
import numpy as np
import pytest

import _loudness_refs as R

PROBLEMS = R.exact_problems()
SMALL = [p for p in PROBLEMS if p["x"].shape[1] <= 2 * R.KERNEL_SEG + 40]


def run(p, **kw):
    return R.reference(**{k: v for k, v in p.items() if k != "name"}, **kw)


def test_design_reproduces_the_standards_table_at_48k():
    (b1, a1), (b2, a2) = R.kweighting(48000)
    assert np.abs(b1 - [1.53512485958697, -2.69169618940638, 1.19839281085285]).max() < 1e-12
    assert np.abs(a1 - [1.0, -1.69065929318241, 0.73248077421585]).max() < 1e-12
    assert np.abs(b2 - [1.0, -2.0, 1.0]).max() == 0
    assert np.abs(a2 - [1.0, -1.99004745483398, 0.99007225036621]).max() < 1e-12


def test_design_at_22050_and_the_package_agrees():
    (b1, a1), (b2, a2) = R.kweighting(22050)
    assert np.abs(b1 - [1.479825350977746, -2.170728612856829, 0.860842484726552]).max() < 1e-12
    assert np.abs(a1[1:] - [-1.338305336066134, 0.508244558913602]).max() < 1e-12
    assert np.abs(a2[1:] - [-1.978397602590119, 0.978514419503251]).max() < 1e-12
    from tt2 import audio
    for sr in (22050, 48000, 16000, 44100):
        got = audio.kweighting(sr)
        assert np.abs(np.array(R.coef10(got)) - np.array(R.coef10(R.kweighting(sr)))).max() < 1e-15
        assert all(isinstance(v, float) for sec in got for ba in sec for v in ba)


@pytest.mark.parametrize("sr,want", [(48000, -3.0103), (22050, -2.9810)])
def test_known_answer_997_hz_sine(sr, want):
    n = 5 * sr
    x = np.sin(2 * np.pi * 997.0 * np.arange(n) / sr).astype(np.float32)[None]
    p = R.default_params(sr)
    res = R.reference(x, None, n_out=0, **p)
    assert abs(float(res["loud"][0]) - want) < 1e-3
    if sr == 48000:
        assert abs(float(res["loud"][0]) + 3.01) < 0.01


def test_scaling_law():
    x, lens = R.random_problem()
    p = R.default_params()
    a = R.reference(x, lens, n_out=0, **p)
    b = R.reference(2.0 * x, lens, n_out=0, **p)
    for ma, mb in zip(a["ms"], b["ms"]):
        assert abs(10 * np.log10(mb) - 10 * np.log10(ma) - 20 * np.log10(2.0)) < 1e-9


def test_reference_against_brute_force():
    x, lens = R.random_problem(seconds=0.6)
    p = R.default_params()
    a = R.reference(x[:2], lens[:2], n_out=50, **p)
    b = R.reference(x[:2], lens[:2], n_out=50, filt=R.filter_brute, **p)
    for sa, sb in zip(a["sub"], b["sub"]):
        assert np.abs(sa / sb - 1).max() < 1e-9
    assert R.same(a, b, keys=("y", "gain", "peak", "limited")) == [] and np.abs(a["loud"] - b["loud"]).max() < 1e-5
    for p in SMALL[:6]:
        assert R.same(run(p), run(p, filt=R.filter_brute)) == [], p["name"]


def test_hand_computed_threshold_cases():
    """_loudness_refs.threshold_problems: a block exactly on a threshold fails."""
    on_rel, on_abs = R.threshold_problems()
    for p in (on_rel, on_abs):
        res = run(p)
        E, pa, both = res["gates"][0]
        assert E.tolist() == [64, 64, 64, 64, 48, 32, 16, 0, 4, 8, 8, 8, 4, 0]
        assert both.tolist() == [True] * 7 + [False] * 2 + [True] * 3 + [False] * 2
        assert res["ms"][0] == 37.6 / 4 and res["peak"][0] == 4
        assert res["loud"][0] == np.float32(-0.691 + 10 * np.log10(9.4))
        # gain: sqrt(2^-4 / 9.4) = 0.0815.. against 0.5 / 4: the target wins
        assert res["gain"][0] == np.float32(np.sqrt(0.0625 / 9.4)) and res["limited"][0] == 0
    assert int(run(on_rel)["gates"][0][1].sum()) == 12 and int(run(on_abs)["gates"][0][1].sum()) == 10


def test_hand_computed_gate_cases():
    p = R.default_params()
    sr, step = 22050, p["step"]
    rng = np.random.default_rng(3)
    tone = rng.normal(size=4 * sr)
    # a half 20 dB down: the relative gate drops it, and the loudness is that of the blocks that reach into the loud half
    x = (0.1 * tone).astype(np.float32)
    y = x.copy()
    y[2 * sr:] *= np.float32(0.1)
    whole, half = R.reference(y[None], None, n_out=0, **p), R.reference(x[None, :2 * sr], None, n_out=0, **p)
    E, pa, both = whole["gates"][0]
    assert pa.all() and both[:17].all() and not both[20:].any()
    # (the three blocks that straddle the step pass both gates at part of the level: 17 + 1.65 of 20)
    assert -0.5 < float(whole["loud"][0]) - float(half["loud"][0]) < -0.2
    assert abs(whole["ms"][0] - E[:20].mean() / (4 * step)) < 1e-15
    # a tail near -80 LKFS: dropped by the absolute gate
    z = x.copy()
    z[2 * sr:] *= np.float32(10 ** (-58 / 20))
    tail = R.reference(z[None], None, n_out=0, **p)
    loud_tail = R.reference(z[None, 2 * sr + step:], None, n_out=0, abs_sum=0.0,
                            **{k: v for k, v in p.items() if k != "abs_sum"})["loud"][0]
    assert -85 < loud_tail < -75
    # (block 20 still holds the filter's ringing from the loud part, 53 dB above the tail)
    assert not tail["gates"][0][1][21:].any() and tail["gates"][0][1][:20].all()
    # silence and anything below four steps are unmeasured: -inf, gain 1, samples unchanged
    for v, L in ((np.zeros(sr, dtype=np.float32), sr), (x, 4 * step - 1), (x, 0)):
        r = R.reference(v[None], [L], n_out=len(v), **p)
        assert r["ms"][0] is None and r["loud"][0] == -np.inf and r["gain"][0] == 1 and r["limited"][0] == 0
        assert np.array_equal(R.bits(r["y"][0, :L]), R.bits(v[:L])) and not r["y"][0, L:].any()
    assert R.reference(x[None], [4 * step], n_out=0, **p)["ms"][0] is not None


def test_integer_problems_are_exact_and_cover_the_geometry():
    assert len(PROBLEMS) >= 14 and {p["step"] for p in PROBLEMS} == set(R.STEPS)
    for p in PROBLEMS:
        assert R.exact(p), p["name"]
    for step in R.STEPS:
        lens = {R.clamp_len(v, p["x"].shape[1]) for p in PROBLEMS if p["step"] == step for v in p["lens"]}
        raw = {v for p in PROBLEMS if p["step"] == step for v in p["lens"]}
        assert {4 * step - 1, 4 * step, 4 * step + 1, 0} <= lens and min(raw) < 0 and max(raw) == 10 ** 6
        if step != 2205:
            for seam in (R.KERNEL_CHUNK, R.KERNEL_SEG, 2 * R.KERNEL_SEG):
                assert {seam - 1, seam + 1} <= lens, (step, seam)
    res = [run(p) for p in PROBLEMS]
    lim = [int(v) for r in res for v in r["limited"]]
    assert 0 in lim and 1 in lim
    assert any(m is None for r in res for m in r["ms"]) and any(m is not None for r in res for m in r["ms"])
    # gated blocks of both kinds occur
    assert any((~pa).any() and pa.any() for r in res for _, pa, _ in r["gates"])
    assert any((pa & ~both).any() for r in res for _, pa, both in r["gates"])


@pytest.mark.parametrize("chunk,lanes", [(1, 64), (7, 4), (32, 64), (64, 2), (2048, 2), (16, 64)])
def test_chunked_model_is_bit_equal_on_the_integer_problems(chunk, lanes):
    for p in SMALL:
        if chunk == 1 and p["x"].shape[1] > 1200 and p["step"] != 1:
            continue                                   # one step is enough for the slowest chunking
        assert R.exact(p, chunk, lanes), p["name"]
        a = run(p)
        b = run(p, filt=lambda v, c: R.chunked_filter(v, c, chunk, lanes))
        assert R.same(a, b) == [], p["name"]
        for sa, sb in zip(a["sub"], b["sub"]):
            assert np.array_equal(sa, sb)


def test_chunked_model_on_the_default_coefficients():
    """At the K-weighting's pole radius the float64 scheme stays within 1e-8 of lfilter (the f32 one
    does not: DESIGN 5.12)."""
    x, lens = R.random_problem()
    p = R.default_params()
    a = R.reference(x, lens, n_out=0, **p)
    b = R.reference(x, lens, n_out=0, filt=R.chunked_filter, **p)
    for sa, sb in zip(a["sub"], b["sub"]):
        assert np.abs(sb / sa - 1).max() < 1e-8


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_rejected_by_an_exact_problem(mutant):
    assert len(R.MUTANTS) >= 12
    with np.errstate(all="ignore"):            # (swapped a1 / a2 make an unstable filter: its output overflows)
        caught = [p["name"] for p in PROBLEMS
                  if p["x"].shape[1] <= 3 * R.KERNEL_SEG + 43 and R.same(run(p, mutant=mutant), run(p))]
    assert caught, mutant


def test_random_problem_is_clear_of_both_thresholds():
    x, lens = R.random_problem()
    p = R.default_params()
    res = R.reference(x, lens, n_out=x.shape[1], **p)
    da, dr = R.threshold_distance(res, p["abs_sum"], p["rel_ratio"])
    print(f"nearest block: {da:.3e} of the absolute, {dr:.3e} of the relative threshold")
    assert da > 1e-6 and dr > 1e-6
    for (E, pa, both) in res["gates"]:
        assert len(E) >= 10
    assert res["limited"].tolist() == [0, 0, 0, 1]
    assert (~res["gates"][1][2] & res["gates"][1][1]).any()           # dropped by the relative gate
    assert (~res["gates"][2][1]).any() and res["gates"][2][1].any()   # dropped by the absolute gate
    assert all(m is not None for m in res["ms"])
