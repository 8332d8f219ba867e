"""CPU: the numpy references of tt2_pitch_track (tests/_pitch_track_refs.py) are what the GPU tests
trust, so they are checked first: against an exhaustive minimum over every state sequence, by
mutants that the exact problem must tell from the definition, for the exactness premise of that
problem, and on the two signals whose lags the kernel tests compare exactly."""
import numpy as np
import pytest

import _pitch_track_refs as R


def test_cost_equals_the_exhaustive_minimum():
    """(a) On dyadic inputs (every sum exact) the reference's cost, and the cost of its own path summed
    again, equal the minimum over all (S + 1)^N state sequences, S <= 3, N <= 5, 300 trials."""
    rng = np.random.default_rng(3)
    for trial in range(300):
        S, N = int(rng.integers(1, 4)), int(rng.integers(1, 6))
        tau_min = int(rng.integers(1, 6))
        tau_max = tau_min + S - 1
        c = rng.integers(0, 9, (N, tau_max + 1)) / 8.0
        pos = np.cumsum(rng.integers(0, 3, tau_max + 1)).astype(np.float64)
        J, W, C = (float(v) / 4 for v in rng.integers(0, 5, 3))
        for dtype in (np.float64, np.float32):
            r = R.track(c, tau_min, tau_max, pos, J, W, C, dtype=dtype)
            want = R.brute_force(c, tau_min, tau_max, pos, J, W, C)
            assert float(r["cost"]) == want, (trial, r["cost"], want)
            assert float(R.path_cost(r["states"], c, tau_min, tau_max, pos, J, W, C)) == want, trial
            assert np.array_equal(R.states_of(r["lag"], tau_min), r["states"])


def _exact_results(**kw):
    pos = R.exact_pos()
    out = []
    for lo, hi, J, W, C in R.exact_cases():
        c = R.exact_cmnd(lo, hi, poison=False)
        for b, n in enumerate(R.EXACT_FRAMES):
            out.append(R.track(c[b, :n], lo, hi, pos, J, W, C, dtype=np.float32, **kw))
    return out


def _same(a, b):
    return all(np.array_equal(x["lag"], y["lag"]) and np.array_equal(R.bits(x["f0"]), R.bits(y["f0"]))
               and R.bits(x["cost"]) == R.bits(y["cost"]) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def exact_definition():
    return _exact_results()


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_exact_problem_tells_every_mutant_from_the_definition(mutant, exact_definition):
    """(b) Each single mistake changes a lag, an f0 bit or a cost bit somewhere in the exact problem."""
    assert not _same(exact_definition, _exact_results(**{mutant: True})), mutant


def test_exact_problem_is_exact_and_twin_equals_float64(exact_definition):
    """(c) Every value the exact problem forms is an integer multiple of 2^-3 below 2^21, so every f32
    operation of the recurrence is exact in any order and with or without an fma; the twin and the
    float64 definition then agree on every lag and every cost.  The problem is not degenerate:
    voiced and unvoiced frames, switches both ways, refined and unrefined f0."""
    pos = R.exact_pos()
    assert np.all(np.diff(pos) > 0) and np.all(pos == np.rint(pos))
    it = iter(exact_definition)
    kinds = set()
    for lo, hi, J, W, C in R.exact_cases():
        assert all(v * 4 == int(v * 4) for v in (J, W, C))
        c = R.exact_cmnd(lo, hi, poison=False)
        assert np.all(c * 8 == np.rint(c * 8)) and c.min() == 0 and c.max() == 1
        p = R.exact_cmnd(lo, hi)
        assert np.isnan(p[:, :, :lo]).all() and np.isnan(p[:, :, hi + 1:]).all() and np.isnan(p[1, 4:]).all()
        assert np.array_equal(p[0, :, lo:hi + 1], c[0, :, lo:hi + 1]) and p.shape[2] > hi + 1
        for b, n in enumerate(R.EXACT_FRAMES):
            rec = []
            r64 = R.track(c[b, :n], lo, hi, pos, J, W, C, dtype=np.float64, record=rec)
            for v in rec:
                assert np.all(v * 8 == np.rint(v * 8)) and np.all(np.abs(v) < 2 ** 21)
            r32 = next(it)
            assert np.array_equal(r32["lag"], r64["lag"]) and float(r32["cost"]) == float(r64["cost"])
            lag = r32["lag"]
            kinds |= {"voiced"} if (lag > 0).any() else set()
            kinds |= {"unvoiced"} if (lag == 0).any() else set()
            kinds |= {"on"} if ((lag[1:] > 0) & (lag[:-1] == 0)).any() else set()
            kinds |= {"off"} if ((lag[1:] == 0) & (lag[:-1] > 0)).any() else set()
            kinds |= {"jump"} if ((lag[1:] > 0) & (lag[:-1] > 0) & (lag[1:] != lag[:-1])).any() else set()
            kinds |= {"refined"} if r32["refined"].any() else set()
            kinds |= {"unrefined inside"} if ((lag > lo) & (lag < hi) & ~r32["refined"]).any() else set()
    assert kinds == {"voiced", "unvoiced", "on", "off", "jump", "refined", "unrefined inside"}, kinds


def test_planted_track_twin_and_float64_agree():
    """The planted-track problem of the kernel test: the twin and the float64 reference find the
    planted lags, and agree on every lag (so the kernel's lags can be compared exactly)."""
    c, lag = R.planted()
    lo, hi = R.PLANT_RANGE
    r64 = R.track(c, lo, hi, R.log2_pos(), *R.DEFAULTS, dtype=np.float64)
    r32 = R.track(c, lo, hi, R.log2_pos(), *R.DEFAULTS, dtype=np.float32)
    assert np.array_equal(r32["lag"], r64["lag"])
    assert np.array_equal(r64["lag"], lag)


def test_glide():
    """(d) On the glide the tracker with the defaults follows the true lag through the frames whose
    odd harmonics fade and reports the noise tail unvoiced; the per-frame selection at threshold
    0.1 reports an octave up in at least 5 of the frames 20 .. 27."""
    c, truth = R.glide_cmnd()
    lo, hi = R.GLIDE_RANGE
    for dtype in (np.float32, np.float64):
        r = R.track(c, lo, hi, R.log2_pos(), *R.DEFAULTS, dtype=dtype)
        assert R.glide_tracked_ok(r["lag"], truth) == [], (r["lag"], np.rint(truth))
    sel = R.select_lags(c, lo, hi)
    assert R.glide_octave_errors(sel, truth) >= 5, (sel[20:28], truth[20:28])
    assert R.glide_tracked_ok(sel, truth) != []
