"""CPU: the numpy references of tests/_yin_refs.py are themselves right (they find the pitch of
tones and call noise unvoiced), the integer problems of the GPU test are exact in f32 and reach
every branch of the search, and each of a list of deliberate mistakes changes some output of
those problems (so a kernel with that mistake fails tests/test_gpu_yin_kernels.py).

Measured here: tones 70..600 Hz within 0.51 cent; 0 of 200 noise frames voiced, their lowest d'
0.80; largest d * tau 5.0e6 and largest S 2.6e6 over the integer frames (2^24 = 1.68e7)."""
import numpy as np
import pytest

import _yin_refs as R

TONE_RANGE = (36, 340)


def tone(f, phase, n=R.FRAME):
    t = np.arange(n) / R.SR
    return np.sin(2 * np.pi * f * t + phase) + 0.5 * np.sin(2 * np.pi * 2 * f * t + 1.7 * phase + 0.4)


def test_tones_within_one_cent():
    worst = 0.0
    for f in (70.0, 82.4, 100.0, 131.7, 180.0, 220.0, 261.6, 330.0, 415.3, 523.25, 600.0):
        for phase in (0.0, 1.1, 2.9):
            r = R.yin_frame(tone(f, phase), *TONE_RANGE, 0.1)
            assert r["voiced"], (f, phase)
            cents = abs(1200 * np.log2(float(r["f0"]) / f))
            worst = max(worst, cents)
            assert cents < 1.0, (f, phase, float(r["f0"]), cents)
    print(f"worst tone error {worst:.3f} cent")


def test_noise_is_unvoiced():
    rng = np.random.default_rng(7)
    voiced, low = 0, np.inf
    for _ in range(200):
        r = R.yin_frame(rng.normal(size=R.FRAME), *TONE_RANGE, 0.1)
        voiced += bool(r["voiced"])
        low = min(low, float(r["cmnd"][TONE_RANGE[0]:TONE_RANGE[1] + 1].min()))
        assert r["f0"] == 0 or r["voiced"]
    print(f"voiced {voiced} of 200, lowest d' {low:.3f}")
    assert voiced == 0
    assert low > 0.5


def test_f32_twin_follows_the_float64_reference_on_real_frames():
    rng = np.random.default_rng(3)
    y = (tone(150.0, 0.5) + 0.05 * rng.normal(size=R.FRAME)).astype(np.float32)
    a, b = R.yin_frame(y, *TONE_RANGE, 0.1), R.yin_frame(y, *TONE_RANGE, 0.1, dtype=np.float32)
    assert b["cmnd"].dtype == np.float32 and b["aper"].dtype == np.float32 and b["energy"].dtype == np.float32
    assert np.allclose(a["cmnd"], b["cmnd"], rtol=1e-4)
    assert a["lag"] == b["lag"] and abs(float(a["f0"]) - float(b["f0"])) < 1e-2
    assert abs(float(a["energy"]) - float(b["energy"])) < 1e-6


def all_exact_frames():
    out = list(R.exact_frames())
    out += [(b, f, y) for b, f, y in R.exact_frames(hop=1)]
    out += [(b, f, y) for b, f, y in R.exact_frames(hop=300, t=7, frames=(7, 7, 7))]
    return out


def test_integer_problems_are_exact_in_f32():
    """Samples in -3..3: d <= 36 * 512, and every d * tau and every S below 2^24, so each is an
    integer that f32 holds exactly whatever the order of the sums; the f32 twin then equals the
    float64 reference in d, S and the numerator, and its divide defines d' to the bit."""
    top_num = top_s = 0.0
    for _, _, y in all_exact_frames():
        assert np.abs(y).max() <= 3 and np.array_equal(y, np.rint(y))
        r64, r32 = R.yin_frame(y, 1, 511, 0.1), R.yin_frame(y, 1, 511, 0.1, dtype=np.float32)
        top_num = max(top_num, float((r64["d"] * np.arange(R.MAX_LAG + 1)).max()))
        top_s = max(top_s, float(r64["S"].max()))
        assert np.array_equal(r64["d"], r32["d"].astype(np.float64))
        assert np.array_equal(r64["S"], r32["S"].astype(np.float64))
        assert np.array_equal(r64["cmnd"].astype(np.float32), r32["cmnd"])   # one rounding of the same quotient
        assert r64["energy"].astype(np.float32) == r32["energy"]
    print(f"max d * tau {top_num:.0f}, max S {top_s:.0f}")
    assert top_num < 2 ** 24 and top_s < 2 ** 24


def twin_results(cmnd_kw=None, select_kw=None):
    """Every (frame, parameter set) of the exact problem through the f32 twin."""
    out = []
    for b, f, y in R.exact_frames():
        for tmin, tmax, thr in R.EXACT_PARAMS:
            out.append(((b, f, tmin, tmax, thr),
                        R.yin_frame(y, tmin, tmax, thr, dtype=np.float32, cmnd_kw=cmnd_kw, select_kw=select_kw)))
    return out


@pytest.fixture(scope="module")
def truth():
    return twin_results()


def test_integer_frames_reach_every_branch(truth):
    seen = set()
    for (b, f, tmin, tmax, thr), r in truth:
        seg = r["cmnd"][tmin:tmax + 1]
        if r["voiced"]:
            if r["steps"] >= 2:
                seen.add("walk")
            if r["steps"] >= 2 and r["refined"]:
                seen.add("walk then refine")
            if r["lag"] == tmin and tmin < tmax:
                seen.add("dip at tau_min")
            if r["lag"] == tmax and tmin < tmax:
                seen.add("dip at tau_max")
            if tmin == tmax:
                seen.add("one-lag range, voiced")
            if r["aper"] == 0:
                seen.add("exact period")
            if r["refined"] and r["steps"] == 0:
                seen.add("refined without a walk")
        else:
            if np.count_nonzero(seg == seg.min()) > 1 and np.any(y_nonzero(b, f)):
                seen.add("no dip, tied minimum")
            if not np.any(y_nonzero(b, f)):
                seen.add("all-zero frame")
            if tmin == tmax:
                seen.add("one-lag range, unvoiced")
    want = {"walk", "walk then refine", "dip at tau_min", "dip at tau_max", "one-lag range, voiced", "exact period",
            "refined without a walk", "no dip, tied minimum", "all-zero frame", "one-lag range, unvoiced"}
    assert seen == want, want - seen
    # the perturbed period-50 tile: a shallow dip, as a voiced speech frame has
    r = dict(truth)[(0, 0, 36, 340, 0.1)]
    assert r["lag"] == 50 and 0 < r["aper"] < 0.02, (r["lag"], r["aper"])


def y_nonzero(b, f):
    return R.exact_signal(poison=False)[b, f * R.HOP:f * R.HOP + R.FRAME] != 0


def differs(r, m):
    same = (r["lag"] == m["lag"] and r["voiced"] == m["voiced"] and
            np.array_equal(np.float32(r["aper"]).view(np.int32), np.float32(m["aper"]).view(np.int32)) and
            np.float32(r["f0"]) == np.float32(m["f0"]) and
            np.array_equal(r["cmnd"].view(np.int32), m["cmnd"].view(np.int32)))
    return not same


MUTANTS = {
    "tau factor dropped": dict(cmnd_kw=dict(tau_factor=False)),
    "<= in the threshold compare": dict(select_kw=dict(thr_le=True)),
    "<= in the walk": dict(select_kw=dict(walk_le=True)),
    "walk omitted": dict(select_kw=dict(no_walk=True)),
    "W = 511": dict(cmnd_kw=dict(W=511)),
    "W = 513": dict(cmnd_kw=dict(W=513)),
    "prefix from tau = 0 with d(0) = 1": dict(cmnd_kw=dict(prefix_from_zero=True)),
    "highest index on a tie": dict(select_kw=dict(tie_high=True)),
    "refinement at an edge": dict(select_kw=dict(refine_edge=True)),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_each_mutant_is_caught_by_some_integer_frame(truth, name):
    mut = twin_results(**MUTANTS[name])
    caught = [k for (k, r), (_, m) in zip(truth, mut) if differs(r, m)]
    print(f"{name}: caught by {len(caught)} of {len(truth)} (frame, parameters) cases, first {caught[:1]}")
    assert caught, name
