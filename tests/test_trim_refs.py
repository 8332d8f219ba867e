"""CPU: the float64 reference of tt2_trim (tests/_trim_refs.py) against a brute-force evaluation of
the definition, hand-computed answers of librosa's rule and a np.convolve formulation; the exactness
of the GPU test's integer problems; the judge against fifteen mutants on that problem set; and the
random problem's distance from the threshold."""
import numpy as np
import pytest

import _trim_refs as R


def test_reference_equals_the_brute_force_definition():
    rng = np.random.default_rng(0)
    for hop, r in [(1, 1), (2, 1), (4, 3), (5, 2), (16, 2), (3, 16)]:
        frame = 2 * r * hop
        for L in (0, 1, hop - 1, hop, hop + 1, r * hop - 1, r * hop + 1, 3 * frame + 1, 5 * frame + hop // 2):
            n_in = L + 3
            x = rng.normal(size=n_in) * (rng.random(n_in) < 0.6)
            x[:min(L, frame)] *= 1e-3
            for keep in (0, 1, hop + 1, 10 * n_in):
                for ratio in (1e-3, 0.25, 0.0, 1.0):
                    for n_out in (max(L - 2, 1), n_in + 2):
                        y, outs, starts, en = R.reference(x[None, :], [L], hop, r, keep, ratio, n_out)
                        by, bo, bs, be = R.brute(x, L, hop, r, keep, ratio, n_out)
                        assert (outs[0], starts[0]) == (bo, bs), (hop, r, L, keep, ratio)
                        assert np.array_equal(y[0], by)
                        F = R.n_frames(L, hop)
                        assert len(be) == F and np.allclose(en[0, :F], be, rtol=1e-13, atol=0)
                        assert not en[0, F:].any() and en.shape[1] == n_in // hop + 1
                        assert 0 <= starts[0] <= starts[0] + outs[0] <= L


def test_convolve_formulation_gives_the_same_energies():
    rng = np.random.default_rng(1)
    for hop, r in [(1, 1), (4, 3), (7, 2), (3, 16)]:
        for L in (1, hop, r * hop + 1, 6 * r * hop + 2):
            x = rng.integers(-3, 4, size=L).astype(np.float64)
            assert np.array_equal(R.by_convolve(x, L, hop, r), R.frame_energies(x, L, hop, r)), (hop, r, L)


def test_known_answers_of_librosas_rule():
    """librosa.effects.trim(y, top_db, frame_length, hop_length) keeps
    [frames_to_samples(first loud), min(len, frames_to_samples(last loud + 1))), loud meaning
    10 log10(mse / max mse) > -top_db on centred zero-padded frames.  By hand, frame 4, hop 2 (r = 1):
    x = 0 0 0 0 0 5 5 0 0 0 0 0, len 12: frames centred on 0, 2, .., 12 cover [-2, 2), [0, 4), ..
    energies 0 0 25 50 25 0 0; any top_db > 3.02 dB makes frames 2, 3, 4 loud: [4, 10)."""
    x = np.zeros((1, 12))
    x[0, 5:7] = 5
    y, outs, starts, en = R.reference(x, None, 2, 1, 0, 10 ** -6.0, 12)
    assert en[0].tolist() == [0, 0, 25, 50, 25, 0, 0] and (starts, outs) == ([4], [6])
    assert y[0].tolist() == [0, 5, 5, 0, 0, 0] + [0] * 6
    # at 3 dB only the frame centred between the two samples is loud: [6, 8), half of the burst --
    # the rule cuts at frame centres, not frame edges
    _, outs, starts, _ = R.reference(x, None, 2, 1, 0, 10 ** -0.3, 12)
    assert (starts, outs) == ([6], [2])
    # exactly on the threshold is silent: ratio 1/2 of 50 is 25
    _, outs, starts, _ = R.reference(x, None, 2, 1, 0, 0.5, 12)
    assert (starts, outs) == ([6], [2])
    # keep widens both ends and is clamped into the utterance
    _, outs, starts, _ = R.reference(x, None, 2, 1, 3, 10 ** -6.0, 12)
    assert (starts, outs) == ([1], [11])
    _, outs, starts, _ = R.reference(x, None, 2, 1, 100, 10 ** -6.0, 12)
    assert (starts, outs) == ([0], [12])
    # a burst at the very start and end, all zero, and a length that is not a multiple of the hop
    x = np.zeros((3, 11))
    x[0, 0] = 1
    x[1, 10] = 1
    y, outs, starts, en = R.reference(x, [11, 11, 11], 2, 1, 0, 10 ** -6.0, 11)
    assert en[0].tolist() == [1, 1, 0, 0, 0, 0] and en[1].tolist() == [0, 0, 0, 0, 0, 1]
    assert (starts, outs) == ([0, 10, 0], [4, 1, 0])
    # interior silence is kept
    x = np.zeros((1, 40))
    x[0, 8] = x[0, 30] = 1
    _, outs, starts, _ = R.reference(x, None, 2, 1, 0, 10 ** -6.0, 40)
    assert (starts, outs) == ([8], [26])       # frames 4 .. 5 and 15 .. 16: [8, 34)
    # lens clamps: above n_in, negative
    _, outs, starts, _ = R.reference(x, [47], 2, 1, 0, 10 ** -6.0, 40)
    assert (starts, outs) == ([8], [26])
    _, outs, starts, _ = R.reference(x, [-1], 2, 1, 0, 10 ** -6.0, 40)
    assert (starts, outs) == ([0], [0])
    # n_out clamps the length, not the start
    y, outs, starts, _ = R.reference(x, None, 2, 1, 0, 10 ** -6.0, 5)
    assert (starts, outs) == ([8], [5]) and y.shape == (1, 5)


@pytest.fixture(scope="module")
def problems():
    return R.exact_problems()


def test_the_exact_problems_are_exact_and_cover_the_cases(problems):
    assert sorted({(p["hop"], p["r"]) for p in problems}) == sorted(R.GEOMETRIES)
    seen_below = seen_above = seen_equal = False
    for p in problems:
        x, lens, hop, r = p["x"], p["lens"], p["hop"], p["r"]
        assert np.abs(x).max() <= 3 and np.array_equal(x, np.rint(x))
        assert R.exact(x, hop, r, p["ratio"], lens), (hop, r, p["ratio"])
        n_in = x.shape[1]
        assert hop == 1 or n_in % hop
        assert max(lens) > n_in and min(lens) < 0
        eff = {R.clamp_len(v, n_in) for v in lens}
        assert {0, 1, hop - 1, hop, hop + 1, r * hop - 1, r * hop + 1} <= eff
        _, outs, starts, en = R.reference(x, lens, hop, r, p["keep"], p["ratio"], n_in + 5)
        seen_below |= any(o > p["n_out"] for o in outs)
        seen_equal |= any(o == p["n_out"] for o in outs)
        seen_above |= all(o < p["n_out"] for o in outs)
        row = dict(zip(p["names"], range(len(lens))))
        assert outs[row["none"]] == 0 and starts[row["none"]] == 0
        if p["keep"] == 0:
            if p["ratio"] < 0.5:         # (at 1/2 the half-covered frame at either end is on the threshold)
                assert starts[row["at_0"]] == 0
                assert starts[row["at_end"]] + outs[row["at_end"]] == n_in
            if p["ratio"] == 0.5:
                b = row["single_frame"]
                e = en[b]
                assert (e > 0.5 * e.max()).sum() == 1 and (e == 0.5 * e.max()).sum() >= 2
            if p["ratio"] == 0.25:
                b = row["threshold"]
                e = en[b]
                assert (e == 0.25 * e.max()).sum() >= 1 and starts[b] > 2 * r * hop
            if p["ratio"] == 2.0 ** -3:
                assert outs[row["all"]] == n_in
            if p["ratio"] < 0.5:
                b = row["islands"]
                e = en[b, :R.n_frames(R.clamp_len(lens[b], n_in), hop)]
                loud = np.nonzero(e > p["ratio"] * e.max())[0]
                assert (np.diff(loud) > 1).any() and starts[b] > 0
    assert seen_below and seen_equal and seen_above
    assert not R.exact(np.array([[0.1, 0.2]]), 1, 1, 0.5) and not R.exact(np.full((1, 4), 3.0), 1, 1, 0.3)


def test_the_judge_accepts_the_reference_and_its_f32_image(problems):
    for p in problems[::5]:
        ref = R.reference(p["x"], p["lens"], p["hop"], p["r"], p["keep"], p["ratio"], p["n_out"])
        got = (ref[0].astype(np.float32), np.array(ref[1], dtype=np.int32), np.array(ref[2], dtype=np.int32),
               np.pad(ref[3].astype(np.float32), ((0, 0), (0, 3)), constant_values=np.nan))
        assert R.judge(got, ref) == []
        assert R.judge((got[0], got[1], got[2], None), ref) == []


@pytest.mark.parametrize("name", R.MUTANTS)
def test_the_judge_rejects_every_mutant(problems, name):
    """Each mistake shows on at least one problem of the set the GPU test runs."""
    rejected = 0
    for p in problems:
        args = (p["x"], p["lens"], p["hop"], p["r"], p["keep"], p["ratio"], p["n_out"])
        if R.judge(R.mutant(name, *args), R.reference(*args)):
            rejected += 1
    assert rejected > 0, name
    assert R.judge(R.mutant("none at all", *args), R.reference(*args)) == []      # the mutant harness itself


RANDOM = [(512, 2, 12 * 2048 + 300, 3), (64, 3, 12 * 384 + 77, 4)]


@pytest.mark.parametrize("hop,r,n_in,seed", RANDOM)
def test_the_random_problem_stays_clear_of_the_threshold(hop, r, n_in, seed):
    """At top_db = 30 under 40 dB steps every frame is further from the threshold than the f32 bound
    lets an energy and the threshold move together, so any evaluation within the bound must take the
    float64 decision, and the GPU test may require it for every utterance."""
    x, lens = R.random_problem(hop, r, n_in, seed)
    ratio = np.float32(10.0 ** -3.0)
    for b in range(4):
        assert R.decision_margin(x[b], lens[b], hop, r, ratio) > 0.5, b
    _, outs, starts, _ = R.reference(x, lens, hop, r, 0, ratio, n_in)
    assert all(o > 0 for o in outs) and starts[2] == 0 and starts[3] + outs[3] == lens[3]
    assert starts[0] > 0 and starts[1] > 0
