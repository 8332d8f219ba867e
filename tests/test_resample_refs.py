"""CPU: the float64 reference of the resampler (tests/_resample_refs.py) against the textbook
construction, the properties of the default bank, the exactness of the integer problems the GPU
test runs, and seven mutants of the definition that each fail a problem with a known answer.

Bars of the bank properties: 2 x the figure the float64 reference itself gives for that rate pair
(MEASURED below, recorded in DESIGN 5.10); they hold the design (cutoff, window, phase), not the
kernel.  The tone figures are over the interior outputs, those whose 2 * half + 1 samples all lie
inside the signal."""
import numpy as np
import pytest

import _resample_refs as R

ALL_PAIRS = R.PAIRS + R.MORE_PAIRS
ids = lambda p: f"{p[0]}-{p[1]}"  # noqa: E731

# (up, down, K) and what the reference gave: DC error, unit tone at 1 kHz, at 0.726 of the lower
# Nyquist, and (where it fits below the input Nyquist) the residue of a tone at 1.15 of the new Nyquist
MEASURED = {
    (48000, 22050): ((147, 320, 119), 2.560e-06, 2.973e-07, 3.990e-06, 5.083e-06),
    (44100, 22050): ((1, 2, 109), 2.422e-06, 2.507e-07, 3.820e-06, 5.139e-06),
    (24000, 22050): ((147, 160, 61), 3.266e-06, 6.838e-07, 4.971e-06, None),
    (16000, 22050): ((441, 320, 55), 3.849e-06, 1.451e-06, 5.138e-06, None),
    (22050, 16000): ((320, 441, 75), 2.803e-06, 1.009e-06, 4.520e-06, 5.225e-06),
    (96000, 22050): ((147, 640, 235), 2.384e-06, 2.554e-07, 3.924e-06, 4.925e-06),
}
N_TONE = 6000


def interior(n_in, up, down, half):
    n = np.arange(R.out_len(n_in, up, down))
    i0 = n * down // up
    return n[(i0 > half) & (i0 < n_in - 1 - half)]


def tone_error(pair, f, reject=False):
    up, down, half, taps = R.design(*pair)
    x = R.tones([f], [1.0], [0.3], pair[0], N_TONE)
    idx = interior(N_TONE, up, down, half)
    assert len(idx) > 500
    y = R.resample(x, N_TONE, taps, up, down, half, idx)
    want = 0.0 if reject else np.sin(2 * np.pi * f * idx / pair[1] + 0.3)
    return float(np.abs(y - want).max())


@pytest.mark.parametrize("pair", ALL_PAIRS, ids=ids)
def test_polyphase_equals_zero_stuff_convolve_decimate(pair):
    up, down, half, taps = R.design(*pair)
    x = np.random.default_rng(7).normal(size=700)
    got = R.resample(x, len(x), taps, up, down, half)
    want = R.zero_stuff(x, up, down, half, R.cutoff(up, down, 0.9), 24, 10.0)
    assert got.shape == want.shape == (R.out_len(700, up, down),)
    err = float(np.abs(got - want).max())
    print(f"{pair}: polyphase against zero-stuffing {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("pair", R.PAIRS, ids=ids)
def test_default_bank_properties(pair):
    (up, down, K), dc0, lo0, hi0, rej0 = MEASURED[pair]
    u, d, half, taps = R.design(*pair)
    assert (u, d, 2 * half + 1) == (up, down, K) and taps.shape == (up, K) and taps.dtype == np.float64
    assert K == 235 if pair[0] == 96000 else 55 <= K <= 119
    # row r's time axis: k - f_r, so the largest tap of a row is at k = 0 or k = 1
    assert set(np.argmax(taps, axis=1) - half) <= {0, 1}
    dc = float(np.abs(taps.sum(axis=1) - 1.0).max())
    lo = tone_error(pair, 1000.0)
    hi = tone_error(pair, 0.726 * min(pair) / 2)
    print(f"{pair}: dc {dc:.3e}, 1 kHz {lo:.3e}, 0.726 Nyquist {hi:.3e}")
    assert dc <= 2 * dc0 and lo <= 2 * lo0 and hi <= 2 * hi0
    assert dc <= 2 * 3.849e-6 and lo <= 2 * 1.451e-6 and hi <= 2 * 5.138e-6    # the worst pair's bars
    if rej0 is not None:
        f = 1.15 * pair[1] / 2
        assert f < pair[0] / 2
        rej = tone_error(pair, f, reject=True)
        print(f"{pair}: tone at 1.15 of the new Nyquist leaves {rej:.3e} ({20 * np.log10(rej):.1f} dB)")
        assert rej <= 2 * rej0 <= 2 * 5.225e-6
    else:
        assert 1.15 * pair[1] / 2 >= pair[0] / 2   # no such tone exists below the input Nyquist


def test_hann_6_zeros_is_why_the_defaults_differ():
    """The window / width / rolloff torchaudio defaults to (Hann, 6 zeros, 0.99), on the same
    prototype: 5.6e-2 at 0.8 of the new Nyquist, where the default bank, already rolling off, is at
    1.5e-3."""
    up, down = R.ratio(48000, 22050)
    c, zeros = 0.99 * up / down, 6
    half = int(np.ceil(zeros / c))
    r = np.arange(up)
    t = np.arange(-half, half + 1)[None, :] - (((r * down) % up) / up)[:, None]
    uu = c * t / zeros
    taps = c * np.sinc(c * t) * np.where(np.abs(uu) < 1, 0.5 + 0.5 * np.cos(np.pi * uu), 0.0)
    f = 0.8 * 11025
    x = R.tones([f], [1.0], [0.3], 48000, N_TONE)
    idx = interior(N_TONE, up, down, half)
    err = np.abs(R.resample(x, N_TONE, taps, up, down, half, idx) - np.sin(2 * np.pi * f * idx / 22050 + 0.3)).max()
    ours = tone_error((48000, 22050), f)      # 0.8 is past the default bank's flat part (0.726), in its roll-off
    print(f"tone at 0.8 of the new Nyquist: Hann / 6 zeros / 0.99 {err:.2e}, the default bank {ours:.2e}")
    assert 4e-2 < err < 8e-2 and ours < 2e-3 and err > 30 * ours


def test_library_bank_is_the_reference_bank():
    """tt2.audio.resample_bank (torch, host) against this file's numpy design: the same float64
    bank up to the two I0 implementations."""
    from tt2 import audio
    for pair in ALL_PAIRS:
        up, down, half, taps = R.design(*pair)
        b = audio.resample_bank(*pair)
        assert (b.up, b.down, b.half) == (up, down, half)
        assert b.taps.dtype.is_floating_point and b.taps.element_size() == 8 and tuple(b.taps.shape) == taps.shape
        assert b.taps.device.type == "cpu"
        assert np.abs(b.taps.numpy() - taps).max() <= 1e-14
    up, down, half, taps = R.design(48000, 22050, zeros=8, rolloff=1.0, beta=5.0)
    b = audio.resample_bank(48000, 22050, zeros=8, rolloff=1.0, beta=5.0)
    assert b.half == half and np.abs(b.taps.numpy() - taps).max() <= 1e-14


def test_bank_argument_checks():
    from tt2 import audio
    for bad in (dict(sr_in=0), dict(sr_out=-1), dict(zeros=0), dict(rolloff=0.0), dict(rolloff=1.01),
                dict(beta=-1.0), dict(beta=float("inf")), dict(beta=float("nan"))):
        kw = dict(sr_in=48000, sr_out=22050)
        kw.update(bad)
        with pytest.raises(ValueError):
            audio.resample_bank(**kw)
    with pytest.raises(ValueError, match="TT2_RESAMPLE_MAX_PHASES"):
        audio.resample_bank(22050, 22051)
    with pytest.raises(ValueError, match="TT2_RESAMPLE_MAX_TAPS"):
        audio.resample_bank(192000, 22050)
    assert audio.resample_bank(48000, 22050, rolloff=1.0).half == 53
    ident = audio.resample_bank(22050, 22050)
    assert (ident.up, ident.down) == (1, 1)


# ---------------------------------------------------------------- the integer problems
def exact_problem(up, down, half, n_in, seed=0, selector=False):
    bank = R.int_bank(up, half, seed, selector)
    x = R.int_signal(3, n_in, seed + 1)
    return bank, x, R.ragged_lens(3, n_in, seed + 2)


@pytest.mark.parametrize("up,down,half", R.EXACT_TRIPLES, ids=[f"{a}-{b}-{c}" for a, b, c in R.EXACT_TRIPLES])
def test_integer_problems_are_exact_in_f32(up, down, half):
    for n_in in R.exact_n_ins(half):
        for selector in (False, True):
            bank, x, lens = exact_problem(up, down, half, n_in, selector=selector)
            assert np.abs(bank).max() <= 8 and np.abs(x).max() <= 64 and R.is_exact(bank, x)
            assert lens[0] == n_in and lens[1] == 0
            if selector:
                assert (bank.sum(axis=1) == 1).all() and (np.abs(bank).sum(axis=1) == 1).all()
                assert up < 3 or len(set(np.argmax(bank, axis=1))) > 1      # row-dependent tap
            y = R.resample(x[0], n_in, bank, up, down, half)
            assert (y == np.rint(y)).all() and np.abs(y).max() < 2 ** 24
            # the same sum in f32 in two orders: the bits the kernel must give
            r, X = R.gather(x[0], n_in, up, down, half, np.arange(len(y)))
            P = bank[r].astype(np.float32) * X.astype(np.float32)
            fwd = np.zeros(len(y), dtype=np.float32)
            for k in range(P.shape[1]):
                fwd = fwd + P[:, k]
            assert np.array_equal(R.bits(fwd + np.float32(0)), R.bits(y))
            assert np.array_equal(R.bits(P[:, ::-1].sum(axis=1, dtype=np.float32) + np.float32(0)), R.bits(y))
    assert not R.is_exact(np.full((1, 3), 0.5), np.ones(4)) and not R.is_exact(np.full((1, 3), 2.0 ** 12), np.full(4, 2.0 ** 11))


def impulse_answer(pair, m, n, zeros=24, rolloff=0.9, beta=10.0):
    """What an impulse at input sample m gives at output n: h(n * down / up - m), by scalar
    arithmetic and a power series for I0, independently of the vectorised design."""
    up, down = R.ratio(*pair)
    c = rolloff * min(1.0, up / down)
    t = n * down / up - m

    def i0(z):
        s, term, j = 1.0, 1.0, 1
        while term > 1e-18 * s:
            term *= (z / (2 * j)) ** 2
            s += term
            j += 1
        return s

    uu = c * t / zeros
    if abs(uu) >= 1:
        return 0.0
    sinc = 1.0 if t == 0 else np.sin(np.pi * c * t) / (np.pi * c * t)
    return c * sinc * i0(beta * np.sqrt(1 - uu * uu)) / i0(beta)


def design_problem_error(pair, mutant):
    up, down, half, taps = R.design(*pair, mutant=mutant)
    n_in, worst = 400, 0.0
    for m in (200, 201, 202):       # three positions: when down > up no single one meets every tap
        x = np.zeros(n_in)
        x[m] = 1.0
        y = R.resample(x, n_in, taps, up, down, half)
        want = np.array([impulse_answer(pair, m, n) for n in range(len(y))])
        worst = max(worst, float(np.abs(y - want).max()))
    return worst


def index_problem_differs(triple, mutant):
    up, down, half = triple
    bank, x, _ = exact_problem(up, down, half, 1001, seed=5)     # 1001 * up / down is no integer
    good = R.resample(x[0], 1001, bank, up, down, half)
    bad = R.resample(x[0], 1001, bank, up, down, half, mutant=mutant)
    return good.shape != bad.shape or not np.array_equal(good, bad)


def test_the_definition_passes_the_impulse_problem():
    for pair in ((48000, 22050), (16000, 22050), (22050, 16000)):
        # two implementations of I0 (a power series here, numpy's Chebyshev fit there), each good to
        # a few tens of ulp of values up to I0(10) = 2816, and a sine of an argument up to 24 pi
        assert design_problem_error(pair, None) <= 1e-13


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_fail(mutant):
    """Each deliberate mistake changes the answer of a problem whose answer is known exactly: the
    impulse response for mistakes in the bank design, an integer problem for mistakes in indexing."""
    if mutant in ("phase", "tap_sign", "no_scale", "support"):
        errs = [design_problem_error(p, mutant) for p in ((48000, 22050), (16000, 22050))]
        print(mutant, errs)
        assert min(errs) > 1e-9
    else:
        triples = [(3, 2, 4), (147, 320, 14), (441, 320, 7)]
        assert all(index_problem_differs(t, mutant) for t in triples)
    # the definition itself does not trip either alarm
    assert not index_problem_differs((3, 2, 4), None)


def test_len_floor_mutant_only_differs_in_length():
    bank, x, _ = exact_problem(3, 2, 4, 1001)
    a, b = R.resample(x[0], 1001, bank, 3, 2, 4), R.resample(x[0], 1001, bank, 3, 2, 4, mutant="len_floor")
    assert len(a) == 1502 and len(b) == 1501 and np.array_equal(a[:1501], b)
    assert R.out_len(2 ** 31 - 1, 1024, 1) == (2 ** 31 - 1) * 1024      # 64-bit and beyond


def test_error_bound_holds_for_an_f32_evaluation_in_both_orders():
    for pair in R.PAIRS:
        up, down, half, taps = R.design(*pair)
        bank = taps.astype(np.float32)
        x = (0.5 * np.random.default_rng(3).normal(size=3000)).astype(np.float32)
        idx = np.arange(0, R.out_len(3000, up, down), 3)
        ref = R.resample(x, 3000, bank, up, down, half, idx)
        E = R.bound(x, 3000, bank, up, down, half, idx)
        r, X = R.gather(x, 3000, up, down, half, idx)
        P = bank[r] * X.astype(np.float32)
        fwd = np.zeros(len(idx), dtype=np.float32)
        bwd = np.zeros(len(idx), dtype=np.float32)
        for k in range(P.shape[1]):
            fwd = fwd + P[:, k]
            bwd = bwd + P[:, P.shape[1] - 1 - k]
        assert (np.abs(fwd - ref) <= E).all() and (np.abs(bwd - ref) <= E).all()
        assert E.max() < 1e-4      # the bound is not vacuous: signals of order 1
