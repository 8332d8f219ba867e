"""float64 numpy references of the polyphase resampler (tt2_resample, tt2.audio.resample_bank) and
the integer problems the exact tests share.  include/tt2_capi.h states the definition; this file
restates it independently of tt2.audio (numpy, np.i0) so that the two can be held against each other.

Every function takes `mutant`: None is the definition, a name from MUTANTS one deliberate mistake.
tests/test_resample_refs.py shows that each of them fails a problem with a known answer, i.e. that
the problems can tell the definition from its neighbours.

Error bound of an f32 evaluation: with u = 2^-24 and K = 2 * half + 1 taps,
    E[n] = (K + 2) * u * sum_k |bank[r][k] * x[i0 + k]|.
A sum of K products evaluated in any order with each product and each addition rounded once is
within ((1 + u)^K - 1) * sum |terms| of the exact sum (Higham, Accuracy and Stability, eq. 3.4: K - 1
additions and one rounding per product); with fmas there are fewer roundings.  (1 + u)^K - 1 <
(K + 1) u for K u < 0.01, and the last u covers rounding the float64 reference's own error and the
comparison.  The bound is fed the f32 bank the kernel is fed, so bank rounding is not in it."""
import math

import numpy as np

U = 2.0 ** -24
SR = 22050
DEFAULTS = dict(zeros=24, rolloff=0.9, beta=10.0)
PAIRS = [(48000, 22050), (44100, 22050), (24000, 22050), (16000, 22050), (22050, 16000), (96000, 22050)]
MORE_PAIRS = [(11025, 22050), (22050, 48000)]
MUTANTS = ("phase", "i0_round", "tap_sign", "len_floor", "no_scale", "support", "edge_clamp")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def ratio(sr_in, sr_out):
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def out_len(n, up, down, mutant=None):
    n, up, down = int(n), int(up), int(down)
    return n * up // down if mutant == "len_floor" else -(-n * up // down)


def cutoff(up, down, rolloff):
    return rolloff * min(1.0, up / down)


def proto(t, c, zeros, beta, mutant=None):
    """h(t) = c sinc(c t) w(c t / zeros) on an array of times in input samples."""
    t = np.asarray(t, dtype=np.float64)
    u = c * t / zeros
    lim = 1.0 - c / zeros if mutant == "support" else 1.0     # the window one input sample short
    w = np.where(np.abs(u) < lim, np.i0(beta * np.sqrt(np.clip(1.0 - u * u, 0.0, None))) / np.i0(beta), 0.0)
    return (1.0 if mutant == "no_scale" else c) * np.sinc(c * t) * w


def design(sr_in, sr_out, zeros=24, rolloff=0.9, beta=10.0, mutant=None):
    """(up, down, half, taps float64 [up, 2 * half + 1])."""
    up, down = ratio(sr_in, sr_out)
    c = cutoff(up, down, rolloff)
    half = math.ceil(zeros / c)
    r = np.arange(up, dtype=np.int64)
    f = ((r * up) % down if mutant == "phase" else (r * down) % up) / up
    k = np.arange(-half, half + 1, dtype=np.float64)
    t = k[None, :] + f[:, None] if mutant == "tap_sign" else k[None, :] - f[:, None]
    return up, down, half, proto(t, c, zeros, beta, mutant)


def gather(x, length, up, down, half, idx, mutant=None):
    """(r [N], X [N, K] float64): the bank row and the samples x[i0 + k], k = -half .. half, of the
    outputs idx, zero outside [0, length)."""
    n = np.asarray(idx, dtype=np.int64)
    q, r = n // up, n % up
    if mutant == "i0_round":
        i0 = q * down + (2 * r * down + up) // (2 * up)
    else:
        i0 = q * down + (r * down) // up
    pos = i0[:, None] + np.arange(-half, half + 1, dtype=np.int64)[None, :]
    ok = (pos >= 0) & (pos < length)
    xs = np.asarray(x, dtype=np.float64)
    if length == 0:
        return r, np.zeros(pos.shape)
    safe = np.clip(pos, 0, length - 1)
    X = xs[safe] if mutant == "edge_clamp" else np.where(ok, xs[safe], 0.0)
    return r, X


def resample(x, length, bank, up, down, half, idx=None, mutant=None):
    """y[n] of the definition for n in idx (default: every n < out_len), float64, from the first
    `length` samples of x.  bank [up, >= K] in any float type."""
    if idx is None:
        idx = np.arange(out_len(length, up, down, mutant))
    r, X = gather(x, length, up, down, half, idx, mutant)
    Bk = np.asarray(bank, dtype=np.float64)[:, :2 * half + 1][r]
    return (Bk * X).sum(axis=1) + 0.0


def bound(x, length, bank, up, down, half, idx=None):
    """E[n] of the module docstring for the same outputs."""
    if idx is None:
        idx = np.arange(out_len(length, up, down))
    r, X = gather(x, length, up, down, half, idx)
    Bk = np.asarray(bank, dtype=np.float64)[:, :2 * half + 1][r]
    return (2 * half + 1 + 2) * U * np.abs(Bk * X).sum(axis=1)


def zero_stuff(x, up, down, half, c, zeros, beta):
    """The textbook construction: zero-stuff by up, convolve with h(j / up), keep every down-th."""
    x = np.asarray(x, dtype=np.float64)
    J = (half + 1) * up
    g = proto(np.arange(-J, J + 1) / up, c, zeros, beta)
    xs = np.zeros(len(x) * up)
    xs[::up] = x
    v = np.convolve(xs, g)                      # v[m + J] = sum_i x[i] h(m / up - i)
    n = np.arange(out_len(len(x), up, down))
    return v[n * down + J]


# ---------------------------------------------------------------- integer problems (exact in f32)
EXACT_TRIPLES = [(1, 1, 0), (1, 2, 13), (2, 1, 7), (3, 2, 4), (147, 320, 14), (441, 320, 7), (320, 441, 9),
                 (147, 640, 127), (1024, 1023, 1)]


def exact_n_ins(half):
    K = 2 * half + 1
    return sorted({1, 2, max(K - 1, 1), K, 1000, 5003})


def int_bank(up, half, seed, selector=False):
    """[up, K] integers in [-8, 8] as float32; selector: one 1 per row, at a row-dependent tap."""
    K = 2 * half + 1
    if selector:
        bank = np.zeros((up, K), dtype=np.float32)
        bank[np.arange(up), (np.arange(up) * 7 + 3) % K] = 1.0
        return bank
    return np.random.default_rng(seed).integers(-8, 9, size=(up, K)).astype(np.float32)


def int_signal(batch, n_in, seed):
    """[batch, n_in] integers in [-64, 64] as float32."""
    return np.random.default_rng(seed).integers(-64, 65, size=(batch, n_in)).astype(np.float32)


def ragged_lens(batch, n_in, seed):
    """Lengths that include 0 and n_in (from batch 2 on) and otherwise anything in between."""
    lens = np.random.default_rng(seed).integers(0, n_in + 1, size=batch)
    lens[0] = n_in
    if batch > 1:
        lens[1] = 0
    return [int(v) for v in lens]


def is_exact(bank, x):
    """Every product and every partial sum, in any order, is an integer below 2^24."""
    bank, x = np.asarray(bank, dtype=np.float64), np.asarray(x, dtype=np.float64)
    whole = bool((bank == np.rint(bank)).all() and (x == np.rint(x)).all())
    return whole and np.abs(bank).sum(axis=1).max() * np.abs(x).max() < 2.0 ** 24


def tones(freqs, amps, phases, sr, n):
    """sum_i amps[i] sin(2 pi freqs[i] t / sr + phases[i]) for t = 0 .. n - 1, float64."""
    t = np.arange(n, dtype=np.float64)
    return sum(a * np.sin(2 * np.pi * f * t / sr + p) for f, a, p in zip(freqs, amps, phases))
