"""Numpy references of tt2_pitch_track (include/tt2_capi.h): the Viterbi path through the lags and
one unvoiced state over YIN's d'.

`track(c, ..., dtype=np.float64)` is the definition in float64.  With dtype=np.float32 it is the f32
twin: every operation the definition names (the subtraction of two positions, the product with
`jump`, each add, the refinement's operations) is rounded to f32.  The twin forms jump * |dp| and
the add as two rounded operations where the kernel may use one fma: the two agree wherever the
product is exact, i.e. on the exact problem below (tests/test_pitch_track_refs.py asserts the
premise), and the bound of the random problem covers both.

Keyword arguments of `track` switch on one deliberate mistake each (the mutants of
test_pitch_track_refs.py); the defaults are the definition.
"""
import itertools

import numpy as np

from _yin_refs import FRAME, HOP, SR, cmnd_of, select

MUTANTS = ("v_le", "u_le", "end_le", "tie_high", "no_switch_uv", "no_switch_vu", "no_unvoiced0", "lag_diff",
           "shift", "refine_any")
UNVOICED = -1   # the unvoiced state among the states 0 .. S - 1 (state i = lag tau_min + i)


def _argmin(x, tie_high):
    """Index of the minimum along the last axis: the lowest on a tie (the highest for the mutant)."""
    if tie_high:
        return x.shape[-1] - 1 - np.argmin(x[..., ::-1], axis=-1)
    return np.argmin(x, axis=-1)


def track(c, tau_min, tau_max, pos, jump, switch, unvoiced, sr=SR, dtype=np.float64, v_le=False, u_le=False,
          end_le=False, tie_high=False, no_switch_uv=False, no_switch_vu=False, no_unvoiced0=False, lag_diff=False,
          shift=False, refine_any=False, record=None):
    """One utterance.  c [N, >= tau_max + 1] = d' of the N valid frames (column = lag), pos
    [>= tau_max + 1] -> dict(lag [N] int, f0 [N], cost, states [N] (UNVOICED or state index), refined
    [N] bool, abc {f: (a, b, c)}).  jump / switch / unvoiced / sr are f32 values, as the kernel holds
    them.  record, a list, receives every array of values the recurrence forms."""
    c = np.asarray(c)
    N = c.shape[0]
    if N == 0:
        return dict(lag=np.zeros(0, np.int64), f0=np.zeros(0, dtype), cost=dtype(0), states=np.zeros(0, np.int64),
                    refined=np.zeros(0, bool), abc={})
    J, W, C, srd = (dtype(np.float32(v)) for v in (jump, switch, unvoiced, sr))
    lags = np.arange(tau_min, tau_max + 1)
    S = len(lags)
    cc = c[:, tau_min:tau_max + 1].astype(dtype)
    p = (lags if lag_diff else np.asarray(pos)[tau_min:tau_max + 1]).astype(dtype)
    dp = np.abs((p[:, None] - p[None, :]).astype(dtype))   # [target, source]
    JD = (J * dp).astype(dtype)
    note = record.append if record is not None else (lambda x: None)
    note(dp), note(JD)
    V = cc[0].copy()
    U = dtype(0) if no_unvoiced0 else C
    from_v = np.zeros((N, S), np.int64)    # predecessor of voiced state i at frame f (UNVOICED or index)
    from_u = np.zeros(N, np.int64)         # predecessor of the unvoiced state
    for f in range(1, N):
        X = (V[None, :] + JD).astype(dtype)
        arg = _argmin(X, tie_high)
        A = X[np.arange(S), arg]
        uw = U if no_switch_uv else dtype(U + W)
        take_u = (uw <= A) if v_le else (uw < A)
        m_arg = int(_argmin(V, tie_high))
        mw = V[m_arg] if no_switch_vu else dtype(V[m_arg] + W)
        take_v = (mw <= U) if u_le else (mw < U)
        note(X), note(np.asarray([uw, mw]))
        from_v[f] = np.where(take_u, UNVOICED, arg)
        from_u[f] = m_arg if take_v else UNVOICED
        V = (cc[f] + np.where(take_u, uw, A).astype(dtype)).astype(dtype)
        U = dtype(C + (mw if take_v else U))
        note(V), note(np.asarray([U]))
    e_arg = int(_argmin(V, tie_high))
    end_u = (U <= V[e_arg]) if end_le else (U < V[e_arg])
    st = UNVOICED if end_u else e_arg
    cost = U if end_u else V[e_arg]
    states = np.zeros(N, np.int64)
    for f in range(N - 1, -1, -1):
        states[f] = st
        if f:
            st = from_u[f] if st == UNVOICED else from_v[f, st]
    if shift:
        states = np.concatenate([states[1:], states[-1:]])
    lag = np.where(states == UNVOICED, 0, states + tau_min)
    f0 = np.zeros(N, dtype)
    refined = np.zeros(N, bool)
    abc = {}
    for f in range(N):
        t = int(lag[f])
        if t == 0:
            continue
        f0[f] = dtype(srd / dtype(t))
        if tau_min < t < tau_max:
            a, b, cq = (dtype(v) for v in c[f, t - 1:t + 2])
            if (a > b and cq >= b) or refine_any:
                num = dtype(dtype(0.5) * dtype(a - cq))
                den = dtype(dtype(a - b) + dtype(cq - b))
                off = dtype(num / den) if den != 0 else dtype(0)
                f0[f] = dtype(srd / dtype(dtype(t) + off))
                refined[f] = a > b and cq >= b
                abc[f] = (a, b, cq)
    return dict(lag=lag, f0=f0, cost=cost, states=states, refined=refined, abc=abc)


def path_cost(states, c, tau_min, tau_max, pos, jump, switch, unvoiced, dtype=np.float64):
    """The cost of a given state sequence (UNVOICED or state index per frame), summed as the
    recurrence sums it: value = c + (value before + transition)."""
    J, W, C = (dtype(np.float32(v)) for v in (jump, switch, unvoiced))
    p = np.asarray(pos)[tau_min:tau_max + 1].astype(dtype)
    cc = np.asarray(c)[:, tau_min:tau_max + 1].astype(dtype)
    if len(states) == 0:
        return dtype(0)
    s = states[0]
    acc = C if s == UNVOICED else cc[0, s]
    for f in range(1, len(states)):
        q, s = s, states[f]
        if s == UNVOICED:
            acc = dtype(C + (acc if q == UNVOICED else dtype(acc + W)))
        elif q == UNVOICED:
            acc = dtype(cc[f, s] + dtype(acc + W))
        else:
            acc = dtype(cc[f, s] + dtype(acc + dtype(J * np.abs(dtype(p[s] - p[q])))))
    return acc


def states_of(lag, tau_min):
    lag = np.asarray(lag, np.int64)
    return np.where(lag == 0, UNVOICED, lag - tau_min)


def brute_force(c, tau_min, tau_max, pos, jump, switch, unvoiced):
    """The minimum of path_cost over all (S + 1)^N state sequences (float64)."""
    S, N = tau_max - tau_min + 1, np.asarray(c).shape[0]
    return min(path_cost(seq, c, tau_min, tau_max, pos, jump, switch, unvoiced)
               for seq in itertools.product(range(-1, S), repeat=N))


def refined_f0(a, b, c, lag, sr=SR):
    """The refinement in float64 on given (a, b, c)."""
    a, b, c = float(a), float(b), float(c)
    return float(np.float32(sr)) / (lag + 0.5 * (a - c) / ((a - b) + (c - b)))


def bits(v):
    return np.asarray(v, dtype=np.float32).view(np.int32)


# ---- the exact problem: d' in {0, 1/8, .. 1}, integer positions, parameters multiples of 1/4
EXACT_B, EXACT_T, EXACT_FRAMES = 4, 9, (9, 4, 1, 0)
EXACT_RANGES = [(36, 340), (1, 511), (40, 40), (1, 2), (500, 511)]
EXACT_PARAMS = [(0.25, 0.5, 0.25), (0.0, 0.25, 0.5), (0.5, 0.0, 0.25), (0.25, 0.25, 0.0), (1.0, 0.5, 0.75),
                (0.25, 0.0, 0.0)]   # (jump, switch, unvoiced)
EXACT_LD = 520   # wider than tau_max + 1 for every range


def exact_pos():
    """An increasing integer-valued table over the lags 0 .. 511 with steps of 1 and 2."""
    rng = np.random.default_rng(11)
    return np.cumsum(rng.integers(1, 3, 512)).astype(np.float32)


def exact_cmnd(tau_min, tau_max, poison=True):
    """cmnd [4, 9, EXACT_LD] float32 in eighths.  Most values are high (3/8 .. 1); each frame has a few
    low ones near a slowly moving lag, some tied, and some frames have none (the unvoiced state
    wins there).  poison=True: every element the definition does not read is NaN."""
    rng = np.random.default_rng(1000 * tau_min + tau_max)
    S = tau_max - tau_min + 1
    c = rng.integers(3, 9, (EXACT_B, EXACT_T, EXACT_LD)).astype(np.float64)
    for b in range(EXACT_B):
        centre = rng.integers(0, S)
        for f in range(EXACT_T):
            if (b == 0 and f in (3, 4)) or (b == 1 and f == 0):
                continue   # a frame with no low value
            centre = int(np.clip(centre + rng.integers(-2, 3), 0, S - 1))
            for k in rng.integers(-3, 4, 4):
                i = int(np.clip(centre + k, 0, S - 1))
                c[b, f, tau_min + i] = rng.integers(0, 3)
            if S > 20:    # a far rival: a jump pays only where `jump` is small
                c[b, f, tau_min + (centre + S // 2) % S] = 0
    c /= 8.0
    if poison:
        c[:, :, :tau_min] = np.nan
        c[:, :, tau_max + 1:] = np.nan
        for b, n in enumerate(EXACT_FRAMES):
            c[b, n:] = np.nan
    return c.astype(np.float32)


def exact_cases():
    """[(tau_min, tau_max, jump, switch, unvoiced)]"""
    return [(lo, hi) + p for lo, hi in EXACT_RANGES for p in EXACT_PARAMS]


def check_outputs(out, b, r, t, sr=SR):
    """A kernel's outputs out = dict(lag, f0, cost) of [B, T] / [B] arrays against the f32 twin's
    result r of utterance b: lags exactly, cost and the unrefined f0 bit for bit, the refined f0
    within 1e-6 relative of the float64 formula on (a, b, c); -1 and 0 past the valid frames."""
    n = len(r["lag"])
    assert np.array_equal(out["lag"][b, :n], r["lag"]), (b, out["lag"][b, :n], r["lag"])
    assert np.all(out["lag"][b, n:t] == -1) and np.all(bits(out["f0"][b, n:t]) == 0), b
    assert bits(out["cost"][b]) == bits(r["cost"]), (b, out["cost"][b], r["cost"])
    for f in range(n):
        got = out["f0"][b, f]
        if r["refined"][f]:
            want = refined_f0(*r["abc"][f], int(r["lag"][f]), sr)
            assert abs(float(got) - want) <= 1e-6 * want, (b, f, got, want)
        else:
            assert bits(got) == bits(r["f0"][f]), (b, f, got, r["f0"][f])


# ---- the planted track: 200 frames, the real log2 table
PLANT_T, PLANT_RANGE, PLANT_UNVOICED = 200, (37, 339), (80, 120)
DEFAULTS = (1.0, 0.1, 0.2)   # jump, switch, unvoiced of PitchTracker


def log2_pos(n=512):
    """pos[tau] = log2(tau) in float64, rounded to f32 (pos[0] = 0: never read)."""
    return np.log2(np.maximum(np.arange(n), 1).astype(np.float64)).astype(np.float32)


def planted():
    """(cmnd [200, 512] float32, lag [200]): uniform [0.5, 1.5] noise, 0.05 along a smooth track, and
    1.0 in every lag of the frames 80 .. 119 (lag 0 there)."""
    rng = np.random.default_rng(5)
    c = rng.uniform(0.5, 1.5, (PLANT_T, 512)).astype(np.float32)
    f = np.arange(PLANT_T)
    lag = np.rint(180 + 70 * np.sin(2 * np.pi * f / PLANT_T) + 12 * np.sin(2 * np.pi * f / 37)).astype(np.int64)
    c[f, lag] = 0.05
    c[PLANT_UNVOICED[0]:PLANT_UNVOICED[1]] = 1.0
    lag[PLANT_UNVOICED[0]:PLANT_UNVOICED[1]] = 0
    return c, lag


# ---- the glide: a harmonic tone whose odd harmonics fade in frames 20 .. 27, then noise
GLIDE_T, GLIDE_RANGE = 60, (37, 339)


def glide_signal():
    """(x [59 * 256 + 1024] float64, true lag [60]): frame f is x[256 f : 256 f + 1024]."""
    rng = np.random.default_rng(7)
    L = (GLIDE_T - 1) * HOP + FRAME
    t = np.arange(L)
    f0 = 110 * 2 ** (0.15 * np.sin(2 * np.pi * t / L))
    ph = 2 * np.pi * np.cumsum(f0) / 22050
    w = np.ones(L)
    w[20 * HOP + 512:28 * HOP + 512] = 0.12
    x = np.zeros(L)
    for h in range(1, 9):
        x += (1.0 / h) * (w if h % 2 else 1.0) * np.sin(h * ph + h)
    x += 0.02 * rng.standard_normal(L)
    x[45 * HOP + 512:] = 0.3 * rng.standard_normal(L - (45 * HOP + 512))
    truth = 22050 / f0[HOP * np.arange(GLIDE_T) + 512]
    return x, truth


_GLIDE = {}


def glide_cmnd():
    """d' [60, 512] float32 of the glide's frames from cmnd_of(..., float32); computed once."""
    if "c" not in _GLIDE:
        x, truth = glide_signal()
        _GLIDE["c"] = np.stack([cmnd_of(x[HOP * f:HOP * f + FRAME], np.float32)[0] for f in range(GLIDE_T)])
        _GLIDE["truth"] = truth
    return _GLIDE["c"], _GLIDE["truth"]


def glide_tracked_ok(lag, truth):
    """The tracker's condition: a voiced lag within 3 of the truth in frames 0 .. 27 and 30 .. 44,
    unvoiced in frames 45 .. 59; frames 28 .. 29 are free.  -> list of offending frames."""
    lag = np.asarray(lag)
    bad = [f for f in list(range(0, 28)) + list(range(30, 45)) if not (lag[f] > 0 and abs(lag[f] - truth[f]) <= 3)]
    return bad + [f for f in range(45, 60) if lag[f] != 0]


def glide_octave_errors(lag, truth):
    """How many of frames 20 .. 27 carry a voiced lag under 0.6 x the true one."""
    lag = np.asarray(lag)
    return sum(1 for f in range(20, 28) if 0 < lag[f] < 0.6 * truth[f])


def select_lags(c, tau_min, tau_max, threshold=0.1):
    """tt2_yin's per-frame selection on d' rows: the lag where voiced, else 0."""
    out = []
    for row in c:
        r = select(row, tau_min, tau_max, threshold, dtype=np.float32)
        out.append(r["lag"] if r["voiced"] else 0)
    return np.asarray(out)


# ---- the random problem and its bound
def random_problem(seed, B, T, frames):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (B, T, 512)).astype(np.float32), np.asarray(frames, np.int32)


def random_bound(N, c_max, pos, tau_min, tau_max, jump, switch, unvoiced):
    """E = 6 N 2^-24 M with M = N (max(c, C) + max(J (p_max - p_min), W)): a value of the recurrence
    is at most M, a frame adds at most three roundings (the product, and the two adds; one fewer
    with an fma) of relative size 2^-24 each, and two paths are compared."""
    p = np.asarray(pos, np.float64)[tau_min:tau_max + 1]
    M = N * (max(c_max, unvoiced) + max(jump * (p.max() - p.min()), switch))
    return 6 * N * 2.0 ** -24 * M
