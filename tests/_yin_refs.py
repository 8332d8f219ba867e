"""Numpy references of tt2_yin (include/tt2_capi.h): YIN steps 1-5 without the best-local-estimate
step, plus the frame's RMS.

`yin_frame(y, ..., dtype=np.float64)` is the definition in float64.  With dtype=np.float32 it is the
f32 twin: every operation the definition names (subtract, square, each add of a sum, the multiply
by tau, the divide, the refinement's operations, the square root) is rounded to f32.  The sums of
the twin run in numpy's order, not the kernel's: the twin defines the kernel's bits only where the
sums are exact in any order, i.e. on the integer problems below (tests/test_yin_refs.py asserts
the premise: every d * tau and every S stays below 2^24).

Keyword arguments of `cmnd_of` and `select` switch on one deliberate mistake each (the mutants of
test_yin_refs.py); the defaults are the definition.
"""
import numpy as np

FRAME, WINDOW, MAX_LAG, HOP, SR = 1024, 512, 511, 256, 22050.0


def cmnd_of(y, dtype=np.float64, W=WINDOW, tau_factor=True, prefix_from_zero=False):
    """d'(0 .. MAX_LAG) of one frame y[1024] -> (cmnd, d, S), all `dtype`."""
    y = np.asarray(y).astype(dtype)
    taus = np.arange(MAX_LAG + 1)
    idx = np.minimum(np.arange(W)[:, None] + taus[None, :], FRAME - 1)   # (W = 513 mutant: clamp the one index past the frame)
    diff = (y[:W, None] - y[idx]).astype(dtype)
    d = np.sum((diff * diff).astype(dtype), axis=0, dtype=dtype)
    d[0] = 0
    S = np.cumsum(d, dtype=dtype)            # S(tau) = d(1) + ... + d(tau): d(0) is 0
    if prefix_from_zero:
        S = (S + dtype(1)).astype(dtype)
    num = (d * taus.astype(dtype)).astype(dtype) if tau_factor else d
    cm = np.ones(MAX_LAG + 1, dtype)
    pos = S > 0
    cm[pos] = (num[pos] / S[pos]).astype(dtype)
    cm[0] = 1
    return cm, d, S


def select(cm, tau_min, tau_max, threshold, sr=SR, dtype=np.float64, thr_le=False, walk_le=False, no_walk=False,
           tie_high=False, refine_edge=False):
    """The search and the outputs from d' -> dict(lag, voiced, aper, f0, refined, steps, abc).
    The threshold and sr are f32 values, as the kernel holds them."""
    cm = np.asarray(cm)
    thr = dtype(np.float32(threshold))
    sr = dtype(np.float32(sr))
    lag, voiced, steps = -1, False, 0
    for tau in range(tau_min, tau_max + 1):
        if cm[tau] <= thr if thr_le else cm[tau] < thr:
            lag, voiced = tau, True
            break
    if voiced and not no_walk:
        while lag + 1 <= tau_max and (cm[lag + 1] <= cm[lag] if walk_le else cm[lag + 1] < cm[lag]):
            lag += 1
            steps += 1
    if not voiced:
        seg = cm[tau_min:tau_max + 1]
        hit = np.flatnonzero(seg == seg.min())
        lag = tau_min + int(hit[-1] if tie_high else hit[0])
    aper = cm[lag]
    f0, refined, abc = dtype(0), False, None
    if voiced:
        inner = tau_min < lag < tau_max
        if inner or (refine_edge and 1 <= lag < MAX_LAG):
            a, b, c = cm[lag - 1], cm[lag], cm[lag + 1]
            abc = (a, b, c)
            num = dtype(dtype(0.5) * dtype(a - c))
            den = dtype(dtype(a - b) + dtype(c - b))
            off = dtype(num / den) if den != 0 else dtype(0)
            f0 = dtype(sr / dtype(dtype(lag) + off))
            refined = inner
        else:
            f0 = dtype(sr / dtype(lag))
    return dict(lag=lag, voiced=voiced, aper=aper, f0=f0, refined=refined, steps=steps, abc=abc)


def refined_f0(a, b, c, lag, sr=SR):
    """The refinement in float64 on given (a, b, c)."""
    a, b, c = float(a), float(b), float(c)
    return float(np.float32(sr)) / (lag + 0.5 * (a - c) / ((a - b) + (c - b)))


def energy_of(y, dtype=np.float64):
    y = np.asarray(y).astype(dtype)
    ss = np.sum((y * y).astype(dtype), dtype=dtype)
    return np.sqrt(dtype(ss * dtype(2.0 ** -10))).astype(dtype)


def yin_frame(y, tau_min, tau_max, threshold, sr=SR, dtype=np.float64, cmnd_kw=None, select_kw=None):
    cm, d, S = cmnd_of(y, dtype, **(cmnd_kw or {}))
    r = select(cm, tau_min, tau_max, threshold, sr, dtype, **(select_kw or {}))
    r.update(cmnd=cm, d=d, S=S, energy=energy_of(y, dtype))
    return r


U = 2.0 ** -24


def bits(v):
    return np.asarray(v, dtype=np.float32).view(np.int32)


def check_selection(out, b, f, cm, tmin, tmax, thr, sr=SR):
    """The f32 twin's selection on d' = cm (the twin's on the exact problem, the kernel's own on the
    random one) against a kernel's outputs out = dict(lag, aper, f0) of [B, T] arrays: lag and
    voicing exactly, aper and the unrefined f0 bit for bit, the refined f0 within 1e-6 relative of
    the float64 formula on (a, b, c)."""
    r = select(cm, tmin, tmax, thr, sr, dtype=np.float32)
    where = (b, f, tmin, tmax, thr)
    assert out["lag"][b, f] == r["lag"], (where, out["lag"][b, f], r["lag"])
    assert bits(out["aper"][b, f]) == bits(r["aper"]), (where, out["aper"][b, f], r["aper"])
    f0 = out["f0"][b, f]
    assert (f0 > 0) == r["voiced"], (where, f0)
    if not r["voiced"]:
        assert f0 == 0
    elif r["refined"]:
        want = refined_f0(*r["abc"], r["lag"], sr)
        assert abs(float(f0) - want) <= 1e-6 * want, (where, f0, want)
    else:
        assert bits(f0) == bits(np.float32(sr) / np.float32(r["lag"])), (where, f0)
    return r


def frames_of(x, t, hop=HOP):
    """[t, 1024] frames of one utterance's padded samples."""
    return np.stack([x[f * hop:f * hop + FRAME] for f in range(t)])


def reflect_pad(x, n, pad=FRAME // 2):
    """np.pad "reflect" of x[:n], as tt2_reflect_pad lays an utterance out."""
    return np.pad(np.asarray(x[:n]), pad, mode="reflect")


# ---- the exact integer problems (samples in {-3 .. 3})
def tiled(rng, period, n, perturb=0):
    """A random period tiled to n samples, then `perturb` samples moved by +-1 (kept in -3 .. 3)."""
    y = np.tile(rng.integers(-3, 4, period), n // period + 1)[:n].astype(np.int64)
    for p in rng.choice(n, perturb, replace=False):
        y[p] = y[p] + 1 if y[p] < 3 else y[p] - 1
    return y


def quantised_sine(period, n, amp=3.0, phase=0.3):
    return np.rint(amp * np.sin(2 * np.pi * np.arange(n) / period + phase)).astype(np.int64)


EXACT_B, EXACT_T, EXACT_FRAMES = 3, 9, (9, 4, 0)
EXACT_STRIDE = (EXACT_T - 1) * HOP + FRAME + 40      # larger than the 3072 samples the frames span
# (tau_min, tau_max, threshold): the parameter edges, then thresholds that d' meets exactly (d'(1) is
# 1 in every frame with d(1) > 0, and an all-zero frame has d' = 1 throughout)
EXACT_PARAMS = [(36, 340, 0.1), (1, 511, 0.1), (40, 40, 0.1), (1, 2, 0.1), (500, 511, 0.1),
                (1, 511, 1.0), (1, 2, 1.5), (1, 511, 1.5)]


def exact_signal(poison=True):
    """x [3, EXACT_STRIDE] float32.  Utterance 0 (9 frames): frame 0 a period-50 tile with 12
    perturbations, frame 4 a quantised sine of period 345 (a long downhill walk; it ends at
    tau_max = 340), frame 8 the tile (1, -1, 0) (an exact period 3: d' = 0 at every multiple of 3,
    so at tau_min = 36 too, and d(1) = d(2): a tied minimum over lags 1..2); the frames between
    straddle two of them.  Utterance 1 (4 frames): frame 0 all zeros, then a period-20 tile.
    Utterance 2 has no frame.  poison=True: every sample no valid frame may read is NaN."""
    rng = np.random.default_rng(2002)
    x = np.zeros((EXACT_B, EXACT_STRIDE))
    x[0, :FRAME] = tiled(rng, 50, FRAME, 12)
    x[0, FRAME:2 * FRAME] = quantised_sine(345, FRAME)
    x[0, 2 * FRAME:3 * FRAME] = np.tile([1, -1, 0], FRAME // 3 + 1)[:FRAME]
    x[0, 3 * FRAME:] = rng.integers(-3, 4, EXACT_STRIDE - 3 * FRAME)
    x[1, FRAME:] = tiled(rng, 20, EXACT_STRIDE - FRAME)
    x[2] = rng.integers(-3, 4, EXACT_STRIDE)
    if poison:
        for b, n in enumerate(EXACT_FRAMES):
            x[b, ((n - 1) * HOP + FRAME if n else 0):] = np.nan
    return x.astype(np.float32)


def exact_frames(hop=HOP, t=EXACT_T, frames=EXACT_FRAMES):
    """[(b, f, y)] of the valid frames of exact_signal at a hop."""
    x = exact_signal(poison=False)
    return [(b, f, x[b, f * hop:f * hop + FRAME]) for b in range(EXACT_B) for f in range(min(frames[b], t))]
