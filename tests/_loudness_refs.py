"""float64 references for tt2_loudness (include/tt2_capi.h has the definition), shared by
tests/test_loudness_refs.py (CPU) and the GPU files.

* ``kweighting``: the K-weighting design, written out independently of tt2.audio.kweighting.
* ``reference``: the definition with two scipy.signal.lfilter sections (float64, unchunked), the
  sub-block sums, blocks, both gates with sequential ascending sums, loudness, peak, gain, y.
* ``brute``: the same by a plain loop over the samples (direct form I, as the header writes it).
* ``chunked_filter``: a float64 model of the kernel's scheme for any chunk length and any power of
  two of chunks per segment: every chunk from zero state, a Kogge-Stone scan with A^(chunk d) over a
  segment, the same scan over the segments' end states, the scan again from the true entry state,
  every chunk again from its true entry state.  Its matrices come from the coefficients by
  square-and-multiply.  ``track`` collects every intermediate.
* ``exact_problems``: integer problems.  The sections' denominators are 1 + z^-2 and 1 - z^-1 + z^-2
  (state matrices of period 4 and 6, so that every power is an integer matrix) or 1, the numerators'
  taps lie in {-1, 0, 1, 2}, and x = a1 * a2 * w with w integers in [-12, 12], so the outputs are the
  small integers b1 * b2 * w.  ``exact`` asserts that every intermediate of the chunked model is an
  integer below 2^53, every sub-block sum below 2^24 and every sample an integer: then every
  bit of energy, peak, limited and the gate decisions is defined; gain and y are defined because
  the division, the square root and the f32 roundings are correctly rounded IEEE operations.
* ``MUTANTS``: wrong readings of the definition, each of which some exact problem tells from it.
* ``random_problem``: Gaussian noise under stepped envelopes at the default 22.05 kHz coefficients.
"""
import numpy as np
from scipy.signal import lfilter

KERNEL_CHUNK, KERNEL_LANES = 16, 64          # csrc/loudness.hip: LK_C, and the 64 chunks of a segment
KERNEL_SEG = KERNEL_CHUNK * KERNEL_LANES


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def clamp_len(v, n_in):
    return n_in if v is None else min(max(int(v), 0), n_in)


def kweighting(sr):
    """((b, a), (b, a)) float64: the shelf and the high-pass of BS.1770 at the rate sr."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    s1 = (np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]),
          np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    s2 = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    return s1, s2


def coef10(sections):
    (b1, a1), (b2, a2) = sections
    return [float(v) for v in (*b1, a1[1], a1[2], *b2, a2[1], a2[2])]


def default_params(sr=22050, target=-23.0, peak_db=-1.0):
    """What LoudnessNormalizer passes to the kernel."""
    step = sr // 10
    return dict(step=step, coef=coef10(kweighting(sr)), abs_sum=4.0 * step * 10.0 ** ((-70.0 + 0.691) / 10.0),
                rel_ratio=0.1, target_ms=10.0 ** ((target + 0.691) / 10.0),
                ceiling=float(np.float32(10.0 ** (peak_db / 20.0))))


# ------------------------------------------------------------------------------------------ filters
def filter_lfilter(x, coef):
    c = coef
    y1 = lfilter(c[0:3], [1.0, c[3], c[4]], np.asarray(x, dtype=np.float64))
    return lfilter(c[5:8], [1.0, c[8], c[9]], y1)


def filter_brute(x, coef):
    """y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2], twice, sample by sample."""
    v = [float(s) for s in x]
    for b0, b1, b2, a1, a2 in (coef[0:5], coef[5:10]):
        out, x1, x2, y1, y2 = [], 0.0, 0.0, 0.0, 0.0
        for s in v:
            y = b0 * s + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
            x2, x1, y2, y1 = x1, s, y1, y
            out.append(y)
        v = out
    return np.array(v, dtype=np.float64)


def one_sample_matrix(c):
    """A of s' = A s + B x, s = (z1, z2, w1, w2) of the two sections in transposed direct form II."""
    return np.array([[-c[3], 1.0, 0.0, 0.0],
                     [-c[4], 0.0, 0.0, 0.0],
                     [c[6] - c[8] * c[5], 0.0, -c[8], 1.0],
                     [c[7] - c[9] * c[5], 0.0, -c[9], 0.0]])


def mat_pow(A, n, track=None):
    """A^n by square-and-multiply (n >= 1)."""
    out, p = None, A.copy()
    while n:
        if n & 1:
            out = p.copy() if out is None else out @ p
        n >>= 1
        if n:
            p = p @ p
        if track is not None:
            track.append(p)
    if track is not None:
        track.append(out)
    return out


def _run(xc, nc, c, s):
    """Rows of xc [N, chunk] from the states s [N, 4], nc [N] samples each: (end states, y)."""
    z1, z2, w1, w2 = (s[:, i].copy() for i in range(4))
    y = np.zeros_like(xc)
    for i in range(xc.shape[1]):
        live = i < nc
        x = xc[:, i]
        y1 = c[0] * x + z1
        n1 = c[1] * x + (-c[3] * y1 + z2)
        n2 = -c[4] * y1 + c[2] * x
        y2 = c[5] * y1 + w1
        m1 = c[6] * y1 + (-c[8] * y2 + w2)
        m2 = -c[9] * y2 + c[7] * y1
        z1, z2 = np.where(live, n1, z1), np.where(live, n2, z2)
        w1, w2 = np.where(live, m1, w1), np.where(live, m2, w2)
        y[:, i] = np.where(live, y2, 0.0)
    return np.stack([z1, z2, w1, w2], 1), y


def _kogge_stone(e, mats, track):
    """Inclusive scan along axis -2 of e [..., lanes, 4]: at distance d, e_l <- M_d e_(l-d) + e_l."""
    e = e.copy()
    d, k = 1, 0
    while d < e.shape[-2]:
        e[..., d:, :] = e[..., :-d, :] @ mats[k].T + e[..., d:, :]
        if track is not None:
            track.append(e.copy())
        d, k = 2 * d, k + 1
    return e


def chunked_filter(x, coef, chunk=KERNEL_CHUNK, lanes=KERNEL_LANES, track=None, zero_chunk_seam=False,
                   zero_segment_seam=False, drop_section2=False):
    """The kernel's scheme in float64 (module docstring).  The three flags are mutants."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if n == 0:
        return np.zeros(0)
    seg = chunk * lanes
    nseg = -(-n // seg)
    A = one_sample_matrix(coef)
    nlev = max(1, lanes.bit_length() - 1)
    cm = [mat_pow(A, chunk << k, track) for k in range(nlev)]               # A^(chunk 2^k)
    sm = [mat_pow(A, seg << k, track) for k in range(nlev)]                 # A^(seg 2^k)
    xc = np.zeros(nseg * seg)
    xc[:n] = x
    xc = xc.reshape(nseg * lanes, chunk)
    nc = np.clip(n - chunk * np.arange(nseg * lanes), 0, chunk)
    zero = np.zeros((nseg * lanes, 4))
    # 1: every chunk from zero state, scanned over its segment; the last lane has the segment's end state
    e, _ = _run(xc, nc, coef, zero)
    inc = _kogge_stone(e.reshape(nseg, lanes, 4), cm, track)
    E = inc[:, -1, :]
    # 2: the segments' entry states, a round of `lanes` segments at a time
    entry = np.zeros((nseg, 4))
    state_in = np.zeros(4)
    for base in range(0, nseg, lanes):
        r = np.zeros((lanes, 4))
        m = min(lanes, nseg - base)
        r[:m] = E[base:base + m]
        r[0] = sm[0] @ state_in + r[0]
        r = _kogge_stone(r, sm, track)
        entry[base] = state_in
        entry[base + 1:base + m] = r[:m - 1]
        state_in = r[-1]
    if zero_segment_seam:
        entry[:] = 0.0
    # 3: the scan again, the first chunk of a segment from the segment's entry state
    first = zero.copy().reshape(nseg, lanes, 4)
    first[:, 0, :] = entry
    e, _ = _run(xc, nc, coef, first.reshape(-1, 4))
    inc = _kogge_stone(e.reshape(nseg, lanes, 4), cm, track)
    true_in = np.concatenate([entry[:, None, :], inc[:, :-1, :]], 1).reshape(-1, 4)
    if zero_chunk_seam:
        true_in = first.reshape(-1, 4)
    if drop_section2:
        true_in[1:, 2:] = 0.0
    end, y = _run(xc, nc, coef, true_in)
    if track is not None:
        track.extend([e, true_in, end, y, entry])
    return y.reshape(-1)[:n]


# ---------------------------------------------------------------------------------------- reference
MUTANTS = ("abs_gate_not_strict", "rel_gate_not_strict", "rel_threshold_from_all_blocks", "offset_dropped",
           "three_step_blocks", "partial_sub_block_counted", "state_zeroed_at_chunk_seam",
           "state_zeroed_at_segment_seam", "section2_state_not_carried", "a1_a2_swapped", "peak_over_padding",
           "ceiling_ignored", "gain_from_ungated_mean", "limited_inverted")


def seq_sum(v):
    """The sum from +0 in ascending order."""
    return float(np.cumsum(np.asarray(v, dtype=np.float64))[-1]) if len(v) else 0.0


def gate(sub, step, abs_sum, rel_ratio, mutant=None):
    """(ms or None, E, passes absolute gate, passes both gates, G1 or None) from sub-block sums."""
    sub = np.asarray(sub, dtype=np.float64)
    k = 3 if mutant == "three_step_blocks" else 4
    N = max(0, len(sub) - (k - 1))
    E = np.zeros(N)
    for i in range(k):
        E = E + sub[i:i + N] if i else sub[:N].copy()
    pa = E >= abs_sum if mutant == "abs_gate_not_strict" else E > abs_sum
    both = np.zeros(N, dtype=bool)
    if not pa.any():
        return None, E, pa, both, None
    G1 = seq_sum(E) / N if mutant == "rel_threshold_from_all_blocks" else seq_sum(E[pa]) / int(pa.sum())
    thr = rel_ratio * G1
    both = pa & (E >= thr if mutant == "rel_gate_not_strict" else E > thr)
    if not both.any():
        return None, E, pa, both, G1
    G2 = seq_sum(E[both]) / int(both.sum())
    if mutant == "gain_from_ungated_mean":
        G2 = seq_sum(E) / N
    return G2 / (4.0 * step), E, pa, both, G1


def reference(x, lens, step, coef, abs_sum, rel_ratio, target_ms, ceiling, n_out, mutant=None, filt=None, **_):
    """The definition for a batch.  x [B, n_in] (whatever lies at or past len_b is not used), lens a list
    (unclamped) or None.  Returns a dict: y [B, n_out] f32, loud / gain / peak [B] f32, limited [B]
    int, energy [B, n_in // step + 1] float64, sub (list of float64 arrays), ms, gates (E, absolute, both)."""
    x = np.asarray(x, dtype=np.float32)
    B, n_in = x.shape
    coef = list(coef)
    if mutant == "a1_a2_swapped":
        coef[3], coef[4], coef[8], coef[9] = coef[4], coef[3], coef[9], coef[8]
    if filt is None:
        filt = filter_lfilter
        if mutant == "state_zeroed_at_chunk_seam":
            filt = lambda v, c: chunked_filter(v, c, zero_chunk_seam=True)        # noqa: E731
        elif mutant == "state_zeroed_at_segment_seam":
            filt = lambda v, c: chunked_filter(v, c, zero_segment_seam=True)      # noqa: E731
        elif mutant == "section2_state_not_carried":
            filt = lambda v, c: chunked_filter(v, c, drop_section2=True)          # noqa: E731
    ne = n_in // step + 1
    out = dict(y=np.zeros((B, n_out), dtype=np.float32), loud=np.zeros(B, dtype=np.float32),
               gain=np.ones(B, dtype=np.float32), peak=np.zeros(B, dtype=np.float32), limited=np.zeros(B, dtype=np.int64),
               energy=np.zeros((B, ne)), sub=[], ms=[], gates=[])
    for b in range(B):
        L = clamp_len(None if lens is None else lens[b], n_in)
        xv = x[b, :L].astype(np.float64)
        yv = filt(xv, coef) if L else np.zeros(0)
        S = -(-L // step) if mutant == "partial_sub_block_counted" else L // step
        sq = np.zeros(S * step)
        sq[:min(L, S * step)] = (yv * yv)[:S * step]
        sub = sq.reshape(S, step).sum(1) if S else np.zeros(0)
        ms, E, pa, both, _ = gate(sub, step, abs_sum, rel_ratio, mutant)
        seen = x[b] if mutant == "peak_over_padding" else x[b, :L]
        peak = np.float32(np.abs(seen).max()) if seen.size else np.float32(0.0)
        g, limited = np.float32(1.0), 0
        if ms is None:
            loud = np.float32(-np.inf)
        else:
            loud = np.float32((0.0 if mutant == "offset_dropped" else -0.691) + 10.0 * np.log10(ms))
            gd = np.sqrt(target_ms / ms)
            if peak > 0 and mutant != "ceiling_ignored":
                c = float(np.float32(ceiling)) / float(peak)
                if c < gd:
                    gd, limited = c, 1
            g = np.float32(gd)
            if mutant == "limited_inverted":
                limited = 1 - limited
        m = min(L, n_out)
        out["y"][b, :m] = g * x[b, :m]                       # one f32 multiply
        out["loud"][b], out["gain"][b], out["peak"][b], out["limited"][b] = loud, g, peak, limited
        out["energy"][b, :min(S, ne)] = sub[:ne]
        out["sub"].append(sub)
        out["ms"].append(ms)
        out["gates"].append((E, pa, both))
    return out


def same(got, ref, keys=("y", "loud", "gain", "peak", "limited", "energy")):
    """The names of the outputs of `got` that differ from `ref` in a bit (energy compared as f32)."""
    bad = []
    for k in keys:
        if k == "limited":
            if [int(v) for v in got[k]] != [int(v) for v in ref[k]]:
                bad.append(k)
        elif not np.array_equal(bits(got[k]), bits(ref[k])):
            bad.append(k)
    return bad


# ------------------------------------------------------------------------------------ exact problems
IDENT = ([1, 0, 0], [1, 0, 0])
FILTERS = {
    "p4-p6": (([1, 0, -1], [1, 0, 1]), ([2, -1, 0], [1, -1, 1])),
    "p6-id": (([1, 2, 0], [1, -1, 1]), IDENT),
    "id-p4": (IDENT, ([0, 1, -1], [1, 0, 1])),
    "p4-p4": (([1, 0, 0], [1, 0, 1]), ([1, 1, 0], [1, 0, 1])),     # a double pole pair: the carries grow with n
    "id-id": (IDENT, IDENT),
}
STEPS = (1, 4, 5, 2205)
JUNK = 1000.0          # what the references see past len_b (the GPU tests put NaN there)


def exact_utterance(rng, n, sections, scales):
    """x [n] = a1 * a2 * w for integers w = scale * {-3 .. 3}, the scale stepping through `scales` in
    equal parts: the filter's output is then b1 * b2 * w."""
    (b1, a1), (b2, a2) = sections
    if n == 0:
        return np.zeros(0)
    part = -(-n // len(scales))
    env = np.repeat(np.asarray(scales, dtype=np.float64), part)[:n]
    w = rng.integers(-3, 4, size=n) * env
    return np.convolve(np.convolve(a1, a2), w)[:n]


def make_problem(name, fname, step, n_in, lens, scales, seed, abs_sum, target_ms, ceiling, n_out, rel_ratio=0.125):
    rng = np.random.default_rng(seed)
    sections = FILTERS[fname]
    x = np.full((len(lens), n_in), JUNK, dtype=np.float32)
    for b, v in enumerate(lens):
        L = clamp_len(v, n_in)
        x[b, :L] = exact_utterance(rng, L, sections, scales[b % len(scales)])
    return dict(name=name, x=x, lens=list(lens), step=step, coef=coef10(sections), abs_sum=float(abs_sum),
                rel_ratio=rel_ratio, target_ms=float(target_ms), ceiling=float(ceiling), n_out=n_out)


def threshold_problems():
    """Identity sections, step 1: y = x, so the blocks can be read off.  x = 4 x7, 0 x4, 2 2, 0 x4 has the
    block sums 64 64 64 64 48 32 16 0 4 8 8 8 4 0.  With abs_sum = 3 twelve blocks pass, G1 = 384 / 12 = 32
    and the relative threshold is exactly 4: the two blocks of 4 sit on it and fail, G2 = 376 / 10.  With
    abs_sum = 4 those two sit on the absolute gate and fail, G1 = G2 = 376 / 10."""
    x = np.array([[4] * 7 + [0] * 4 + [2, 2] + [0] * 4], dtype=np.float32)
    out = []
    for name, abs_sum in (("on-rel-threshold", 3.0), ("on-abs-threshold", 4.0)):
        out.append(dict(name=name, x=x.copy(), lens=[17], step=1, coef=coef10(FILTERS["id-id"]), abs_sum=abs_sum,
                        rel_ratio=0.125, target_ms=2.0 ** -4, ceiling=0.5, n_out=17))
    return out


def exact_problems():
    """The list that both the CPU and the GPU file run.  Each is ragged with B = 5 (the threshold
    problems: B = 1); among the lengths 4 step - 1, 4 step, 4 step + 1, every chunk and segment seam
    of the kernel +- 1, 0, a negative one and one above n_in."""
    loud_quiet_silent = [(4, 1, 0), (1, 4, 1), (0, 4, 4), (1,), (4, 0, 1, 4)]
    ps = threshold_problems()
    seed = 100
    for step in STEPS:
        s4 = 4 * step
        groups = [
            [s4 - 1, s4, s4 + 1, 0, -5],
            [KERNEL_CHUNK - 1, KERNEL_CHUNK, KERNEL_CHUNK + 1, 2 * KERNEL_CHUNK + 1, 3 * KERNEL_CHUNK - 1],
            [KERNEL_SEG - 1, KERNEL_SEG, KERNEL_SEG + 1, 2 * KERNEL_SEG - 1, 2 * KERNEL_SEG + 1],
            [3 * KERNEL_SEG + 7, 10 ** 6, 2 * KERNEL_SEG, 700, 1500],
        ]
        if step == 2205:
            groups = [[s4 - 1, s4, s4 + 1, 0, -5], [3 * s4 + 17, 10 ** 6, 2 * s4 + KERNEL_SEG + 1, KERNEL_SEG - 1, 9 * step]]
        for gi, lens in enumerate(groups):
            fname = list(FILTERS)[(gi + STEPS.index(step)) % 4]
            n_in = max(min(v, 3 * KERNEL_SEG + 40) for v in lens) + (3 if gi % 2 else 0)
            if step == 2205:
                n_in = max(min(v, 3 * s4 + 30) for v in lens) + (3 if gi % 2 else 0)
            seed += 1
            # the absolute gate at a mean square of 2; a target that the loud utterances miss under the ceiling
            ps.append(make_problem(f"step{step}-g{gi}-{fname}", fname, step, n_in, lens, loud_quiet_silent, seed,
                                   abs_sum=8.0 * step, target_ms=2.0 ** (gi - 1), ceiling=2.0 ** (gi - 4),
                                   n_out=n_in + 5 if gi % 2 else max(n_in - 9, n_in // 2)))
    return ps


def exact(p, chunk=KERNEL_CHUNK, lanes=KERNEL_LANES):
    """True iff every value the scheme meets on problem p is exactly representable (module docstring)."""
    x = np.asarray(p["x"], dtype=np.float32)
    n_in = x.shape[1]
    for b in range(x.shape[0]):
        L = clamp_len(p["lens"][b] if p["lens"] is not None else None, n_in)
        xv = x[b, :L].astype(np.float64)
        track = []
        y = chunked_filter(xv, p["coef"], chunk, lanes, track)
        for t in track + [xv, np.asarray(p["coef"])]:
            t = np.asarray(t)
            if t.size and not (np.all(t == np.rint(t)) and np.abs(t).max() < 2.0 ** 53):
                return False
        S = L // p["step"]
        if S and not ((y * y)[:S * p["step"]].reshape(S, p["step"]).sum(1) < 2.0 ** 24).all():
            return False
    for v in (p["abs_sum"], p["rel_ratio"], p["target_ms"], p["ceiling"]):
        m, _ = np.frexp(v)
        if m * 2.0 ** 24 != np.rint(m * 2.0 ** 24):        # dyadic with a short mantissa
            return False
    return True


# ------------------------------------------------------------------------------------ random problem
def random_problem(seed=7, sr=22050, seconds=1.5):
    """(x [4, n] f32, lens): Gaussian noise at 22.05 kHz.  Utterance 0 is level throughout; 1 has a
    second half 20 dB down (the relative gate drops it); 2 ends in a tail near -80 LKFS (the absolute
    gate drops it) and is shorter; 3 is quiet but for one sample at 0.9, so the peak ceiling sets its gain."""
    rng = np.random.default_rng(seed)
    n = int(sr * seconds) + 37
    x = rng.normal(size=(4, n))
    x[0] *= 0.05
    x[1] *= 0.1 * np.where(np.arange(n) < n // 2, 1.0, 0.1)
    x[2] *= np.where(np.arange(n) < n // 3, 0.02, 3e-5)
    x[3] *= 0.02
    x[3, 5000] = 0.9
    lens = [n, n - 1000, n - 4321, n - 3]
    return x.astype(np.float32), lens


def threshold_distance(res, abs_sum, rel_ratio):
    """The smallest relative distance of a block from the absolute and from the relative threshold."""
    da, dr = np.inf, np.inf
    for (E, pa, both), ms in zip(res["gates"], res["ms"]):
        if len(E):
            da = min(da, float(np.abs(E / abs_sum - 1.0).min()))
        if pa.any():
            thr = rel_ratio * seq_sum(E[pa]) / int(pa.sum())
            dr = min(dr, float(np.abs(E / thr - 1.0).min()))
    return da, dr
