"""float64 numpy reference of tt2_trim (include/tt2_capi.h has the definition), the exactness
predicate, the problem set and the judge of tests/test_gpu_trim_kernels.py, and the mutants that
tests/test_trim_refs.py holds the judge against.  No GPU, no torch.

reference(): block sums, frame energies as sums of 2r block sums, the strict relative threshold,
start / end with `keep` clamped into the utterance, the copy with a zeroed tail.  brute() evaluates
the same definition frame by frame on an explicitly zero-padded copy; by_convolve() gets the
energies from np.convolve of the squared signal with a box.

Exact problems: samples are integers in [-3, 3], so every square is an integer <= 9 and every partial
sum of a frame, in any order, a non-negative integer below 2^24 (exact() asserts it, and that
ratio * emax is an f32 value): the f32 energies, the threshold and with them every output bit are
then defined by the definition whatever order a block is summed in.

The random problem's bound: a frame energy is a sum of `frame` = 2 r hop non-negative terms x^2, each
rounded once (relative 2^-24), added in some order by f32 additions (each relative 2^-24 of a partial
sum that never exceeds the total, the terms being >= 0).  Sequentially that is at most
(frame - 1 + 1) 2^-24 sum x^2 to first order, and any tree is below the sequential figure, so
E[f] = frame 2^-24 sum x^2 covers every order."""
import numpy as np

MAX_R = 16
GEOMETRIES = [(1, 1), (4, 1), (4, 3), (256, 2), (512, 2), (3, 16)]     # (hop, r)
MUTANTS = ["nonstrict", "uncentred", "end_no_plus1", "keep_unclamped_0", "keep_unclamped_len",
           "emax_ignores_len", "emax_other_utterance", "ratio_amplitude", "f0_f1_swapped",
           "second_island_dropped", "partial_block_ignored", "F_ceil", "out_lens_unclamped",
           "tail_not_zeroed", "copy_ignores_keep"]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def clamp_len(v, n_in):
    return n_in if v is None else min(max(int(v), 0), n_in)


def n_frames(length, hop):
    return 0 if length == 0 else 1 + length // hop


def block_sums(x, length, hop):
    """float64 sums of x^2 over the blocks [j hop, (j + 1) hop) within [0, length)."""
    sq = np.asarray(x[:length], dtype=np.float64) ** 2
    nblk = -(-length // hop)
    return np.array([sq[j * hop:(j + 1) * hop].sum() for j in range(nblk)], dtype=np.float64)


def frame_energies(x, length, hop, r):
    """e[f], f < F: the sum of the block sums f - r .. f + r - 1 that exist."""
    bs = block_sums(x, length, hop)
    F = n_frames(length, hop)
    return np.array([bs[max(f - r, 0):min(f + r, len(bs))].sum() for f in range(F)], dtype=np.float64)


def decide(e, length, hop, keep, ratio):
    """(start, end) of the rule on the energies e[0 .. F).  On float32 energies (a kernel's own) the
    threshold is the f32 product the definition names; on float64 energies ratio (an f32 value) times
    emax in float64, which is the same number wherever that product is exact."""
    if len(e) == 0:
        return 0, 0
    e = np.asarray(e)
    if e.dtype == np.float32:
        thr = np.float32(ratio) * e.max()
    else:
        thr = float(np.float32(ratio)) * float(e.max())
    loud = np.nonzero(e > thr)[0]
    if len(loud) == 0:
        return 0, 0
    f0, f1 = int(loud[0]), int(loud[-1])
    return max(0, f0 * hop - keep), min(length, (f1 + 1) * hop + keep)


def copy_out(x, start, end, n_out):
    out = min(end - start, n_out)
    y = np.zeros(n_out, dtype=np.float64)
    y[:out] = x[start:start + out]
    return y, out


def reference(x, lens, hop, r, keep, ratio, n_out, energies=None):
    """(y [B, n_out] float64, out_lens, start, energy [B, n_in // hop + 1] float64) of the definition.
    x [B, n_in]; lens a list as passed to the kernel (unclamped) or None.  energies: per-utterance
    energies to decide on instead of the reference's own (a kernel's, as float32)."""
    x = np.asarray(x)
    B, n_in = x.shape
    nf = n_in // hop + 1
    y = np.zeros((B, n_out))
    en = np.zeros((B, nf))
    outs, starts = [], []
    for b in range(B):
        L = clamp_len(None if lens is None else lens[b], n_in)
        e = frame_energies(x[b], L, hop, r)
        en[b, :len(e)] = e
        s, t = decide(e if energies is None else np.asarray(energies[b])[:len(e)], L, hop, keep, ratio)
        y[b], out = copy_out(x[b], s, t, n_out)
        outs.append(out)
        starts.append(s)
    return y, outs, starts, en


def brute(x, length, hop, r, keep, ratio, n_out):
    """One utterance straight from the definition: per-frame slices of a zero-padded copy."""
    half = r * hop
    pad = np.zeros(length + 2 * half)
    pad[half:half + length] = np.asarray(x[:length], dtype=np.float64)
    F = n_frames(length, hop)
    e = np.array([np.sum(pad[f * hop:f * hop + 2 * half] ** 2) for f in range(F)])
    start = end = 0
    if F and (e > float(np.float32(ratio)) * e.max()).any():
        loud = [f for f in range(F) if e[f] > float(np.float32(ratio)) * e.max()]
        start = max(0, min(loud) * hop - keep)
        end = min(length, (max(loud) + 1) * hop + keep)
    out = min(end - start, n_out)
    y = np.zeros(n_out)
    for i in range(out):
        y[i] = x[start + i]
    return y, out, start, e


def by_convolve(x, length, hop, r):
    """Frame energies as samples of the squared signal convolved with a box of 2 r hop ones."""
    F = n_frames(length, hop)
    if F == 0:
        return np.zeros(0)
    sq = np.asarray(x[:length], dtype=np.float64) ** 2
    full = np.convolve(sq, np.ones(2 * r * hop))       # full[k] = sum sq[k - 2rh + 1 .. k]
    # frame f covers [f hop - r hop, f hop + r hop): k = f hop + r hop - 1
    k = np.arange(F) * hop + r * hop - 1
    return np.where(k < len(full), full[np.minimum(k, len(full) - 1)], sq.sum())


def exact(x, hop, r, ratio, lens=None):
    """Every square, block sum, frame sum (in any order) and ratio * emax is an exact f32 value."""
    x = np.asarray(x, dtype=np.float64)
    B, n_in = x.shape
    for b in range(B):
        L = clamp_len(None if lens is None else lens[b], n_in)
        sq = x[b, :L] ** 2
        if not (np.array_equal(sq, np.rint(sq)) and np.array_equal(sq, sq.astype(np.float32).astype(np.float64))):
            return False
        e = frame_energies(x[b], L, hop, r)
        if len(e) == 0:
            continue
        # non-negative integers with a total below 2^24: every partial sum in any order is exact
        if e.max() >= 2 ** 24:
            return False
        thr = float(np.float32(ratio)) * float(e.max())
        if float(np.float32(thr)) != thr:
            return False
    return True


def judge(got, want, nf=None):
    """The fields of (y, out_lens, start, energy) in which `got` differs from `want` in any bit
    (empty: accepted).  A None energy in `got` is not compared."""
    bad = []
    gy, gl, gs, ge = got
    wy, wl, ws, we = want
    if not (np.shape(gy) == np.shape(wy) and np.array_equal(bits(gy), bits(wy))):
        bad.append("y")
    if [int(v) for v in gl] != [int(v) for v in wl]:
        bad.append("out_lens")
    if [int(v) for v in gs] != [int(v) for v in ws]:
        bad.append("start")
    if ge is not None:
        nf = np.shape(we)[1] if nf is None else nf
        if not np.array_equal(bits(np.asarray(ge)[:, :nf]), bits(np.asarray(we)[:, :nf])):
            bad.append("energy")
    return bad


# ------------------------------------------------------------------ the exact problem set
def _signed(rng, n, amp):
    return (amp * rng.choice([-1, 1], size=n)).astype(np.float32)


def exact_batch(hop, r, seed=0):
    """(x [B, n_in] float32 integers in [-3, 3], lens as passed, row names) for one geometry.  x is
    meaningful (random, loud) also past each utterance's length: the device copy is NaN there, and a
    mutant that reads it shows.  n_in = 8 frames + hop // 2 + 1 is no multiple of hop (hop > 1)."""
    rng = np.random.default_rng(1000 * hop + r + seed)
    frame = 2 * r * hop
    n_in = 8 * frame + hop // 2 + 1
    rows, lens, names = [], [], []

    def add(name, length, segs=None):
        row = _signed(rng, n_in, 3)                      # loud everywhere, overwritten inside the utterance
        L = clamp_len(length, n_in)
        if segs is None:
            row[:L] = rng.integers(-3, 4, size=L).astype(np.float32)
        else:
            row[:L] = 0
            for lo, hi, amp in segs:
                lo, hi = max(lo, 0), min(hi, L)
                if hi > lo:
                    row[lo:hi] = _signed(rng, hi - lo, amp)
        rows.append(row), lens.append(length), names.append(name)

    for L in (0, 1, hop - 1, hop, hop + 1, r * hop - 1, r * hop + 1):
        add(f"short{L}", L)
    N = n_in
    add("at_0", N, [(0, frame, 3)])
    add("at_end", N, [(N - frame, N, 3), (0, N - frame, 1)])
    # two impulses frame - 1 apart: one frame holds both (18), its neighbours one (9); at ratio 1/2 the
    # nines sit exactly on the threshold and only frame k + r is loud
    k = 3 * r
    add("single_frame", N, [(k * hop, k * hop + 1, 3), (k * hop + frame - 1, k * hop + frame, 3)])
    add("none", N, [])
    add("all", N, [(0, N, 3)])
    add("all_above_n_in", N + 7, [(0, N, 2)])
    add("negative_len", -2)
    add("islands", N - hop - 1, [(frame + hop // 2, 2 * frame, 3), (5 * frame, 6 * frame + 1, 2)])
    # a stretch of ones whose inner frames are exactly 1/4 of a frame of twos: silent at ratio 1/4
    add("threshold", N - 1, [(0, 2 * frame + hop, 1), (4 * frame, 6 * frame, 2)])
    add("islands_in_noise", N, [(0, N, 1), (2 * frame + 1, 3 * frame, 3), (6 * frame - 1, 7 * frame - hop, 3)])
    return np.stack(rows), lens, names


def exact_problems():
    """Every exact call of the GPU test: dicts of x, lens, hop, r, keep, ratio, n_out, names."""
    out = []
    for hop, r in GEOMETRIES:
        x, lens, names = exact_batch(hop, r)
        n_in = x.shape[1]
        frame = 2 * r * hop
        combos = [(keep, ratio) for ratio in (2.0 ** -3, 2.0 ** -2, 2.0 ** -1)
                  for keep in (0, 1, 3 * frame, 10 * n_in)]
        for i, (keep, ratio) in enumerate(combos):
            _, outs, _, _ = reference(x, lens, hop, r, keep, ratio, n_in + 5)
            longest = max(outs)
            n_out = [max(longest - 3, 1), max(longest, 1), n_in + 5][i % 3]
            out.append(dict(x=x, lens=lens, hop=hop, r=r, keep=keep, ratio=ratio, n_out=n_out, names=names))
    return out


# ------------------------------------------------------------------ mutants
def mutant(name, x, lens, hop, r, keep, ratio, n_out):
    """What a kernel with one named mistake would return: (y, out_lens, start, energy)."""
    x = np.asarray(x)
    B, n_in = x.shape
    nf = n_in // hop + 1
    y = np.zeros((B, n_out))
    en = np.zeros((B, nf))
    outs, starts = [], []
    ratio64 = float(np.float32(ratio))
    all_e = []
    for b in range(B):
        L = clamp_len(lens[b], n_in)
        F = -(-L // hop) if name == "F_ceil" else n_frames(L, hop)
        if name == "uncentred":
            sq = np.concatenate([np.asarray(x[b, :L], dtype=np.float64) ** 2, np.zeros(2 * r * hop + hop)])
            e = np.array([sq[f * hop:f * hop + 2 * r * hop].sum() for f in range(F)])
        elif name == "partial_block_ignored":
            bs = block_sums(x[b], L - L % hop, hop)
            e = np.array([bs[max(f - r, 0):min(f + r, len(bs))].sum() for f in range(F)])
        else:
            e = frame_energies(x[b], L, hop, r)[:F]
        all_e.append(e)
    for b in range(B):
        L = clamp_len(lens[b], n_in)
        e = all_e[b]
        en[b, :len(e)] = e
        start = end = src = 0
        if len(e):
            emax = e.max()
            if name == "emax_ignores_len":
                emax = frame_energies(x[b], n_in, hop, r).max()
            if name == "emax_other_utterance":
                emax = max(v.max() for v in all_e if len(v))
            thr = (np.sqrt(ratio64) if name == "ratio_amplitude" else ratio64) * emax
            loud = np.nonzero(e >= thr if name == "nonstrict" else e > thr)[0]
            if len(loud):
                f0, f1 = int(loud[0]), int(loud[-1])
                if name == "second_island_dropped":
                    run = np.nonzero(np.diff(loud) > 1)[0]
                    f1 = int(loud[run[0]]) if len(run) else f1
                if name == "f0_f1_swapped":
                    f0, f1 = f1, f0
                start = f0 * hop - keep
                if name != "keep_unclamped_0":
                    start = max(0, start)
                end = (f1 + (0 if name == "end_no_plus1" else 1)) * hop + keep
                if name != "keep_unclamped_len":
                    end = min(L, end)
                src = f0 * hop if name == "copy_ignores_keep" else start
        full = max(end - start, 0)
        out = min(full, n_out)
        wide = np.concatenate([np.zeros(n_in + keep + 1), np.asarray(x[b], dtype=np.float64), np.zeros(n_out + keep + 1)])
        y[b, :out] = wide[n_in + keep + 1 + src:n_in + keep + 1 + src + out]
        if name == "tail_not_zeroed":
            y[b, out:] = np.nan
        outs.append(full if name == "out_lens_unclamped" else out)
        starts.append(start)
    return y, outs, starts, en


# ------------------------------------------------------------------ the random problem
def random_problem(hop, r, n_in, seed):
    """Gaussian noise under a stepped envelope of 40 dB steps (amplitude 1 or 0.01), the steps half a
    hop off the frame grid: (x [4, n_in] float32, lens).  At top_db = 30 no frame comes near the
    threshold (decision_margin)."""
    rng = np.random.default_rng(seed)
    frame = 2 * r * hop
    x = rng.normal(size=(4, n_in))
    env = np.full((4, n_in), 0.01)
    h = hop // 2
    env[0, 3 * frame + h:n_in - 2 * frame - h] = 1.0                       # one loud stretch
    env[1, 2 * frame + h:4 * frame + h] = 1.0                               # two, interior silence
    env[1, 7 * frame + h:9 * frame + h] = 1.0
    env[2, :5 * frame + h] = 1.0                                            # loud from sample 0
    env[3, 4 * frame + h:] = 1.0                                            # loud to the end
    lens = [n_in, n_in - frame - 3, n_in - 1, n_in - hop - 7]
    return (0.3 * x * env).astype(np.float32), lens


def energy_bound(x, length, hop, r):
    """E[f] = frame 2^-24 sum x^2 (the module docstring derives it)."""
    return 2 * r * hop * 2.0 ** -24 * frame_energies(x, length, hop, r)


def decision_margin(x, length, hop, r, ratio):
    """min over frames of (|e[f] - thr| - slack[f]) / thr, with slack the most an energy and the
    threshold can both move under energy_bound (thr moves by ratio E[fmax], plus 2^-23 thr for the
    f32 product): positive means every f32 evaluation within the bound takes the float64 decision."""
    e = frame_energies(x, length, hop, r)
    E = energy_bound(x, length, hop, r)
    ratio64 = float(np.float32(ratio))
    thr = ratio64 * e.max()
    slack = E + ratio64 * E.max() + 2.0 ** -23 * thr
    return float(((np.abs(e - thr) - slack) / thr).min())
