"""References, mutants and problem sets of the length regulator (csrc/regulate.hip; include/tt2_capi.h
has the definition).  Everything here is numpy and plain Python: no GPU, no torch.

* plan_ref: the plan in Python integers (ends, index, frames, total).
* fwd_ref: the expansion, a row copy of bits.
* bwd_model: the segment sum in numpy float32, one add per frame in ascending frame order, rounded
  once to bf16 (integer bit operations) for a bf16 output.  The kernel must match it bit for bit on
  ANY input: there is no tolerance anywhere in this feature.  bwd_f64 is the float64 sum, for
  information only.
* mutants: the reference with one mistake each (MUTANTS); reject() is the bar the GPU tests apply
  (bit equality of every output), and test_regulate_refs.py shows that it rejects each of them on the
  problem sets the GPU tests run.
* plan_problems, layout, fwd_problem, bwd_exact_problem, bwd_mixed_problem: those problem sets, shared by the CPU and the GPU tests.

bf16 tensors are uint16 arrays of bits, f32 tensors float32 arrays; compare through bits()."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
INT32_MIN = -2 ** 31
MAX_PHONEMES = 4096
HUGE = INT32_MAX                 # what durations hold at and past key_len[b]: never to be read

PLAN_MUTANTS = ["ends off by one", "highest t at zero durations", "negatives not clamped", "key_len ignored",
                "no clamp at n_out", "32-bit wrap", "no -1 fill"]
BWD_MUTANTS = ["descending", "pairwise", "bf16 after every add", "rows past Tx_b unwritten", "dy read past frames"]
MUTANTS = PLAN_MUTANTS + BWD_MUTANTS
POISON = -77                     # what an output that a mutant leaves unwritten holds


def clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def wrap32(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


# ------------------------------------------------------------------------------------------- plan
def plan_ref(durations, key_len, tx, n_out, mut=None):
    """durations: B rows of at least tx integers; key_len: B integers or None.  Returns a dict of
    int32 arrays: ends [B, tx], index [B, n_out], frames [B], total [B]."""
    B = len(durations)
    ends = np.zeros((B, tx), dtype=np.int32)
    index = np.full((B, n_out), -1, dtype=np.int32)
    frames = np.zeros(B, dtype=np.int32)
    total = np.zeros(B, dtype=np.int32)
    for b in range(B):
        txb = tx if key_len is None or mut == "key_len ignored" else clamp(key_len[b], 0, tx)
        S, run = [], 0
        for t in range(tx):
            d = int(durations[b][t]) if t < txb else 0
            if mut != "negatives not clamped":
                d = max(d, 0)
            run += d
            if mut == "32-bit wrap":
                run = wrap32(run)
            S.append(run)
        if mut == "ends off by one" and tx:           # the exclusive sum in place of the inclusive one
            S = [0] + S[:-1]
        cap = INT32_MAX if mut == "no clamp at n_out" else n_out
        e = [clamp(s, INT32_MIN, cap) for s in S]
        ends[b] = e
        frames[b] = e[-1] if tx else 0
        total[b] = clamp(S[-1], INT32_MIN, INT32_MAX) if tx else 0
        t = 0
        for n in range(n_out):
            if n >= frames[b]:
                if mut == "no -1 fill":
                    index[b, n] = POISON
                continue
            while t < tx - 1 and e[t] <= n:
                t += 1
            index[b, n] = t
            if mut == "highest t at zero durations":
                index[b, n] = _highest_start(e, n, tx)
    return {"ends": ends, "index": index, "frames": frames, "total": total}


def _highest_start(e, n, tx):
    """What a search from the wrong side returns: the owner of frame n, then on over the phonemes of
    zero duration that follow it (they end where it ends)."""
    t = 0
    while t < tx - 1 and e[t] <= n:
        t += 1
    while t + 1 < tx and e[t + 1] == e[t]:
        t += 1
    return t


def plan_brute(durations, key_len, tx, n_out):
    """np.repeat per utterance: the textbook length regulator, for test_regulate_refs.py."""
    B = len(durations)
    index = np.full((B, n_out), -1, dtype=np.int32)
    frames, total = [], []
    for b in range(B):
        txb = tx if key_len is None else clamp(key_len[b], 0, tx)
        d = np.array([max(int(v), 0) for v in durations[b][:txb]], dtype=object)
        tot = int(d.sum()) if txb else 0
        total.append(min(tot, INT32_MAX))
        frames.append(min(tot, n_out))
        seq = []
        for t in range(txb):                      # np.repeat would materialise 2^31 entries
            if len(seq) >= n_out:
                break
            seq.extend([t] * min(int(d[t]), n_out - len(seq)))
        index[b, :len(seq)] = seq
    return index, frames, total


# ---------------------------------------------------------------------------------------- forward
def bits(x):
    """An integer view that compares -0, NaN payloads and all."""
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def fwd_ref(h, index, tx):
    """h [B, >= tx, D] (float32, or uint16 bf16 bits), index [B, n_out] -> y [B, n_out, D]: rows copied,
    zeros where the index is outside [0, tx)."""
    hb = bits(h)
    B, n_out = index.shape
    y = np.zeros((B, n_out, h.shape[2]), dtype=hb.dtype)
    for b in range(B):
        ok = (index[b] >= 0) & (index[b] < tx)
        y[b, ok] = hb[b, index[b, ok]]
    return y.view(h.dtype)


# --------------------------------------------------------------------------------------- backward
def bf16_to_f32(u):
    return (np.asarray(u, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16(x):
    """Round to nearest, ties to even, in integer arithmetic (NaN stays a quiet NaN)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u >> 16) | 0x40, r)
    return r.astype(np.uint16)


def _as_f32(x):
    return x if x.dtype == np.float32 else bf16_to_f32(x)


def _sum_f32(rows, order):
    """rows [k, D] float32 -> [D] float32, from +0, one f32 add per row."""
    acc = np.zeros(rows.shape[1], dtype=np.float32)
    if order == "pairwise":
        if len(rows) == 0:
            return acc
        if len(rows) == 1:
            return acc + rows[0]
        m = len(rows) // 2
        return _sum_f32(rows[:m], order) + _sum_f32(rows[m:], order)
    seq = rows[::-1] if order == "descending" else rows
    for r in seq:
        acc = acc + r
        if order == "bf16 after every add":
            acc = bf16_to_f32(f32_to_bf16(acc))
    return acc


def bwd_model(dy, ends, n_out, mut=None, key_len=None, raw=False):
    """dy [B, >= n_out, D] (float32 or bf16 bits), ends [B, tx] -> dh [B, tx, D] of dy's dtype: the
    float32 model of tt2_regulate_bwd.  key_len only serves the mutant that leaves rows unwritten;
    raw=True returns the float32 accumulators before the rounding to bf16."""
    x = _as_f32(dy)
    B, tx = ends.shape
    out = np.zeros((B, tx, dy.shape[2]), dtype=np.float32)
    order = mut if mut in ("descending", "pairwise", "bf16 after every add") else "ascending"
    for b in range(B):
        for t in range(tx):
            s = clamp(ends[b, t - 1], 0, n_out) if t else 0
            e = clamp(ends[b, t], 0, n_out)
            if mut == "dy read past frames" and t == tx - 1:
                e = n_out                              # the last segment taken to the end of the buffer
            out[b, t] = _sum_f32(x[b, s:max(e, s)], order)
            if mut == "rows past Tx_b unwritten" and key_len is not None and t >= clamp(key_len[b], 0, tx):
                out[b, t] = POISON
    return out if raw or dy.dtype == np.float32 else f32_to_bf16(out)


def bwd_f64(dy, ends, n_out):
    x = _as_f32(dy).astype(np.float64)
    B, tx = ends.shape
    out = np.zeros((B, tx, dy.shape[2]))
    for b in range(B):
        for t in range(tx):
            s = clamp(ends[b, t - 1], 0, n_out) if t else 0
            out[b, t] = x[b, s:max(clamp(ends[b, t], 0, n_out), s)].sum(axis=0)
    return out


def reject(got, want):
    """The bar of every GPU test: the names of the outputs that differ in any bit."""
    bad = []
    for k in want:
        g, w = bits(np.asarray(got[k])), bits(np.asarray(want[k]))
        if g.shape != w.shape or g.dtype != w.dtype or not np.array_equal(g, w):
            bad.append(k)
    return bad


# ---------------------------------------------------------------------------------- plan problems
PLAN_TX = [0, 1, 2, 63, 64, 65, 257, 4096]
PLAN_NOUT = [0, 1, 37, 257, 1030]


def _spread(rng, tx, total, lo_frac=0.0, hi_frac=1.0):
    """tx integers >= 0 with the given sum, about half of them zero, all zero outside
    [lo_frac, hi_frac) of the range (so: runs of zeros at both ends)."""
    d = np.zeros(tx, dtype=np.int64)
    lo, hi = int(tx * lo_frac), max(int(tx * hi_frac), int(tx * lo_frac) + 1)
    live = np.arange(lo, min(hi, tx))
    if tx == 0 or total <= 0 or len(live) == 0:
        return d
    live = live[rng.random(len(live)) < 0.5] if len(live) > 1 else live
    if len(live) == 0:
        live = np.array([lo])
    d[live] = rng.multinomial(total, np.full(len(live), 1.0 / len(live)))
    return d


def plan_rows(tx, n_out, seed=0):
    """The rows a (tx, n_out) plan case is made of: name -> (durations [tx], key_len)."""
    rng = np.random.default_rng(1000 * tx + n_out + seed)
    rows = {}
    rows["exact"] = (_spread(rng, tx, n_out), tx + 3)                        # the total exactly n_out
    rows["below"] = (_spread(rng, tx, n_out - 1, 0.25, 0.75), tx)            # one below, zeros at both ends
    d = _spread(rng, tx, n_out + 1)                                          # one above, with negatives
    zero = np.nonzero(d == 0)[0]
    d[zero[::2]] = -rng.integers(1, 6, size=len(zero[::2]))
    if len(zero):
        d[zero[0]] = INT32_MIN
    rows["above"] = (d, tx)
    d = np.zeros(tx, dtype=np.int64)                                         # the seams of any block scan
    d[::64], d[::256], d[::1024] = 1, 2, 3
    if tx:
        d[tx - 1] += 1
    rows["seams"] = (d, tx + 1)
    d = _spread(rng, tx, 5)
    if tx:
        d[0] = d[tx - 1] = INT32_MAX                                         # tx = 1: one of them
        d[tx // 2] = INT32_MAX
    rows["huge"] = (d, tx)
    rows["mid"] = (_spread(rng, tx, n_out + 7), tx // 2)
    rows["klen0"] = (_spread(rng, tx, n_out), 0)
    rows["kneg"] = (_spread(rng, tx, n_out), -5)
    rows["ones"] = (np.ones(tx, dtype=np.int64), tx)
    out = {}
    for name, (d, k) in rows.items():
        d = d.copy()
        d[clamp(k, 0, tx):] = HUGE                                           # never to be read
        out[name] = (d, k)
    return out


PLAN_BATCHES = [("exact", "below", "above", "seams"), ("huge", "mid", "klen0", "kneg"),
                ("kneg", "ones", "exact", "mid"), ("above", "huge", "seams", "klen0")]


def plan_problems(tx, n_out):
    """B = 4 problems with a different case in every row, the same rows at different batch positions,
    and one problem without key_len (rows whose key_len is >= tx anyway)."""
    rows = plan_rows(tx, n_out)
    probs = []
    for names in PLAN_BATCHES:
        d = np.stack([rows[n][0] for n in names]).astype(np.int64).reshape(len(names), tx)
        probs.append({"names": names, "durations": d, "key_len": [rows[n][1] for n in names], "tx": tx, "n_out": n_out})
    first = dict(probs[0])
    first["key_len"] = None
    first["durations"] = np.where(first["durations"] == HUGE, 0, first["durations"]) if tx else first["durations"]
    probs.append(first)
    return probs


# ------------------------------------------------------------------------ forward / backward problems
DIMS = [1, 3, 7, 8, 260, 512]
LAYOUTS = {
    # tx, n_out, durations per utterance, key_len.  "long" has one phoneme of 1030 frames; "many" more
    # phonemes than any one work group takes and two work groups' worth of frames at every dim
    "long": dict(tx=9, n_out=1100, key_len=[9, 6, 12, 0],
                 durations=[[0, 3, 1030, 0, 0, 1, 17, 2, 0], [2, 0, 0, 40, 1, 5, 900, 900, 900],
                            [30, 1030, 50, 0, 7, 1, 0, 2, 1], [4, 4, 4, 4, 4, 4, 4, 4, 4]]),
    "many": dict(tx=300, n_out=1101, key_len=[300, 257, 300, -1], durations=None),
}


def layout(name):
    """-> dict(tx, n_out, durations [B, tx] int64, key_len, plan)."""
    L = dict(LAYOUTS[name])
    if L["durations"] is None:
        rng = np.random.default_rng(7)
        d = rng.integers(0, 8, size=(4, L["tx"])) * (rng.random((4, L["tx"])) < 0.7)
        d[2, 100] = 400                                   # row 2 is cut at n_out
        L["durations"] = d
    L["durations"] = np.array(L["durations"], dtype=np.int64)
    for b, k in enumerate(L["key_len"]):
        L["durations"][b, clamp(k, 0, L["tx"]):] = HUGE
    L["plan"] = plan_ref(L["durations"], L["key_len"], L["tx"], L["n_out"])
    return L


def _from_f32(x, dtype):
    return x.astype(np.float32) if dtype == "f32" else f32_to_bf16(x)


def _nan(shape, dtype):
    return np.full(shape, np.nan, dtype=np.float32) if dtype == "f32" else np.full(shape, 0x7FC1, dtype=np.uint16)


SPECIALS = {"f32": np.array([0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x807FFFFF], dtype=np.uint32).view(np.float32),
            "bf16": np.array([0x8000, 0x0001, 0x7F80, 0xFF80, 0x807F], dtype=np.uint16)}


def fwd_problem(L, dim, dtype, seed=0):
    """h [B, tx, dim]: random values, -0 / denormals / infinities in column 0 of the rows that frames
    name, NaN in every row that no frame names."""
    rng = np.random.default_rng(seed + dim)
    B, tx = L["durations"].shape
    h = _from_f32(rng.normal(size=(B, tx, dim)), dtype)
    sp = SPECIALS[dtype]
    for b in range(B):
        named = set(int(i) for i in L["plan"]["index"][b] if i >= 0)
        for t in range(tx):
            if t in named:
                h[b, t, 0] = sp[(b + t) % len(sp)]
            else:
                h[b, t] = _nan(dim, dtype)
    return h


def bwd_exact_problem(L, dim, dtype, seed=0):
    """dy [B, n_out, dim] of -1 / 0 / 1 (so every partial sum is a small integer), NaN at and past
    frames[b]."""
    rng = np.random.default_rng(seed + 3 * dim)
    B, n_out = len(L["durations"]), L["n_out"]
    dy = _from_f32(rng.integers(-1, 2, size=(B, n_out, dim)).astype(np.float32), dtype)
    for b in range(B):
        dy[b, L["plan"]["frames"][b]:] = _nan(dim, dtype)
    return dy


def is_exact(dy, ends, n_out, dtype):
    """The premise of an exact problem: integer values whose segment sums (hence every partial sum,
    for values in {-1, 0, 1}... bounded by the count) stay within 2^24 for f32 and 256 for a bf16
    output, where every integer is representable."""
    x = _as_f32(dy)
    B, tx = ends.shape
    bound = 2 ** 24 if dtype == "f32" else 256
    for b in range(B):
        fr = clamp(ends[b, tx - 1], 0, n_out) if tx else 0
        v = x[b, :fr].astype(np.float64)
        if not np.array_equal(v, np.rint(v)):
            return False
        prev = 0
        for t in range(tx):
            e = clamp(ends[b, t], 0, n_out)
            if e > prev and np.abs(np.cumsum(v[prev:e], axis=0)).max() > bound:
                return False
            prev = max(prev, e)
    return True


def bwd_mixed_problem(L, dim, dtype, seed=0):
    """dy of widely mixed magnitude (2^-12 .. 2^12 times a random mantissa, random sign): the order
    of the adds shows in the low bits.  NaN at and past frames[b]."""
    rng = np.random.default_rng(seed + 5 * dim + 1)
    B, n_out = len(L["durations"]), L["n_out"]
    x = rng.normal(size=(B, n_out, dim)) * 2.0 ** rng.integers(-12, 13, size=(B, n_out, dim))
    dy = _from_f32(x, dtype)
    for b in range(B):
        dy[b, L["plan"]["frames"][b]:] = _nan(dim, dtype)
    return dy


def order_sensitive(dy, ends, n_out):
    """True where ascending, descending and pairwise float32 sums give three different results (the
    accumulators: with few elements a bf16 rounding can hide the difference)."""
    a = bits(bwd_model(dy, ends, n_out, raw=True))
    d = bits(bwd_model(dy, ends, n_out, mut="descending", raw=True))
    p = bits(bwd_model(dy, ends, n_out, mut="pairwise", raw=True))
    return not np.array_equal(a, d) and not np.array_equal(a, p) and not np.array_equal(d, p)
