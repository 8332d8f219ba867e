"""References, mutants, bars and problem sets of Gaussian upsampling (csrc/upsample.hip;
include/tt2_capi.h has the definition).  Everything here is numpy: no GPU, no torch.

* evaluate(p): the forward (y, lse) and the four gradients (dh, dcenter, dprec, dbias) of a problem,
  per utterance, in the dtype asked for.  float64 is the reference; float32 (float32_evaluations: two
  accumulation orders) is the yardstick of the f32 kernels; with twin=True it is the bf16-rounding
  twin in the manner of _attn_refs.py: float64 arithmetic with the roundings the bf16 data path
  cannot avoid -- the weights of the forward product and of the dh product rounded to bf16, y rounded
  to bf16 and read back rounded by delta, dh rounded to bf16.  The twin is the yardstick of the bf16
  kernels, except for lse, which no bf16 value enters: there it is the float32 evaluation.
* MUTANTS: the reference with one mistake each, over every row or (confine=True) over the rows of
  one 32-row tile only (the one that holds an interior length); judge() is the bar the GPU tests apply, and test_upsample_refs.py shows that it
  rejects each of them.
* judge(): per frame row (y, lse) and per phoneme (dh row, dcenter, dprec, dbias), the error against
  float64 over max(4 x the yardstick's own error on that row, 2 ulp of the row's scale), <= 1 passes;
  the yardstick's error on a row counts as no less than its RMS error relative to scale over the
  utterance's rows times the row's scale (one evaluation is one draw, and a row can be one number).
  The error of a row is its L2 norm.  The scale of a row is the magnitude of what is summed into it
  (scales()): sum_t W |h| for y, sum_n W |dy| for dh, sum_n |W| (|dW| + |delta|) times the factor of
  the output for the three per-phoneme sums, max(|lse|, 1) for lse.  The ulp is that of the output's
  dtype: bf16 for y and dh of a bf16 problem, f32 for everything else.  One allowance beyond that
  bar, absolute and tiny: the GPU's exponential and its f32 arithmetic flush results below 2^-126 (the
  smallest normal float32) to zero where numpy keeps denormals, so each weight may be off by
  FTZ = 2^-126 and each output by as much again; a row may therefore miss by FTZ times what its
  weights multiply (tiny(): sum_t |h| for y, sum_n |dy| for dh, sum_n (|dW| + |delta|) |factor| for
  the sums) plus FTZ per element.  It matters only for rows whose every weight is below ~1e-30 (a
  phoneme tens of frames away from every live frame); test_upsample_refs.py measures it against the
  float32 reference with its weights flushed, not against a kernel.  The padding (y and lse at and
  past Ty_b, every gradient at and past Tx_b) must be exactly +0.
* selector_problem / uniform_problem: the exact problems, compared bit for bit; exact_outputs() says
  which outputs of a problem are order-independent in float32 (every summand a multiple of one
  quantum, the sum of magnitudes below 2^24 quanta) and therefore must match to the bit.
* espnet_problem / mix_problem: the random problems.

A problem is a dict: h [B, tx, dim] and dy [B, n_out, dim] float64 holding values of `dtype`
("f32" | "bf16"), center / prec / bias [B, tx] float64 holding f32 values (bias may be None), q_len /
key_len (lists, unclamped), offset.  Entries the contract does not read hold finite decoys here (the
mutants read them); the GPU tests upload NaN in their place."""
import numpy as np

SHAPES = [(1, 1, 1), (1, 3, 8), (33, 5, 17), (64, 64, 64), (65, 33, 80), (257, 37, 96), (130, 129, 512)]
# the kernels' tiles: 64 (fwd) and 32 (bwd) frames, 32 phonemes, 128 (fwd work group), 32 (bwd K step)
# and 16 (MFMA) columns, 128 frames (the most one work group of the backward walks before the frames are shared)
# -- the edges +- 1 of each that SHAPES does not already hold, and 2100 frames: more than 64 frame tiles, where a
# work group of the backward walks more than four
EDGE_SHAPES = [(31, 31, 15), (32, 32, 16), (63, 65, 31), (33, 63, 127), (66, 2, 129), (5, 34, 128), (128, 3, 9), (129, 3, 9), (33, 3, 32), (5, 3, 33), (2100, 2, 1)]
OUTPUTS = ("y", "lse", "dh", "dcenter", "dprec", "dbias")
MUTANTS = ["softmax over tx", "offset dropped", "center[t+1]", "bias ignored", "|x - c| for the square",
           "2 prec missing from dcenter", "dprec sign flipped", "delta missing from dE", "delta over n < n_out",
           "rows past Ty_b not zero", "gradients past Tx_b not zero", "dh from dW"]
TILE = 32


def clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def bf16_round(x):
    """float array -> the nearest bf16 values (ties to even), as float64."""
    f = np.ascontiguousarray(x, dtype=np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(x))


def bf16_bits(x):
    """float array of bf16 values -> uint16 bits."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_from_bits(b):
    return (np.ascontiguousarray(b).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def lengths(p):
    B, tx, _ = p["h"].shape
    n_out = p["dy"].shape[1]
    txs = [tx if p["key_len"] is None else clamp(p["key_len"][b], 0, tx) for b in range(B)]
    tys = [n_out if p["q_len"] is None else clamp(p["q_len"][b], 0, n_out) for b in range(B)]
    return txs, tys


FTZ = 2.0 ** -126


def evaluate(p, dt=np.float64, twin=False, mut=None, flip=False, ftz=False, tiled=False, fma=False):
    """-> dict of float64 arrays y [B, n_out, dim], lse [B, n_out], dh [B, tx, dim], dcenter, dprec,
    dbias [B, tx].  dt: the arithmetic; twin: the bf16 roundings (see the module docstring); flip: the
    sums over phonemes, frames and columns in the reverse order (another draw of the float32
    rounding errors); tiled: the sums in the kernels' order -- the forward an online softmax over
    phoneme tiles of 32 (with twin, the weights rounded to bf16 relative to the running maximum), the
    backward over frame blocks of 128 added in ascending order -- a third draw; fma: the score's product and sum rounded once, as a fused multiply-add does (the
    kernels' gu_score), instead of twice -- another draw of e's own rounding, which flip does not redraw; mut: one of MUTANTS; ftz: weights below 2^-126 flushed to zero, as the GPU has
    them."""
    B, tx, dim = p["h"].shape
    n_out = p["dy"].shape[1]
    rw = bf16_round if twin else (lambda v: v)
    out = {"y": np.zeros((B, n_out, dim)), "lse": np.zeros((B, n_out)), "dh": np.zeros((B, tx, dim)),
           "dcenter": np.zeros((B, tx)), "dprec": np.zeros((B, tx)), "dbias": np.zeros((B, tx))}
    txs, tys = lengths(p)
    offset = 0.0 if mut == "offset dropped" else p["offset"]
    for b in range(B):
        txb, tyb = txs[b], tys[b]
        if mut == "softmax over tx":
            txb = tx
        ty_f = n_out if mut == "rows past Ty_b not zero" else tyb         # the forward's rows
        ty_b = n_out if mut == "delta over n < n_out" else tyb            # the backward's rows
        rows = max(ty_f, ty_b)
        if txb == 0 or rows == 0:
            continue
        sl = slice(None, None, -1) if flip else slice(None)
        c = p["center"][b, :txb].astype(dt)
        if mut == "center[t+1]":
            c = np.roll(c, -1)
        pr = p["prec"][b, :txb].astype(dt)
        bi = np.zeros(txb, dtype=dt) if p["bias"] is None or mut == "bias ignored" else p["bias"][b, :txb].astype(dt)
        h = p["h"][b, :txb].astype(dt)
        x = np.arange(rows).astype(dt) + dt(offset)
        d = x[:, None] - c[None, :]
        q = np.abs(d) if mut == "|x - c| for the square" else d * d
        e = bi[None, :] - pr[None, :] * q
        if fma and mut is None:
            e = (bi[None, :].astype(np.float64) - pr[None, :].astype(np.float64) * q.astype(np.float64)).astype(dt)
        m = e.max(axis=1, keepdims=True)
        pe = np.exp(e - m)
        if ftz:
            pe = np.where(pe < FTZ, 0, pe).astype(dt)
        l = pe[:, sl].sum(axis=1, keepdims=True)
        y_acc = (rw(pe).astype(dt)[:, sl] @ h[sl]) / l
        if tiled:
            m_run, l, acc = np.full((rows, 1), -np.inf, dtype=dt), np.zeros((rows, 1), dtype=dt), np.zeros((rows, dim), dtype=dt)
            for t0 in range(0, txb, TILE):
                et = e[:, t0:t0 + TILE]
                mn = np.maximum(m_run, et.max(axis=1, keepdims=True))
                alpha, pt = np.exp(m_run - mn), np.exp(et - mn)
                l = l * alpha + pt.sum(axis=1, keepdims=True)
                acc = acc * alpha + rw(pt).astype(dt) @ h[t0:t0 + TILE]
                m_run = mn
            m, y_acc = m_run, acc / l
        y = rw(y_acc).astype(dt)
        lse = m + np.log(l)
        out["y"][b, :ty_f] = y[:ty_f]
        out["lse"][b, :ty_f] = lse[:ty_f, 0]
        if ty_b == 0:
            continue
        # what the forward left: zeros at and past Ty_b
        ys, ls = y[:ty_b].copy(), lse[:ty_b].copy()
        ys[tyb:], ls[tyb:] = 0, 0
        dy = p["dy"][b, :ty_b].astype(dt)
        W = np.exp(e[:ty_b] - ls)
        if ftz:
            W = np.where(W < FTZ, 0, W).astype(dt)
        delta = (dy * ys)[:, sl].sum(axis=1, keepdims=True)
        if mut == "delta missing from dE":
            delta = np.zeros_like(delta)
        dW = dy[:, sl] @ h[:, sl].T
        dE = W * (dW - delta)
        A = dE if mut == "dh from dW" else rw(W).astype(dt)
        out["dh"][b, :txb] = rw(A.T[:, sl] @ dy[sl])
        out["dbias"][b, :txb] = dE[sl].sum(axis=0)
        if tiled:
            blocks = [slice(f, f + 4 * TILE) for f in range(0, ty_b, 4 * TILE)]
            out["dh"][b, :txb] = rw(sum(A.T[:, k] @ dy[k] for k in blocks))
            out["dbias"][b, :txb] = sum(dE[k].sum(axis=0) for k in blocks)
        fac = d[:ty_b] if mut == "2 prec missing from dcenter" else 2 * pr[None, :] * d[:ty_b]
        out["dcenter"][b, :txb] = (dE * fac)[sl].sum(axis=0)
        sp = (dE * q[:ty_b])[sl].sum(axis=0)
        if tiled:
            out["dcenter"][b, :txb] = sum((dE * fac)[k].sum(axis=0) for k in blocks)
            sp = sum((dE * q[:ty_b])[k].sum(axis=0) for k in blocks)
        out["dprec"][b, :txb] = sp if mut == "dprec sign flipped" else 0 - sp
        if mut == "gradients past Tx_b not zero":
            for k in ("dh", "dcenter", "dprec", "dbias"):
                out[k][b, txs[b]:] = 0.25
    return {k: v.astype(np.float64) for k, v in out.items()}


def confined_tile(rows):
    """The 32-row tile that holds the interior length (rows + 1) // 2 of length_cases: it has live
    rows of one utterance and padding of another."""
    r0 = (rows + 1) // 2 // TILE * TILE
    return r0, r0 + TILE


def mutant(p, name, confine=False):
    """The float64 reference with the mistake `name`, over every row or over one 32-row tile of each
    output's rows only (confined_tile: frames for y and lse, phonemes for the gradients)."""
    good, bad = evaluate(p), evaluate(p, mut=name)
    if not confine:
        return bad
    for k in OUTPUTS:
        r0, r1 = confined_tile(good[k].shape[1])
        good[k][:, r0:r1] = bad[k][:, r0:r1]
    return good


def float32_evaluations(p):
    return [evaluate(p, dt=np.float32), evaluate(p, dt=np.float32, flip=True)]


def yardstick(p):
    """What the kernels of p's dtype are held to: the float32 evaluations, or the bf16 twin.  lse is
    f32 arithmetic on f32 inputs whatever the dtype of h (no bf16 value enters it), so its yardstick is
    the float32 evaluations' in both cases: the twin forms e in float64 and has no error there."""
    f32 = float32_evaluations(p)
    if p["dtype"] == "f32":
        return f32
    twin = evaluate(p, twin=True)
    return [dict(twin, lse=y["lse"]) for y in f32]


def scales(p):
    """The magnitude of what is summed into each row (float64), per output: [B, rows]."""
    B, tx, dim = p["h"].shape
    n_out = p["dy"].shape[1]
    s = {"y": np.zeros((B, n_out)), "lse": np.ones((B, n_out)), "dh": np.zeros((B, tx)),
         "dcenter": np.zeros((B, tx)), "dprec": np.zeros((B, tx)), "dbias": np.zeros((B, tx))}
    ref = evaluate(p)
    txs, tys = lengths(p)
    for b in range(B):
        txb, tyb = txs[b], tys[b]
        if txb == 0 or tyb == 0:
            continue
        c, pr = p["center"][b, :txb], p["prec"][b, :txb]
        bi = np.zeros(txb) if p["bias"] is None else p["bias"][b, :txb]
        h, dy = p["h"][b, :txb], p["dy"][b, :tyb]
        d = (np.arange(tyb) + p["offset"])[:, None] - c[None, :]
        q = d * d
        W = np.exp(bi[None, :] - pr[None, :] * q - ref["lse"][b, :tyb, None])
        s["y"][b, :tyb] = np.linalg.norm(W @ np.abs(h), axis=1)
        s["lse"][b, :tyb] = np.maximum(np.abs(ref["lse"][b, :tyb]), 1.0)
        s["dh"][b, :txb] = np.linalg.norm(W.T @ np.abs(dy), axis=1)
        mag = W * (np.abs(dy) @ np.abs(h).T + (np.abs(dy) * np.abs(ref["y"][b, :tyb])).sum(axis=1, keepdims=True))
        s["dbias"][b, :txb] = mag.sum(axis=0)
        s["dcenter"][b, :txb] = (mag * np.abs(2 * pr[None, :] * d)).sum(axis=0)
        s["dprec"][b, :txb] = (mag * q).sum(axis=0)
    return s


def tiny(p):
    """What a row's weights multiply, plus one per element: times FTZ, the absolute allowance for
    flush-to-zero (see the module docstring).  [B, rows] per output."""
    B, tx, dim = p["h"].shape
    n_out = p["dy"].shape[1]
    ref = evaluate(p)
    t = {"y": np.zeros((B, n_out)), "lse": np.zeros((B, n_out)), "dh": np.zeros((B, tx)),
         "dcenter": np.zeros((B, tx)), "dprec": np.zeros((B, tx)), "dbias": np.zeros((B, tx))}
    txs, tys = lengths(p)
    for b in range(B):
        txb, tyb = txs[b], tys[b]
        if txb == 0 or tyb == 0:
            continue
        h, dy = p["h"][b, :txb], p["dy"][b, :tyb]
        d = (np.arange(tyb) + p["offset"])[:, None] - p["center"][b, :txb][None, :]
        t["y"][b, :tyb] = np.linalg.norm(np.abs(h).sum(axis=0)) + np.sqrt(dim)
        t["dh"][b, :txb] = np.linalg.norm(np.abs(dy).sum(axis=0)) + np.sqrt(dim)
        mag = np.abs(dy) @ np.abs(h).T + (np.abs(dy) * np.abs(ref["y"][b, :tyb])).sum(axis=1, keepdims=True)
        t["dbias"][b, :txb] = mag.sum(axis=0) + 1
        t["dcenter"][b, :txb] = (mag * np.abs(2 * p["prec"][b, :txb][None, :] * d)).sum(axis=0) + 1
        t["dprec"][b, :txb] = (mag * d * d).sum(axis=0) + 1
    return t


def out_ulp(p, name):
    return 2.0 ** -8 if p["dtype"] == "bf16" and name in ("y", "dh") else 2.0 ** -23


def _row_err(a, ref):
    d = np.asarray(a, dtype=np.float64) - ref
    d = np.where(np.isfinite(d), d, np.inf)
    return np.abs(d) if d.ndim == 2 else np.sqrt((d * d).sum(axis=2))


def padding_faults(p, out):
    """Names of the outputs whose padding is not exactly +0 (the sign bit counts)."""
    txs, tys = lengths(p)
    bad = []
    for k in out:
        lim = tys if k in ("y", "lse") else txs
        for b, n in enumerate(lim):
            pad = np.asarray(out[k][b, n:], dtype=np.float64)
            if pad.size and not (np.array_equal(pad, np.zeros_like(pad)) and not np.signbit(pad).any()):
                bad.append(k)
                break
    return bad


def judge(p, out, ref=None, yard=None, sc=None, ftz=True, detail=None, pool=True):
    """-> (worst ratio per output, names whose padding is not +0).  out: dict of arrays (any subset of
    OUTPUTS) holding the values of the kernel's outputs.  A ratio <= 1 passes.  sc: (scales(p),
    tiny(p)).  ftz=False leaves the flush-to-zero allowance out, pool=False the pooling of the
    yardstick's error (the issue's bar to the letter).  detail: a dict that receives, per
    output, (utterance, row, error, allowed, scale) of the worst row."""
    ref = evaluate(p) if ref is None else ref
    yard = yardstick(p) if yard is None else yard
    sc, tn = (scales(p), tiny(p)) if sc is None else sc
    ratios = {}
    for k in out:
        err = _row_err(out[k], ref[k])
        ey = np.max([_row_err(y[k], ref[k]) for y in yard], axis=0)
        # one evaluation is one draw of the rounding errors, and a row can be a single number (a phoneme's
        # dcenter) on which the draw happens to be 100 times smaller than on its neighbours: the
        # yardstick's error on a row is taken as no less than its RMS error relative to scale over the
        # utterance's rows, times the row's scale
        rel = np.where(sc[k] > 0, ey / np.where(sc[k] > 0, sc[k], 1.0), 0.0)
        live = np.maximum((sc[k] > 0).sum(axis=1, keepdims=True), 1)
        pooled = np.sqrt((rel * rel).sum(axis=1, keepdims=True) / live) * sc[k]
        allowed = np.maximum(4 * (np.maximum(ey, pooled) if pool else ey), 2 * out_ulp(p, k) * sc[k]) + (FTZ * tn[k] if ftz else 0.0)
        r = np.where(err == 0, 0.0, err / np.where(allowed > 0, allowed, 1e-300))
        ratios[k] = float(r.max()) if r.size else 0.0
        if detail is not None and r.size:
            b, i = np.unravel_index(np.argmax(r), r.shape)
            detail[k] = (int(b), int(i), float(err[b, i]), float(allowed[b, i]), float(sc[k][b, i]))
    return ratios, padding_faults(p, out)


def rejected(p, out, **kw):
    ratios, pads = judge(p, out, **kw)
    return bool(pads) or any(not (r <= 1.0) for r in ratios.values())


# ------------------------------------------------------------------------------------- problems
def length_cases(n, keys=False):
    """full, interior, 0 and above the bound: the frames in that order, the phonemes (keys=True) as
    interior, above the bound, full and 0, so that an interior length of either kind meets a full one
    of the other."""
    return [(n + 1) // 2, n + 3, n, 0] if keys else [n, (n + 1) // 2, 0, n + 3]


def _round_in(x, dtype):
    return bf16_round(x) if dtype == "bf16" else np.asarray(x, dtype=np.float32).astype(np.float64)


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _finish(p, n_out, tx, dim, dtype, rng, ints=None):
    B = 4
    if ints is None:
        p["h"] = _round_in(rng.normal(size=(B, tx, dim)), dtype)
        p["dy"] = _round_in(rng.normal(size=(B, n_out, dim)), dtype)
    else:
        p["h"] = rng.integers(-ints[0], ints[0] + 1, size=(B, tx, dim)).astype(np.float64)
        p["dy"] = rng.integers(-ints[1], ints[1] + 1, size=(B, n_out, dim)).astype(np.float64)
    p["dtype"] = dtype
    return p


def espnet_problem(n_out, tx, dim, dtype, seed=0):
    """ESPnet's convention: delta = 0.1, no bias, offset 0, centres from integer durations that fill
    about n_out frames."""
    rng = np.random.default_rng(1000 + seed)
    B = 4
    mean = max(n_out / max(tx, 1), 0.5)
    d = rng.poisson(mean, size=(B, tx)).astype(np.float64)
    p = {"center": _f32(np.cumsum(d, axis=1) - d / 2), "prec": _f32(np.full((B, tx), 0.1)), "bias": None,
         "offset": 0.0, "q_len": length_cases(n_out), "key_len": length_cases(tx, keys=True)}
    return _finish(p, n_out, tx, dim, dtype, rng)


def mix_problem(n_out, tx, dim, dtype, seed=0):
    """Wide and sharp phonemes side by side: prec log-uniform in [1e-3, 4], a bias in [-1, 1], centres
    spread over the frames in random order, offset 1 (Non-Attentive Tacotron's)."""
    rng = np.random.default_rng(2000 + seed)
    B = 4
    p = {"center": _f32(rng.uniform(0, max(n_out, 1), size=(B, tx))),
         "prec": _f32(np.exp(rng.uniform(np.log(1e-3), np.log(4.0), size=(B, tx)))),
         "bias": _f32(rng.uniform(-1, 1, size=(B, tx))), "offset": 1.0,
         "q_len": length_cases(n_out), "key_len": length_cases(tx, keys=True)}
    return _finish(p, n_out, tx, dim, dtype, rng)


def selector_problem(n_out, tx, dim, dtype, seed=0):
    """center[t] = t, offset 0, prec = 256, Ty_b = Tx_b: exp(-256) is exactly 0 in float32, so W is
    one-hot, y[n] is the bits of h[n], lse is exactly 0, dh[t] is the bits of dy[t] and dcenter, dprec
    and dbias are exactly 0.  h and dy are small integers."""
    rng = np.random.default_rng(3000 + seed)
    B = 4
    both = [min(v, min(n_out, tx)) for v in length_cases(min(n_out, tx))]
    both[3] = min(n_out, tx)
    p = {"center": _f32(np.broadcast_to(np.arange(tx), (B, tx))), "prec": _f32(np.full((B, tx), 256.0)),
         "bias": None, "offset": 0.0, "q_len": list(both), "key_len": list(both)}
    return _finish(p, n_out, tx, dim, dtype, rng, ints=(4, 4))


UNIFORM_TX = (16, 4, 2, 1)     # ln of these is exact enough in float32: see assert_uniform_premise


def uniform_problem(n_out, tx, dim, dtype, seed=0):
    """prec = 0 and bias = 0 with Tx_b a power of two: W = 1 / Tx_b, y is the exact mean, and with
    small-integer h and dy every gradient is an exact dyadic value.  Tx_b comes from UNIFORM_TX (the
    largest that fits, then the next ones; one utterance has Tx_b = 0)."""
    rng = np.random.default_rng(4000 + seed)
    B = 4
    fit = [v for v in UNIFORM_TX if v <= tx] or [0]
    key_len = [fit[0], fit[min(1, len(fit) - 1)], 0, fit[min(2, len(fit) - 1)]]
    p = {"center": _f32(np.broadcast_to(np.arange(tx), (B, tx))), "prec": np.zeros((B, tx)),
         "bias": np.zeros((B, tx)), "offset": 0.0, "q_len": length_cases(n_out), "key_len": key_len}
    return _finish(p, n_out, tx, dim, dtype, rng, ints=(2, 1))


def assert_uniform_premise():
    """Why UNIFORM_TX: the backward recomputes W = exp(-lse) with lse = ln Tx_b as float32.  For
    Tx_b = 2^k with k a power of two (or 0), float32(k ln 2) = k float32(ln 2) exactly, it differs from
    k ln 2 by less than 2^-26 relative, and its float32 product with float32(log2 e) is exactly k: the
    recomputed weight is exactly 2^-k whether the exponential is taken directly or through exp2."""
    ln2, log2e = np.float32(np.log(2.0)), np.float32(1.4426950408889634)
    for tx in UNIFORM_TX:
        k = int(np.log2(tx))
        lse = np.float32(np.log(np.float64(tx)))
        assert lse == np.float32(k) * ln2, tx
        assert np.float32(lse * log2e) == np.float32(k), tx
        assert np.float32(np.exp(-np.float64(lse))) == np.float32(1.0 / tx), tx
        # ... and through exp2 with the product carried in two floats (csrc/upsample.hip, gu_exp)
        hi, lo = np.float32(1.4426950216293335), np.float32(1.9259629911266175e-8)
        t = np.float32(-lse * hi)
        err = np.float32((-np.float64(lse) * np.float64(hi) - np.float64(t)) + np.float64(np.float32(-lse * lo)))
        r = np.float64(2.0) ** np.float64(t)
        assert t == -k and np.float32(r + r * np.float64(np.float32(err * ln2))) == np.float32(1.0 / tx), tx


def exact_expected(p):
    """What an exact problem's outputs must be, to the bit: the float32 evaluation (in which exp(-256)
    is 0 and exp(-ln 2^k) is 2^-k; test_upsample_refs.py checks it against the closed forms)."""
    return {k: v + 0.0 for k, v in evaluate(p, dt=np.float32).items()}       # a zero sum is +0


def exact_outputs(p):
    """The outputs of an exact problem that every float32 summation order gives to the bit: those
    whose expected value is representable in the output dtype, the same in both orders of
    float32_evaluations, and whose summands are all multiples of one quantum with magnitudes summing
    to less than 2^24 quanta (scales() has the magnitudes; the quantum is 2^-8: W, y and delta are
    multiples of 2^-4 at most, dE of 2^-8, and the factors of dcenter and dprec are integers).  The
    frame offsets of dprec grow as n^2, so at the larger shapes its float32 sum depends on the order
    and it is judged by the bar instead."""
    a, b = float32_evaluations(p)
    sc = scales(p)
    quantum = 2.0 ** -8
    names = []
    for k in OUTPUTS:
        r = a[k]
        rep = np.array_equal(bf16_round(r), r) if out_ulp(p, k) == 2.0 ** -8 else True
        # scales of y and dh are L2 norms over the columns: an upper bound of every column's magnitude
        if (rep and np.array_equal(r, b[k]) and np.all(sc[k] < 2.0 ** 24 * quantum)
                and np.array_equal(np.round(r / quantum), r / quantum)):
            names.append(k)
    return names
