"""References, problem builders and judges of the decode-step kernels (csrc/decode.hip and the
decode epilogues of csrc/gemm_skinny.hip), written from the contracts in include/tt2_capi.h.
Everything runs on the CPU.  tests/test_decode_refs.py validates this file against torch and
proves with mutants that the judges bite; tests/test_gpu_decode_exact.py holds the kernels to it.

Layout of a decode attention problem: one query row per batch element, q [B, H, 64] (or the
projection input x [B, 512] with Wq [512, 512], bq [512]), the keys and values of every cache
position K, V [B, T, H, 64], nk[b] visible keys (what min(tk, *t_ptr + 1, key_len[b]) comes to),
optionally Wo [H 64, H 64] (the fused output projection into one f32 slab per head) and the mask
of finished utterances.  Values are float64 numbers representable in the type under test.

evaluate() is the float64 reference and, in float32 with permuted summation orders, the yardstick
of the f32 outputs (the f32 kernel's `out`, and the slabs of every type: the kernel projects the
unrounded f32 head output).  The twin of a 16-bit `out` is the float64 result rounded once at the
store: the decode kernel keeps q, P and O in f32 and rounds nowhere else."""
from dataclasses import dataclass, field

import torch

import _attn_refs as A
from _attn_refs import D, F64, INF, LOG2E
from _misc_refs import EXACT_LIMIT

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NW, ITER = 8, 32                    # waves per (batch, head); keys per wave iteration (two buffers)
T_MAX = 520
BATCH = 3
NK = (0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 264, 511, 512, 513, 520)
DM = 512                            # the fused query projection's input width


# ------------------------------------------------------------------ the plain references
def ref_attn_decode(q, K, V, nk, scale, stop_mask=None):
    """o[B, H 64] in float64: softmax(scale q k^T) v over the keys j < nk[b]; zero where nk[b] <= 0
    or the utterance is finished.  q [B, H 64], K and V [B, T, H 64]."""
    B, HD = q.shape
    H = HD // D
    out = torch.zeros(B, HD, dtype=F64)
    for b in range(B):
        n = min(max(int(nk[b]), 0), K.shape[1])
        if n == 0 or (stop_mask is not None and bool(stop_mask[b])):
            continue
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            s = (K[b, :n, sl].to(F64) @ q[b, sl].to(F64)) * scale
            e = torch.exp(s - s.max())
            out[b, sl] = (e / e.sum()) @ V[b, :n, sl].to(F64)
    return out


def ref_qproj(x, Wq, bq):
    """q[b, r] = sum_k x[b, k] Wq[r, k] + bq[r] (float64)."""
    return x.to(F64) @ Wq.to(F64).t() + (0 if bq is None else bq.to(F64))


def ref_slabs(o, Wo):
    """slab[h, b, n] = sum_j o[b, 64 h + j] Wo[n, 64 h + j]: [H, B, H 64] float64."""
    B, HD = o.shape
    H = HD // D
    return torch.einsum("bhj,nhj->hbn", o.to(F64).view(B, H, D), Wo.to(F64).view(HD, H, D))


def ref_kv_append(cache, src, t, n):
    """cache [B, t_max, c_ld] after the call: row t, columns < n, becomes src[:, :n]; nothing is
    written for t >= t_max."""
    out = cache.clone()
    if 0 <= t < cache.shape[1]:
        out[:, t, :n] = src[:, :n]
    return out


def _f32(x):
    return torch.as_tensor(x, dtype=F32)


class EmitRef:
    """tt2_decode_emit (and the skinny GEMM's emit epilogue) as the header documents it, in float32
    where the kernel computes (one add, one compare).  The decisions are methods so that
    tests/test_decode_refs.py can derive deliberately wrong copies."""

    def stops(self, logit, thr):
        return logit >= thr

    def may_set(self, stop_len, t):
        return stop_len > t                   # the first stop wins

    def frames(self, mel, stop_len, t):
        return mel if stop_len is None else torch.where((stop_len <= t)[:, None], torch.zeros_like(mel), mel)

    def live(self, t, t_max):
        return t < t_max                      # the counter saturates at t_max

    def __call__(self, heads, t, t_max, n_mels, stop_bias, stop_len, stop_thr, seed, prev_dtype=F32):
        """heads [B, >= n_mels + 1] f32.  Returns {'mel': the new mel_seq[:, t] [B, n_mels] f32 or None,
        'stop': the new stop_seq[:, t] [B] or None, 'prev': [B, n_mels] of prev_dtype or None,
        'stop_len': [B] int32 or None, 't', 'seed'}; None = nothing written."""
        out = {"mel": None, "stop": None, "prev": None, "t": t, "seed": seed,
               "stop_len": None if stop_len is None else stop_len.clone()}
        if not self.live(t, t_max):
            return out
        heads = _f32(heads)
        mel = self.frames(heads[:, :n_mels], stop_len, t)
        logit = heads[:, n_mels] if stop_bias is None else heads[:, n_mels] + _f32(stop_bias)[:, min(t, t_max - 1)]
        out.update(mel=mel, stop=logit, prev=mel.to(prev_dtype), t=t + 1,
                   seed=None if seed is None else (seed + 1) & 0xFFFFFFFF)
        if stop_len is not None:
            hit = self.stops(logit, _f32(stop_thr)) & self.may_set(stop_len, t)
            out["stop_len"] = torch.where(hit, torch.full_like(stop_len, t + 1), stop_len)
        return out


def ref_emit(heads, t, t_max, n_mels, stop_bias, stop_len, stop_thr, seed, prev_dtype=F32):
    return EmitRef()(heads, t, t_max, n_mels, stop_bias, stop_len, stop_thr, seed, prev_dtype)


def emit_sequence(emit, heads_steps, t_max, n_mels, stop_bias, stop_len0, stop_thr, seed0, prev_dtype=F32):
    """`emit` applied step after step to buffers that start as NaN (mel_seq, stop_seq, prev): the
    list of states {'mel_seq' [B, t_max, n_mels], 'stop_seq' [B, t_max], 'prev', 'stop_len', 't',
    'seed'} after every step."""
    B = heads_steps[0].shape[0]
    st = {"mel_seq": torch.full((B, t_max, n_mels), float("nan")), "stop_seq": torch.full((B, t_max), float("nan")),
          "prev": torch.full((B, n_mels), float("nan")).to(prev_dtype),
          "stop_len": None if stop_len0 is None else stop_len0.clone(), "t": 0, "seed": seed0}
    states = []
    for heads in heads_steps:
        r = emit(heads, st["t"], t_max, n_mels, stop_bias, st["stop_len"], stop_thr, st["seed"], prev_dtype)
        st = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
        if r["mel"] is not None and st["t"] < t_max:
            st["mel_seq"][:, st["t"]], st["stop_seq"][:, st["t"]], st["prev"] = r["mel"], r["stop"], r["prev"]
        st["stop_len"], st["t"], st["seed"] = r["stop_len"], r["t"], r["seed"]
        states.append(st)
    return states


def same_state(a, b):
    """The names of the fields in which two emit states differ bit for bit (NaN equal to NaN)."""
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if torch.is_tensor(x):
            ok = x.dtype == y.dtype and torch.equal(torch.nan_to_num(x.double(), nan=1e300),
                                                    torch.nan_to_num(y.double(), nan=1e300))
        else:
            ok = x == y
        if not ok:
            bad.append(k)
    return bad


# The scripted stop logits of the emit tests: t_max = 4, five steps (the fifth, at t = t_max, must
# change nothing), threshold 0.5.  A logit is coarse + fine, fine = 0 or -2^-25, so that
# nextafter(0.5, 0) is a sum of two bf16 / f16 values (the heads GEMM of the skinny test places the
# two terms in different wave slices of K, whose partials meet in one IEEE f32 add).  Row:
#   0  nextafter(0.5, 0) at step 0 (no stop), exactly 0.5 at step 1 (>= stops it: stop_len = 2)
#   1  crosses at step 0 and again at step 2 (the first wins: stop_len = 1; zero frames from step 1)
#   2  -0.25 at every step, lifted over the threshold at step 2 by stop_bias alone (stop_len = 3)
#   3  nextafter(0.5, 0) at every step: never stops (stop_len stays INT32_MAX)
#   4+ -2 at every step
EMIT_TMAX, EMIT_THR, EMIT_FINE = 4, 0.5, -2.0 ** -25
INT32_MAX = 2 ** 31 - 1


def emit_script(B):
    """(coarse [steps, B], fine [steps, B], stop_bias [B, t_max], expected final stop_len [B])."""
    steps = EMIT_TMAX + 1
    coarse, fine = torch.full((steps, B), -2.0, dtype=F64), torch.zeros(steps, B, dtype=F64)
    want = torch.full((B,), INT32_MAX, dtype=torch.int32)
    bias = torch.zeros(B, EMIT_TMAX, dtype=F32)
    if B > 0:
        coarse[0, 0], fine[0, 0], coarse[1, 0] = 0.5, EMIT_FINE, 0.5
        want[0] = 2
    if B > 1:
        coarse[:3, 1] = torch.tensor([1.0, -1.0, 2.0], dtype=F64)
        want[1] = 1
    if B > 2:
        coarse[:, 2] = -0.25
        bias[2, 2] = 1.0
        want[2] = 3
    if B > 3:
        coarse[:, 3], fine[:, 3] = 0.5, EMIT_FINE
    coarse[EMIT_TMAX], fine[EMIT_TMAX] = 4.0, 0.0      # the step at t_max would stop every row if it ran
    return coarse, fine, bias, want


# ------------------------------------------------------------------ decode attention problems
@dataclass
class DecProblem:
    k: torch.Tensor                 # [B, T, H, 64] float64
    v: torch.Tensor                 # [B, T, H, 64]
    nk: list                        # B visible key counts (0 .. T)
    scale: float                    # a float32 value
    q: torch.Tensor = None          # [B, H, 64], or None with the fused projection:
    x: torch.Tensor = None          # [B, 512]
    wq: torch.Tensor = None         # [512, 512]
    bq: torch.Tensor = None         # [512]
    wo: torch.Tensor = None         # [H 64, H 64] or None
    stopped: list = None            # B bools or None
    sel: torch.Tensor = None        # selector problem: the selected key of each (b, h), -1 = none
    extra: dict = field(default_factory=dict)

    @property
    def shape(self):
        B, T, H, _ = self.k.shape
        return B, H, T

    def query(self, dtype=F64, perm=None):
        """[B, H, 64] in `dtype`: q, or x Wq^T + bq computed in `dtype` (k permuted by `perm`)."""
        B, H, T = self.shape
        if self.q is not None:
            return self.q.to(dtype)
        x, w = self.x.to(dtype), self.wq.to(dtype)
        if perm is not None:
            x, w = x[:, perm], w[:, perm]
        return (x @ w.t() + self.bq.to(dtype)).view(B, H, D)


def counts_weights(p, nk=None):
    """[B, H, T] float64 multiplicity of every key: 1 for j < nk[b], else 0."""
    B, H, T = p.shape
    n = torch.tensor(p.nk if nk is None else nk).clamp(0, T)
    return (torch.arange(T)[None, :] < n[:, None]).to(F64)[:, None, :].expand(B, H, T).clone()


def evaluate(p, dtype=F64, rnd=None, weights=None, perms=None, round_o_for_proj=None):
    """{'o': [B, H, 64] float64 (rounded to `rnd` at the store), 'slab': [H, B, H 64] or None}.
    weights [B, H, T]: how often each key counts (the mutants of tests/test_decode_refs.py drop,
    leak and double keys through it).  perms = (perm of the 64 head dims, perm of the T keys, perm
    of the 512 projection inputs): another summation order, for the float32 yardstick.
    round_o_for_proj: round the head output to this type before the projection (a mutant)."""
    B, H, T = p.shape
    pd, pt, px = perms if perms is not None else (None, None, None)
    w = counts_weights(p) if weights is None else weights
    q, k, v = p.query(dtype, px), p.k.to(dtype), p.v.to(dtype)
    if pd is not None:
        q, k = q[..., pd], k[..., pd]
    if pt is not None:
        k, v, w = k[:, pt], v[:, pt], w[..., pt]
    c = torch.tensor(p.scale, dtype=dtype) * torch.tensor(LOG2E, dtype=dtype)
    s = torch.einsum("bhd,bthd->bht", q, k) * c
    s = s.masked_fill(w == 0, -INF)
    m = s.amax(-1, keepdim=True) if T > 0 else torch.full((B, H, 1), -INF, dtype=dtype)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp2(s - m) * w.to(dtype)
    l = e.sum(-1, keepdim=True)
    o = torch.einsum("bht,bthd->bhd", e, v) / torch.where(l > 0, l, torch.ones_like(l))
    o = torch.where(l > 0, o, torch.zeros_like(o))
    if p.stopped is not None:
        o = o * (~torch.tensor(p.stopped))[:, None, None].to(dtype)
    slab = None
    if p.wo is not None:
        op = o if round_o_for_proj is None else o.to(round_o_for_proj).to(dtype)
        slab = torch.einsum("bhj,nhj->hbn", op, p.wo.to(dtype).view(H * D, H, D)).to(F64)
    o = o if rnd is None else o.to(rnd).to(dtype)
    return {"o": o.to(F64), "slab": slab}


def float32_evaluations(p, orders=6):
    """evaluate() in float32 in `orders` summation orders (the first is the plain one), the
    yardstick of the f32 outputs, as _attn_refs.float32_evaluations."""
    B, H, T = p.shape
    outs = []
    for i in range(orders):
        if i == 0:
            outs.append(evaluate(p, F32))
            continue
        g = torch.Generator().manual_seed(i)
        outs.append(evaluate(p, F32, perms=(torch.randperm(D, generator=g), torch.randperm(T, generator=g),
                                            torch.randperm(DM, generator=g))))
    return outs


def twin(p, dtype):
    """What a 16-bit kernel may be held to for `out`: float64, rounded once at the store."""
    return evaluate(p, F64, rnd=dtype)


# ---- the seams of the kernel's key walk
def wave_ranges(nk):
    """[(k0, k1)] of the 8 waves: contiguous ranges of per = roundup8(ceil(nk / 8)) keys."""
    per = ((nk + NW - 1) // NW + 7) & ~7
    return [(w * per, min(nk, (w + 1) * per)) for w in range(NW)]


def seam_keys(nk):
    """The key positions a selector problem visits, in order: the first and last key, the first and
    last key of every non-empty wave range, and both sides of every 32-key iteration boundary of
    the first and the last non-empty wave."""
    if nk <= 0:
        return []
    live = [(a, b) for a, b in wave_ranges(nk) if a < b]
    out = [0, nk - 1]
    for a, b in live:
        out += [a, b - 1]
    for a, b in (live[0], live[-1]):
        for kb in range(a + ITER, b, ITER):
            out += [kb - 1, kb]
    seen, uniq = set(), []
    for x in out:
        if x not in seen:
            seen.add(x)
            uniq.append(x)
    return uniq


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(x) for x in key)) % (2 ** 31))


def _labelled_values(g, B, T, H):
    """V [B, T, H, 64], small integers, every row distinct per key, head and batch element: the
    first four entries spell (key mod 128 - 64, key div 128, head, batch), the rest are in [-2, 2]."""
    v = _ints(g, -2, 2, B, T, H, D)
    t = torch.arange(T, dtype=F64)
    v[..., 0] = (t % 128 - 64)[None, :, None]
    v[..., 1] = (t // 128)[None, :, None]
    v[..., 2] = torch.arange(H, dtype=F64)[None, None, :]
    v[..., 3] = torch.arange(B, dtype=F64)[:, None, None]
    return v


def solve_wq(g, x, target, density=0.25):
    """(Wq [512, 512], bq [512]) of small integers with x Wq^T + bq == target exactly, for an x
    [B, 512] whose first B columns are the identity: the other columns of Wq are random in
    {-1, 0, 1} (a quarter of them non-zero), bq in [-3, 3], and column b takes what row b still
    lacks.  A wrong index anywhere in the projection then misses the target code."""
    B = x.shape[0]
    assert torch.equal(x[:, :B], torch.eye(B, dtype=F64))
    wq = _ints(g, -1, 1, DM, DM) * (torch.rand(DM, DM, generator=g) < density)
    bq = _ints(g, -3, 3, DM)
    wq[:, :B] = 0
    wq[:, :B] = (target - (x @ wq.t() + bq)).t()
    assert torch.equal(x @ wq.t() + bq, target)
    return wq, bq


def selector_problem(H, nk, T=T_MAX, rot=0, wo=False, wq=False, x=None, stopped=None, seed=0):
    """The exact problem.  K[b, t, h] = the code of key t (_attn_refs.selector_codes: 64 at two
    places), q[b, h] = the code of one visible key, scale 0.125: that key leads every other by
    4096 in the dot product, 738 in the log2 domain, so every other exp2f term is exactly 0 in f32
    and o[b, h] is exactly the selected key's V row.  The selected key walks seam_keys(nk[b]) with
    (b, h) (from `rot` on).  The first key past nk[b] is a copy of the selected one with another V
    row: a key leaking in from beyond the count halves the answer.  nk[b] == 0: q = 0, o = 0.
    wo: Wo of integers in [-2, 2].  wq: the query is x Wq^T + bq with integers (solve_wq); x given
    ([B, 512], first B columns the identity): the projection input an LN prologue produces."""
    B = len(nk)
    g = _gen(1, H, rot, seed, *nk)
    codes = A.selector_codes(T)
    k = codes[None, :, None, :].expand(B, T, H, D).clone()
    v = _labelled_values(g, B, T, H)
    sel = torch.full((B, H), -1, dtype=torch.long)
    q = torch.zeros(B, H, D, dtype=F64)
    for b in range(B):
        seams = seam_keys(min(nk[b], T))
        for h in range(H):
            if not seams:
                continue
            t = seams[(b * H + h + rot) % len(seams)]
            sel[b, h] = t
            q[b, h] = codes[t]
            if nk[b] < T:
                k[b, nk[b], h] = codes[t]
                v[b, nk[b], h, 4:] = 7.0
    p = DecProblem(k, v, list(nk), 0.125, q=q, sel=sel, stopped=stopped)
    if wo:
        p.wo = _ints(g, -2, 2, H * D, H * D)
    if wq:
        assert H * D == DM
        if x is None:
            x = _ints(g, -1, 1, B, DM)
            x[:, :B] = torch.eye(B, dtype=F64)
        p.x = x
        p.wq, p.bq = solve_wq(g, x, q.view(B, DM))
        p.q = None
    return p


def ln_selector_problem(nk, rot=0, seed=0):
    """The selector problem behind the fused LayerNorm prologue: (ln, p).  ln is a
    _norm_refs.LnFwdExact(B, splits = 8) (rows K +- 1, eps = 3: mean K, rstd 1 / 2 exactly) whose
    gamma / beta make every normalised value a small integer and the first B columns the identity
    (gamma 1, beta 1 / 2, the row's own column at K + 1 and the others at K - 1, each swapped with
    a later column of the row so that it stays half and half); ln.y is that row, the projection
    input of p = selector_problem(8, nk, wo, wq, x = ln.y)."""
    import _norm_refs as N
    B = len(nk)
    ln = N.LnFwdExact(B, splits=8, seed=seed)
    g = _gen(4, rot, seed, *nk)
    d = ln.s - ln.K[:, None]
    for b in range(B):
        for k in range(B):
            want = 1.0 if k == b else -1.0
            if d[b, k] != want:
                j = B + int((d[b, B:] == want).nonzero()[0])
                d[b, k], d[b, j] = d[b, j].item(), d[b, k].item()
    ln.s = ln.K[:, None] + d
    ln.x = ln.s - ln.bias - ln.parts.sum(0)
    ln.gamma = torch.tensor([2.0, -2.0, 4.0, -4.0], dtype=F64)[torch.randint(0, 4, (N.LN_C,), generator=g)]
    ln.gamma[:B], ln.beta[:B] = 1.0, 0.5
    assert ln.exact()[0]
    ln.y = N.ref_ln_combine(ln.x, ln.parts, ln.bias, ln.gamma, ln.beta, ln.EPS)
    assert torch.equal(ln.y, ln.y.round()) and ln.y.abs().max() <= 5 and torch.equal(ln.y[:, :B], torch.eye(B, dtype=F64))
    return ln, selector_problem(8, nk, rot=rot, wo=True, wq=True, x=ln.y, seed=seed)


def selector_expected(p):
    """o [B, H, 64] in closed form: V[b, sel[b, h], h], 0 without a key or when finished."""
    B, H, T = p.shape
    o = torch.zeros(B, H, D, dtype=F64)
    for b in range(B):
        for h in range(H):
            if p.sel[b, h] >= 0 and not (p.stopped is not None and p.stopped[b]):
                o[b, h] = p.v[b, p.sel[b, h], h]
    return o


def uniform_problem(H, nk, T=T_MAX, wo=False, stopped=None, seed=0):
    """q = 0: every visible key has p = 1 and o is the mean of the nk[b] visible V rows, an exact
    integer sum divided once.  V in [-2, 2]; with wo, V in [0, 4] and Wo in [0, 2]: each slab entry
    is then a sum of non-negative terms, so its float32 error is a few ulp of the entry itself and
    the 4-ulp bar is meaningful (with mixed signs a slab entry can cancel to a value far below its
    terms, where no float32 evaluation keeps 4 ulp of it)."""
    B = len(nk)
    g = _gen(2, H, seed, int(wo), *nk)
    k = _ints(g, -2, 2, B, T, H, D)
    v = _ints(g, 0, 4, B, T, H, D) if wo else _ints(g, -2, 2, B, T, H, D)
    p = DecProblem(k, v, list(nk), 0.125, q=torch.zeros(B, H, D, dtype=F64), stopped=stopped)
    if wo:
        p.wo = _ints(g, 0, 2, H * D, H * D)
    return p


def uniform_expected(p):
    """o [B, H, 64]: the exact integer sum of the visible V rows divided once by their number."""
    w = counts_weights(p)
    n = w.sum(-1).clamp_min(1)
    o = torch.einsum("bht,bthd->bhd", w, p.v) / n[..., None]
    if p.stopped is not None:
        o = o * (~torch.tensor(p.stopped))[:, None, None].to(F64)
    return o


def random_problem(H, nk, dtype, T=T_MAX, wo=False, wq=False, stopped=None, seed=0):
    """Gaussian inputs rounded to `dtype`; scale 0.1 (c = scale log2(e) is no power of two); the
    projections are scaled by 1 / sqrt(fan-in)."""
    B = len(nk)
    g = _gen(3, H, seed, *nk)
    rd = lambda t: t.to(dtype).to(F64)                                     # noqa: E731
    k, v = rd(torch.randn(B, T, H, D, generator=g)), rd(torch.randn(B, T, H, D, generator=g))
    p = DecProblem(k, v, list(nk), A.f32_scale(0.1), q=rd(torch.randn(B, H, D, generator=g)), stopped=stopped)
    if wo:
        p.wo = rd(torch.randn(H * D, H * D, generator=g) / (H * D) ** 0.5)
    if wq:
        assert H * D == DM
        p.x, p.wq = rd(torch.randn(B, DM, generator=g)), rd(torch.randn(DM, DM, generator=g) / DM ** 0.5)
        p.bq = torch.randn(DM, generator=g).to(F32).to(F64)
        p.q = None
    return p


# ------------------------------------------------------------------ exactness of the exact problems
def _sum_exact(terms, dim):
    """sum |terms| < 2^24 along dim for integer-valued terms: every f32 partial sum is exact."""
    assert torch.equal(terms, terms.round()), "not integer-valued"
    return bool((terms.abs().sum(dim) < EXACT_LIMIT).all())


def assert_exact_selector(p, dtype):
    """Proves on the CPU what the selector problem claims: inputs and the float64 result are values
    of `dtype` (the slabs of f32), the selected key leads by more than 200 in the log2 domain
    (exp2f is 0 below -150), the float64 result is the closed form, and every partial sum of the
    projections is exact in f32.  Returns the float64 reference."""
    B, H, T = p.shape
    for name in ("q", "x", "wq", "k", "v", "wo"):
        t = getattr(p, name)
        assert t is None or A.representable(t, dtype), f"selector: {name} is not a {dtype} value"
    q = p.query()
    if p.wq is not None:
        assert _sum_exact(p.x[:, None, :] * p.wq[None], -1) and A.representable(q, F32)
    s = torch.einsum("bhd,bthd->bht", q, p.k) * (p.scale * LOG2E)
    s = s.masked_fill(counts_weights(p) == 0, -INF)
    top = s.topk(min(2, T), -1).values
    for b in range(B):
        if p.nk[b] > 1:
            assert (top[b, :, 0] - top[b, :, 1]).min().item() > 200, "selector: the lead is too small"
        if p.nk[b] > 0:
            assert torch.equal(s[b].argmax(-1), p.sel[b])
    ref = evaluate(p)
    want = selector_expected(p)
    assert (ref["o"] - want).abs().max().item() < 1e-100 and A.representable(ref["o"], dtype)
    ref["o"] = want
    if p.wo is not None:
        terms = want[:, :, None, :] * p.wo.view(H * D, H, D).permute(1, 0, 2)[None]      # [B, H, N, 64]
        assert _sum_exact(terms, -1)
        ref["slab"] = terms.sum(-1).permute(1, 0, 2).contiguous()
        assert A.representable(ref["slab"], F32)
    return ref


def assert_exact_uniform(p):
    """The integer sums of the uniform problem are exact in f32 in any order, and so is every
    slab entry of a batch element whose count is a power of two."""
    B, H, T = p.shape
    assert _sum_exact(p.v * counts_weights(p).permute(0, 2, 1)[..., None], 1)
    if p.wo is not None:
        tot = torch.einsum("bht,bthd->bhd", counts_weights(p), p.v)
        assert _sum_exact(tot[:, :, None, :] * p.wo.view(H * D, H, D).permute(1, 0, 2)[None], -1)


# ------------------------------------------------------------------ judges
# Each takes what a kernel (or a mutant) returned, {'o': [B, H, 64] float64 or None, 'slab':
# [H, B, H 64] float64 or None}, and returns (failures in words, figures for `pytest -s`).
F32_FLOOR = A.F32_FLOOR


def _first_diff(a, b):
    i = (a != b).nonzero()[0].tolist()
    return f"first at {i}: got {a[tuple(i)].item()!r}, expected {b[tuple(i)].item()!r} ({int((a != b).sum())} differ)"


def judge_selector(out, ref, dtype):
    """Bit-equal: o to the float64 reference cast to `dtype`, the slabs to it in f32."""
    fails = []
    for n, dt in (("o", dtype), ("slab", F32)):
        if out.get(n) is None:
            continue
        want = ref[n].to(dt).to(F64)
        if not torch.equal(out[n], want):
            fails.append(f"{n} differs from the float64 reference: {_first_diff(out[n], want)}")
    return fails, {}


def judge_uniform(out, p, dtype):
    """o: equal to RN(mean) where the count is a power of two (and where it is 0), elsewhere
    within 1 ulp of RN(mean) in a 16-bit type and 4 f32 ulp of the mean in f32.  Slabs: equal where
    the count is a power of two, elsewhere within 4 f32 ulp."""
    fails, figs = [], {}
    B, H, T = p.shape
    n = torch.tensor(p.nk).clamp(0, T)
    pow2 = (n & (n - 1)) == 0
    o_ref = uniform_expected(p)
    if out.get("o") is not None:
        want = o_ref.to(dtype).to(F64)
        if not torch.equal(out["o"][pow2], want[pow2]):
            fails.append("o differs where the count is a power of two: " + _first_diff(out["o"][pow2], want[pow2]))
        d = A.ulp_distance(out["o"], o_ref if dtype == F32 else want, dtype)
        figs["o_ulp"] = d.max().item() if d.numel() else 0.0
        if not figs["o_ulp"] <= (4 if dtype == F32 else 1):
            fails.append(f"o is {figs['o_ulp']:.3g} ulp from the mean")
    if out.get("slab") is not None:
        s_ref = torch.einsum("bhj,nhj->hbn", o_ref, p.wo.view(H * D, H, D))
        want = s_ref.to(F32).to(F64)
        if not torch.equal(out["slab"][:, pow2], want[:, pow2]):
            fails.append("slab differs where the count is a power of two: "
                         + _first_diff(out["slab"][:, pow2], want[:, pow2]))
        d = A.ulp_distance(out["slab"], s_ref, F32)
        figs["slab_ulp"] = d.max().item() if d.numel() else 0.0
        if not figs["slab_ulp"] <= 4:
            fails.append(f"slab is {figs['slab_ulp']:.3g} f32 ulp from the reference")
    return fails, figs


def vector_ratio(out, ref, yard, dtype):
    """_attn_refs.worst_ratio with one (b, h) vector per block: the vector's error against float64
    over max(factor x the yardstick's error on the same vector, floor); 2 x the twin for a 16-bit
    type, max(4 x the float32 evaluations, 2 f32 ulp) for f32.  Tensors [X, Y, n]."""
    factor, floor = (4.0, F32_FLOOR) if dtype == F32 else (2.0, 0.0)
    v4 = lambda t: t[:, :, None, :]                                        # noqa: E731
    ys = [v4(y) for y in yard] if isinstance(yard, (list, tuple)) else v4(yard)
    return A.worst_ratio(v4(out), v4(ref), ys, factor, floor, rows=1)


def judge_random(out, ref, yard16, yard32, dtype):
    """Every (b, h) 64-vector of o against the twin (16-bit) or the float32 evaluations (f32), every
    (h, b) row of the slabs against the float32 evaluations."""
    fails, figs = [], {}
    if out.get("o") is not None:
        figs["o"] = vector_ratio(out["o"], ref["o"], [y["o"] for y in yard32] if dtype == F32 else yard16["o"], dtype)
        if not figs["o"] <= 1:
            fails.append(f"o: worst (b, h) vector at {figs['o']:.3g} times its bar")
    if out.get("slab") is not None:
        figs["slab"] = vector_ratio(out["slab"], ref["slab"], [y["slab"] for y in yard32], F32)
        if not figs["slab"] <= 1:
            fails.append(f"slab: worst (h, b) row at {figs['slab']:.3g} times its bar")
    return fails, figs


def old_global_bar(out, ref):
    """The bar of tests/test_gpu_decode_kernels.py: relative Frobenius norm over the whole output
    < 1e-2.  True if it accepts `out`."""
    ok = True
    for n in ("o", "slab"):
        if out.get(n) is not None:
            ok &= ((out[n] - ref[n]).norm() / ref[n].norm().clamp_min(1e-30)).item() < 1e-2
    return ok


def show(figs):
    return ", ".join(f"{k} {v:.3f}" for k, v in figs.items()) or "equal"


# ------------------------------------------------------------------ the cases of the GPU test
def nk_triple(i):
    """Three key counts for B = 3 starting at NK[i]: over i every count of NK is met three times,
    once per batch slot, next to counts from other parts of the list (0 among them)."""
    return [NK[i], NK[(i + 5) % len(NK)], NK[(i + 11) % len(NK)]]


FORMS = ("self", "cross", "both")
DTYPES = (BF16, F16, F32)


def cases(rot):
    """[(id, i, nk [3], form, dtype)]: every count of NK with one form and one type, taken in turn
    from `rot` on (each problem passes another rot, so a count meets all three of each).
    self: t_ptr = nk - 1 for every batch element; cross: ragged key_len; both: t_ptr, key_len and
    a tk below some of them, the minimum applies."""
    out = []
    for i, n in enumerate(NK):
        form, dtype = FORMS[(i + rot) % 3], DTYPES[(i // 3 + rot) % 3]
        nk = [n] * BATCH if form == "self" else nk_triple(i)
        tag = {BF16: "bf16", F16: "f16", F32: "f32"}[dtype]
        out.append((f"nk{n}-{form}-{tag}", i, nk, form, dtype))
    return out


SELECTOR_ROT, UNIFORM_ROT, RANDOM_ROT = 0, 1, 2
