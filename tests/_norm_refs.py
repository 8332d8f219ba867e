"""Plain references of the LayerNorm and BatchNorm kernels in csrc/layernorm.hip and
csrc/batchnorm.hip, written from the
contracts in include/tt2_capi.h (not from the kernels), and the exact-arithmetic problems of
tests/test_gpu_norm_exact.py.  Everything runs on the CPU in float64 unless a `dtype` is given:
the same code in float32 is the yardstick of the non-exact checks (`worst_ratio_by`).  No
autograd.  Inputs are taken in their storage type (bf16 / f16 tensors are already rounded), so
the reference sees what the kernel reads.  tests/test_norm_refs.py validates all of this against
torch.nn.functional and autograd and shows, with a numpy model of the kernels and fifteen wrong
copies of it, that the bars bite.

Dropout: `keep` is the bool mask of tt2_oracle.dropout_keep (None: no dropout) and `scale` the
float32 factor 1 / (1 - p) the kernel is handed."""
import numpy as np
import torch

from _misc_refs import EXACT_LIMIT, F64, ulp, worst_ratio
from tt2_oracle import dropout_keep

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
LN_C = 512


def f32w(v):
    """A Python float as the kernel sees it after the C ABI's float argument: rounded to f32."""
    return float(np.float32(v))


def drop_scale(p):
    return f32w(1.0 / (1.0 - p)) if p > 0 else 1.0


def keep_mask(seed, site, m, c, p):
    """bool [m, c] keep mask of the flat element index m * c + col (None for p == 0)."""
    if p <= 0:
        return None
    return torch.from_numpy(dropout_keep(seed, site, m * c, p)).view(m, c)


def _keepf(keep, scale, like, dtype):
    """The dropout factor per element: scale where kept, 0 where dropped, 1 without dropout."""
    if keep is None:
        return torch.ones((), dtype=dtype)
    return torch.where(keep, torch.tensor(f32w(scale), dtype=dtype), torch.zeros((), dtype=dtype))


def _act(act, v):
    return v.clamp_min(0) if act == ACT_RELU else (torch.tanh(v) if act == ACT_TANH else v)


def _act_grad_from_out(act, z):
    if act == ACT_RELU:
        return (z > 0).to(z.dtype)
    return 1 - z * z if act == ACT_TANH else torch.ones_like(z)


# --------------------------------------------------------------- LayerNorm
def ref_ln_fwd(x, branch, keep, gamma, beta, eps, scale=1.0, dtype=F64):
    """s = x + drop(branch); y = (s - mean(s)) * rstd * gamma + beta with the biased variance.
    Returns y, mean, rstd ([M, C], [M], [M])."""
    s = x.to(dtype)
    if branch is not None:
        s = s + branch.to(dtype) * _keepf(keep, scale, s, dtype)
    C = s.shape[1]
    mean = s.sum(1) / C
    d = s - mean[:, None]
    rstd = 1 / torch.sqrt((d * d).sum(1) / C + torch.tensor(f32w(eps), dtype=dtype))
    y = d * rstd[:, None] * gamma.to(dtype) + beta.to(dtype)
    return y, mean, rstd


def ref_ln_bwd(dy, x, branch, keep, gamma, mean, rstd, grad_beta=0.0, dgamma0=None, dbeta0=None, dbias0=None,
               scale=1.0, dtype=F64):
    """The backward of ref_ln_fwd with `mean` and `rstd` taken as given (they need not be the
    rows' own statistics).  xh = (s - mean) * rstd, gd = gamma * dy, c1 = mean(gd),
    c2 = mean(gd * xh): dx = rstd * (gd - c1 - xh * c2), dbranch = drop(dx),
    dgamma = grad_beta * dgamma0 + sum_rows dy * xh, dbeta = ... + sum_rows dy,
    dbias = ... + sum_rows dbranch (of the unrounded dbranch).  grad_beta == 0 ignores the priors.
    Returns dx, dbranch, dgamma, dbeta, dbias."""
    s = x.to(dtype)
    kf = _keepf(keep, scale, s, dtype)
    if branch is not None:
        s = s + branch.to(dtype) * kf
    C = s.shape[1]
    rs = rstd.to(dtype)[:, None]
    xh = (s - mean.to(dtype)[:, None]) * rs
    d = dy.to(dtype)
    gd = gamma.to(dtype) * d
    c1 = gd.sum(1, keepdim=True) / C
    c2 = (gd * xh).sum(1, keepdim=True) / C
    dx = rs * (gd - c1 - xh * c2)
    dbr = dx * kf

    def acc(v, prior):
        return v if grad_beta == 0 else f32w(grad_beta) * prior.to(dtype) + v
    return dx, dbr, acc((d * xh).sum(0), dgamma0), acc(d.sum(0), dbeta0), acc(dbr.sum(0), dbias0)


def ref_ln_combine(x, parts, bias, gamma, beta, eps, dtype=F64):
    """y = LN(x + bias + sum_s parts[s]); x [M, C] bf16 / f16, parts [S, M, C] f32."""
    v = x.to(dtype) + (bias.to(dtype) + parts.to(dtype).sum(0))
    y, _, _ = ref_ln_fwd(v, None, None, gamma, beta, eps, dtype=dtype)
    return y


# --------------------------------------------------------------- BatchNorm
def ref_bn_fwd(y, gamma, beta, keep, res, act, eps, momentum, run_mean, run_var, training, scale=1.0, dtype=F64):
    """z = act((y - mean) * rstd * gamma + beta); out = drop(z) (+ res[:, :C]).  Training: the
    column mean and biased variance of y, and running = (1 - momentum) * running + momentum *
    (mean, unbiased variance; the biased one for M == 1).  Eval: the running statistics, left
    unchanged.  eps and momentum are float32 values widened (the kernel's double arithmetic
    sees them so).  Returns out, mean, rstd, run_mean, run_var."""
    v = y.to(dtype)
    M, C = v.shape
    e, mo = torch.tensor(f32w(eps), dtype=dtype), torch.tensor(f32w(momentum), dtype=dtype)
    if training:
        mean = v.sum(0) / M
        m2 = ((v - mean) ** 2).sum(0)
        var = m2 / M
        unb = m2 / (M - 1) if M > 1 else var
        rstd = 1 / torch.sqrt(var + e)
        new_rm, new_rv = None, None
        if run_mean is not None:
            new_rm = (1 - mo) * run_mean.to(dtype) + mo * mean
            new_rv = (1 - mo) * run_var.to(dtype) + mo * unb
    else:
        mean = run_mean.to(dtype)
        rstd = 1 / torch.sqrt(run_var.to(dtype) + e)
        new_rm, new_rv = run_mean.to(dtype), run_var.to(dtype)
    out = ref_bn_apply(y, mean, rstd, gamma, beta, keep, res, act, scale=scale, dtype=dtype)
    return out, mean, rstd, new_rm, new_rv


def ref_bn_apply(y, mean, rstd, gamma, beta, keep, res, act, scale=1.0, dtype=F64):
    """out = drop(act((y - mean) * rstd * gamma + beta)) (+ res[:, :C]) with the statistics given."""
    C = y.shape[1]
    z = _act(act, (y.to(dtype) - mean.to(dtype)) * rstd.to(dtype) * gamma.to(dtype) + beta.to(dtype))
    out = z * _keepf(keep, scale, z, dtype)
    if res is not None:
        out = out + res[:, :C].to(dtype)
    return out


def ref_bn_combine(mom, rows, m, eps, dtype=F64):
    """Chunk moments [R, 2, C] (chunks of `rows` rows, a short last one) -> mean, M2, rstd of the
    m rows: mean = sum n_c mean_c / m, M2 = sum M2_c + n_c (mean_c - mean)^2."""
    n = torch.tensor([r1 - r0 for r0, r1 in _chunks(m, rows)], dtype=dtype)[:, None]
    mc, m2c = mom[:, 0].to(dtype), mom[:, 1].to(dtype)
    mean = (n * mc).sum(0) / m
    m2 = (m2c + n * (mc - mean) ** 2).sum(0)
    return mean, m2, 1 / torch.sqrt(m2 / m + torch.tensor(f32w(eps), dtype=dtype))


def _bn_dpre(y, dout, gamma, beta, mean, rstd, keep, act, scale, dtype):
    xh = (y.to(dtype) - mean.to(dtype)) * rstd.to(dtype)
    z = _act(act, xh * gamma.to(dtype) + beta.to(dtype))
    return dout.to(dtype) * _keepf(keep, scale, z, dtype) * _act_grad_from_out(act, z), xh


def ref_bn_bwd(y, dout, gamma, beta, mean, rstd, keep, act, training, m_total, scale=1.0, sums=None, dtype=F64):
    """dpre = dout * drop' * act'(z), the activation gradient formed from the recomputed output
    z (z > 0, or 1 - z * z); dbeta = sum_rows dpre, dgamma = sum_rows dpre * xh (these rows' own
    sums); dy = gamma * rstd * (dpre - Sb / m_total - xh * Sg / m_total) in training, where
    (Sb, Sg) = `sums` (SyncBatchNorm: the sums over all ranks' rows) or else (dbeta, dgamma);
    eval: dy = gamma * rstd * dpre.  Returns dy, dgamma, dbeta."""
    dp, xh = _bn_dpre(y, dout, gamma, beta, mean, rstd, keep, act, scale, dtype)
    dbeta, dgamma = dp.sum(0), (dp * xh).sum(0)
    gr = gamma.to(dtype) * rstd.to(dtype)
    if not training:
        return gr * dp, dgamma, dbeta
    sb, sg = (dbeta, dgamma) if sums is None else (sums[0].to(dtype), sums[1].to(dtype))
    return gr * (dp - sb / m_total - xh * sg / m_total), dgamma, dbeta


def _chunks(M, rows_per):
    return [(r0, min(M, r0 + rows_per)) for r0 in range(0, M, rows_per)]


def ref_bn_chunk_moments(y, rows_per, dtype=F64):
    """[R, 2, C]: (mean, M2 = sum (y - mean)^2) of each chunk of rows_per rows (a short last one)."""
    v = y.to(dtype)
    out = []
    for r0, r1 in _chunks(v.shape[0], rows_per):
        mu = v[r0:r1].sum(0) / (r1 - r0)
        out.append(torch.stack([mu, ((v[r0:r1] - mu) ** 2).sum(0)]))
    return torch.stack(out)


def ref_bn_bwd_chunk_sums(y, dout, gamma, beta, mean, rstd, keep, act, rows_per, scale=1.0, dtype=F64):
    """[R, 2, C]: (sum dpre, sum dpre * xh) of each chunk of rows_per rows."""
    dp, xh = _bn_dpre(y, dout, gamma, beta, mean, rstd, keep, act, scale, dtype)
    return torch.stack([torch.stack([dp[r0:r1].sum(0), (dp[r0:r1] * xh[r0:r1]).sum(0)])
                        for r0, r1 in _chunks(dp.shape[0], rows_per)])


def bn_rows_per(m):
    """The header's chunk rule: 64 rows, halved down to 8 while fewer than 256 chunks result."""
    rp = 64
    while rp > 8 and (m + rp - 1) // rp < 256:
        rp >>= 1
    return rp


def ln_bwd_blocks(m):
    """Work-groups (= partial rows) of the LayerNorm backward: 16+ rows each, at most 256."""
    return min(256, (m + 15) // 16)


# ------------------------------------------------- the non-exact yardstick
def worst_ratio_by(got, ref64, ref32, out_dtype=F32, dim=1, extra_abs=0.0, kind=None, pool=()):
    """_misc_refs.worst_ratio applied to every slice along `dim` on its own (dim = 1: per row of a
    [M, C] tensor, LayerNorm; dim = 0: per column, BatchNorm): max over elements of
    |got - ref64| / (max(4 * E32, 2 ulp(out_dtype at |ref64|)) + extra_abs), E32 = the worst
    float32-CPU error of the same reference over the element's own row (column).  One bad row
    cannot hide behind the others' errors.

    pool: the kinds (kind: one integer per slice) whose slices take the worst E32 over the
    slices of that kind instead of their own.  It is for slices whose elements share one draw of
    their largest error, the rounding of the slice's mean (a row or column at mean 1e3 x std; a
    column of a handful of rows): a single float32 evaluation may draw (nearly) zero there, the
    slices built to the same recipe draw again, and a bad slice still cannot hide behind slices
    of a worse-conditioned kind.  Every other slice is held to its own E32 (LN_POOL, bn_pool).
    Returns (ratio, index of the worst slice)."""
    g, r, r32 = (torch.as_tensor(a).to(F64).cpu() for a in (got, ref64, ref32))
    if r.numel() == 0:
        return 0.0, -1
    if dim == 0:
        g, r, r32 = g.t(), r.t(), r32.t()
        if torch.is_tensor(extra_abs):
            extra_abs = extra_abs.t()
    e32 = (r32 - r).abs().amax(1, keepdim=True)
    for k in pool:
        if (kind == k).any():
            e32[kind == k] = e32[kind == k].max()
    allowed = torch.maximum(2 * ulp(r, out_dtype), 4 * e32) + extra_abs
    err = (g - r).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = (err / allowed).amax(1)
    return ratio.max().item(), int(ratio.argmax())


FEW_ROWS = 16


def bn_pool(m):
    """The kinds worst_ratio_by pools for a BatchNorm tensor of m rows: all of them below FEW_ROWS
    rows, none otherwise.  Every element of a column carries the rounding of the column's mean
    and rstd; over a handful of rows that shared draw is the float32 reference's whole error and
    may come out (nearly) zero (a correct f32 model of the kernel shows 1.09 on one ordinary
    column of 9 x 8 against its own E32, and at most 0.70 on every larger shape and on every
    LayerNorm row, which are therefore held to their own E32)."""
    return (0, 1, 2) if m < FEW_ROWS else ()


# ------------------------------------- inputs and bars of the random-input tests
# The absolute error of fast_tanh (__expf, __fdividef), which the float32 CPU reference does not
# model.  Measured on the MI355X over the shapes of test_bn_random's act = tanh cases (f32, the
# ordinary columns, no residual or dropout, the reference given the device's mean and rstd, so that
# tanh's own error is what is left): worst |out - ref64| = 2.48 x 2^-24 (the float32 reference:
# 2.01); allowed 4 x that rounded up to a power of two.  The bar adds TANH_ABS * the dropout scale.
TANH_ABS = 16 * 2.0 ** -24


def ln_random(m, dtype, seed):
    """Rows of four kinds: ordinary; mean up to 1e3 x std (f32; 8 x std in bf16, whose grid has
    8 bits); constant (variance 0: a dyadic value, so that the row's f32 sums are exact in any
    order and y = beta is the only correct answer); and rows of magnitude 1e4 among rows of 1e-2."""
    g = torch.Generator().manual_seed(seed)
    LC = LN_C
    x = torch.randn(m, LC, generator=g)
    kind = torch.arange(m) % 4 if m > 4 else torch.zeros(m, dtype=torch.long)
    big = 1e3 if dtype == F32 else 8.0
    x[kind == 1] += big * torch.rand(int((kind == 1).sum()), 1, generator=g)
    x[kind == 2] = 3.25
    x[kind == 3] *= 1e-2
    if m > 7:
        x[7] *= 1e6   # one row of magnitude 1e4 among the small ones
    br = 0.5 * torch.randn(m, LC, generator=g)
    br[kind == 2] = 0
    gamma, beta = 1 + 0.1 * torch.randn(LC, generator=g), 0.1 * torch.randn(LC, generator=g)
    dy = torch.randn(m, LC, generator=g)
    return x.to(dtype), br.to(dtype), gamma, beta, dy.to(dtype), kind


def bn_random(m, c, dtype, seed):
    """y = randn * 3 + 1.5 with columns 0 and 2 at mean +-1e3 x std (bf16: +-1024 + 8 k, on bf16's
    own grid) and columns 1 and 3 constant; kinds 0 / 1 / 2 = ill-conditioned / constant /
    ordinary (columns 4 ...)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(m, c, generator=g) * 3 + 1.5
    for col, mu in ((0, 1000.0), (2, -1024.0)):
        if dtype == F32:
            y[:, col] = mu + torch.randn(m, generator=g)
        else:
            y[:, col] = (1024.0 if mu > 0 else -1024.0) + 8 * torch.randint(-3, 4, (m,), generator=g).float()
    y[:, 1], y[:, 3] = 0.7, -2.5
    kind = torch.full((c,), 2)
    kind[0] = kind[2] = 0
    kind[1] = kind[3] = 1
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    dout = torch.randn(m, c, generator=g)
    res = torch.randn(m, c + 16, generator=g)
    rm0, rv0 = 0.1 * torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g)
    return y.to(dtype), gamma, beta, dout.to(dtype), res.to(BF16), rm0, rv0, kind


def by_kind(worst, name, got, r64, r32, kind, extra=None):
    """A per-column (per-row) vector of scalars into worst[...] = (ratio, kind): worst_ratio over
    the columns of each kind (kind None: over the whole vector).  A scalar's own float32 error is
    a single draw; the columns built to the same recipe share its scale.  extra: an absolute
    term added to what is allowed (tanh_bwd_extra)."""
    groups = [(name, torch.ones(len(r64), dtype=torch.bool), -1)] if kind is None else \
        [(f"{name} kind {k}", kind == k, k) for k in kind.unique().tolist()]
    for key, sel, k in groups:
        if extra is None:
            worst[key] = (worst_ratio(got[sel], r64[sel], r32[sel]), k)
        else:
            g, r, r3 = got[sel].double(), r64[sel].double(), r32[sel].double()
            allowed = torch.clamp_min(2 * ulp(r, F32), 4 * (r3 - r).abs().max().item()) + extra[sel]
            worst[key] = (((g - r).abs() / allowed).max().item(), k)


def tanh_bwd_extra(y, dout, gamma, beta, mean, rstd, keep, scale, m_total):
    """First-order bound of what |z - tanh| <= TANH_ABS does to the backward: act' = 1 - z^2
    moves by at most 2 TANH_ABS, so dpre by e = 2 TANH_ABS |dout * drop|; dbeta by sum e, dgamma
    by sum e |xh|, dy by |gamma rstd| (e + sum e / M + |xh| sum e |xh| / M)."""
    kf = _keepf(keep, scale, None, F64)
    xh = ((y.double() - mean.double()) * rstd.double()).abs()
    e = 2 * TANH_ABS * (dout.double() * kf).abs()
    eb, eg = e.sum(0), (e * xh).sum(0)
    return (gamma.double() * rstd.double()).abs() * (e + eb / m_total + xh * eg / m_total), eg, eb


# ------------------------------------------------ exact-arithmetic problems
def _resolution(t):
    """The largest power of two of which every element of t (float64) is a multiple."""
    for k in range(0, 60):
        s = t * 2.0 ** k
        if torch.equal(s, s.round()):
            return 2.0 ** -k
    raise AssertionError("not a dyadic tensor")


def sum_is_exact(terms, dim=0):
    """sum |terms| / resolution < 2^24 for every sum along dim: every partial sum is then exact in
    f32 in any order.  Returns (ok, log2 of the worst sum |terms| / resolution)."""
    t = terms.to(F64)
    worst = (t.abs().sum(dim) / _resolution(t)).max().item()
    return worst < EXACT_LIMIT, float(np.log2(max(worst, 1.0)))


def is_f32(t):
    """Every element of the float64 tensor is representable in f32."""
    return torch.equal(t.to(F32).to(F64), t)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _choice(g, values, *shape):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def _pm_rows(g, m, c):
    """[m, c] of +-1, each row half +1 and half -1 in shuffled order."""
    base = torch.cat([torch.ones(c // 2), -torch.ones(c - c // 2)]).to(F64)
    return torch.stack([base[torch.randperm(c, generator=g)] for _ in range(m)]) if m else base[None][:0]


class LnBwdExact:
    """x + keep * branch - mean in {-1, 0, 1} with an integer mean, rstd in {1, 0.5}, dy in
    {-1, 0, 1}, gamma in {+-0.5, +-1, +-2}, dropout p = 0.5 (scale 2) or off, integer priors."""
    SEED, SITE = 77, 21

    def __init__(self, m, dtype, p, with_branch, grad_beta, mixed_rstd, seed=0):
        g = _gen(1000 * seed + m)
        C = LN_C
        self.m, self.dtype, self.p, self.grad_beta = m, dtype, p, grad_beta
        self.keep = keep_mask(self.SEED, self.SITE, m, C, p) if with_branch else None
        self.scale = drop_scale(p) if with_branch else 1.0
        self.mean = _ints(g, -3, 3, m)
        t = _ints(g, -1, 1, m, C)
        self.rstd = _choice(g, [1.0, 0.5], m) if mixed_rstd else torch.ones(m, dtype=F64)
        self.dy = _ints(g, -1, 1, m, C)
        self.gamma = _choice(g, [0.5, -0.5, 1, -1, 2, -2], C)
        s = self.mean[:, None] + t
        if with_branch:
            self.branch = _ints(g, -2, 2, m, C)
            self.x = s - self.branch * _keepf(self.keep, self.scale, s, F64)
        else:
            self.branch, self.x = None, s
        self.prior = [_ints(g, -4, 4, C) for _ in range(3)]   # dgamma, dbeta, dbias before the call
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = ref_ln_bwd(self.dy, self.x, self.branch, self.keep, self.gamma, self.mean, self.rstd,
                                   self.grad_beta, *self.prior, scale=self.scale)
        return self._ref

    def with_grad_beta(self, grad_beta):
        """The same problem accumulating onto its priors with another grad_beta (asserted exact)."""
        self.grad_beta, self._ref = grad_beta, None
        assert self.exact()[0], f"LnBwdExact(m={self.m}, grad_beta={grad_beta}) is not exact in f32"
        return self

    def exact(self):
        """(ok, worst log2): every product and output is an f32 value and every column sum (with
        its grad_beta * prior term) and row sum has sum |terms| / resolution < 2^24."""
        s = self.x if self.branch is None else self.x + self.branch * _keepf(self.keep, self.scale, self.x, F64)
        xh = (s - self.mean[:, None]) * self.rstd[:, None]
        gd = self.gamma * self.dy
        dx, dbr, dg, db, dd = self.ref()
        ok = all(is_f32(t) for t in (xh, gd, gd * xh, dx, dbr, dg, db, dd)) and float(self.scale) == int(self.scale)
        worst = 0.0
        for terms, prior, dim in ((gd, None, 1), (gd * xh, None, 1), (self.dy * xh, self.prior[0], 0),
                                  (self.dy, self.prior[1], 0), (dbr, self.prior[2], 0)):
            if prior is not None and self.grad_beta != 0:
                terms = torch.cat([terms, self.grad_beta * prior[None]])
            if terms.numel():
                o, w = sum_is_exact(terms, dim)
                ok, worst = ok and o, max(worst, w)
        return ok, worst


def ln_bwd_exact(m, dtype, p, with_branch, grad_beta=0.0, seed=0):
    """The mixed-rstd problem where its predicate holds (decided at grad_beta = 1, the largest
    prior term, so that every grad_beta of the tests sees the same problem), else rstd = 1."""
    pr = LnBwdExact(m, dtype, p, with_branch, 1.0, True, seed)
    if not pr.exact()[0]:
        pr = LnBwdExact(m, dtype, p, with_branch, 1.0, False, seed)
    return pr.with_grad_beta(grad_beta)


class LnFwdExact:
    """Every row of s = x + drop(branch) (or x + bias + sum slabs, ln_combine) is half K + 1 and
    half K - 1 with an integer K; eps = 3: mean = K, variance 1, rstd = 1 / sqrt(4) = 0.5;
    gamma a power of two, beta an integer."""
    SEED, SITE, EPS = 78, 22, 3.0

    def __init__(self, m, p=0.0, with_branch=False, splits=0, seed=0):
        g = _gen(2000 * seed + 10 * m + splits)
        C = LN_C
        self.m = m
        self.K = _ints(g, -8, 8, m)
        self.s = self.K[:, None] + _pm_rows(g, m, C)
        self.gamma = _choice(g, [1.0, -1.0, 2.0, -2.0, 4.0, 0.5], C)
        self.beta = _ints(g, -3, 3, C)
        self.keep = keep_mask(self.SEED, self.SITE, m, C, p) if with_branch else None
        self.scale = drop_scale(p) if with_branch else 1.0
        self.branch = self.parts = self.bias = None
        self.x = self.s
        if with_branch:
            self.branch = _ints(g, -2, 2, m, C)
            self.x = self.s - self.branch * _keepf(self.keep, self.scale, self.s, F64)
        if splits:
            self.parts = _ints(g, -2, 2, splits, m, C)
            self.bias = _ints(g, -3, 3, C)
            self.x = self.s - self.bias - self.parts.sum(0)

    def exact(self):
        d = self.s - self.K[:, None]
        ok = is_f32(self.x) and self.x.abs().max().item() <= 256 if self.m else True   # exact in bf16 / f16
        o1, w1 = sum_is_exact(self.s, 1) if self.m else (True, 0.0)
        o2, w2 = sum_is_exact(d * d, 1) if self.m else (True, 0.0)
        return bool(ok and o1 and o2 and torch.equal((d * d).sum(1), torch.full((self.m,), 512.0, dtype=F64))), max(w1, w2)


class BnFwdExact:
    """Integer y; every 8-row group of a column holds four K + 1 and four K - 1 in shuffled
    order.  design 1: one integer K per column (chunk moments exact in f32, mean K, variance 1);
    design 2: K + 2, K - 2, K + 2, ... per chunk of rows_per rows (0 in the last chunk of an odd
    count), so the chunk means differ and the double combine carries the variance: the sums stay
    exact integers in double.  eps = 3; gamma a power of two, beta and the residual integers."""
    SEED, SITE, EPS, MOM = 79, 23, 3.0, 0.1

    def __init__(self, m, c, design, p=0.0, with_res=False, res_ld=0, seed=0):
        assert m % 8 == 0
        g = _gen(3000 * seed + m + c + design)
        self.m, self.c, self.design = m, c, design
        self.rows_per = bn_rows_per(m)
        assert m % self.rows_per == 0
        K = _ints(g, -8, 8, c)
        base = torch.tensor([1.0, 1, 1, 1, -1, -1, -1, -1], dtype=F64)
        pm = base[torch.argsort(torch.rand(m // 8, c, 8, generator=g), dim=2)]       # [m / 8, c, 8]
        y = K[None] + pm.permute(0, 2, 1).reshape(m, c)
        R = m // self.rows_per
        if design == 2 and R > 1:
            off = torch.tensor([2.0 if r % 2 == 0 else -2.0 for r in range(R)], dtype=F64)
            if R % 2:
                off[-1] = 0
            y = y + off.repeat_interleave(self.rows_per)[:, None]
        self.y = y
        self.gamma = _choice(g, [1.0, -1.0, 2.0, -2.0, 4.0], c)
        self.beta = _ints(g, -3, 3, c)
        self.keep = keep_mask(self.SEED, self.SITE, m, c, p)
        self.scale = drop_scale(p)
        self.res_ld = res_ld or c
        self.res = _ints(g, -4, 4, m, self.res_ld) if with_res else None
        self.rm0, self.rv0 = _ints(g, -4, 4, c), _ints(g, 1, 4, c)

    def ref(self, act):
        return ref_bn_fwd(self.y, self.gamma, self.beta, self.keep, self.res, act, self.EPS, self.MOM, self.rm0,
                          self.rv0, True, scale=self.scale)

    def exact(self):
        """The shifted chunk sums of bn_stats_kernel (shift = the chunk's first row) are exact in
        f32, the chunk means are integers, the combine's sums are integers below 2^53, and (design
        1) mean = K, variance 1 and every product of the apply is an f32 value."""
        ok, worst = True, 0.0
        for r0 in range(0, self.m, self.rows_per):
            d = self.y[r0:r0 + self.rows_per] - self.y[r0]
            for t in (d, d * d):
                o, w = sum_is_exact(t, 0)
                ok, worst = ok and o, max(worst, w)
        mom = ref_bn_chunk_moments(self.y, self.rows_per)
        ok = ok and torch.equal(mom, mom.round()) and is_f32(mom)
        mu = self.y.sum(0) / self.m
        m2 = ((self.y - mu) ** 2).sum(0)
        ok = ok and torch.equal(mu, mu.round()) and torch.equal(m2, m2.round()) and m2.max().item() < 2.0 ** 53
        if self.design == 1:
            ok = ok and torch.equal(m2, torch.full_like(m2, float(self.m)))
            ok = ok and all(is_f32(self.ref(a)[0]) for a in (ACT_NONE, ACT_RELU))
        return bool(ok), worst


class BnBwdExact:
    """Given integer mean and rstd in {0.5, 1} per column, y = mean + {-2 .. 2}, dout in
    {-1, 0, 1}, gamma in {+-0.5, +-1, +-2}, integer beta in {-1, 0, 1}: pre-activations are
    multiples of 0.25, some exactly 0 and some on the other side of 0 from xh * gamma;
    M a power of two (1 / M exact), dropout p = 0.5 (scale 2) or off."""
    SEED, SITE = 80, 24

    def __init__(self, m, c, p=0.0, seed=0):
        g = _gen(4000 * seed + m + c)
        self.m, self.c = m, c
        self.mean = _ints(g, -4, 4, c)
        self.rstd = _choice(g, [0.5, 1.0], c)
        self.y = self.mean[None] + _ints(g, -2, 2, m, c)
        self.dout = _ints(g, -1, 1, m, c)
        self.gamma = _choice(g, [0.5, -0.5, 1, -1, 2, -2], c)
        self.beta = _ints(g, -1, 1, c)
        self.keep = keep_mask(self.SEED, self.SITE, m, c, p)
        self.scale = drop_scale(p)

    def ref(self, act, training):
        return ref_bn_bwd(self.y, self.dout, self.gamma, self.beta, self.mean, self.rstd, self.keep, act, training,
                          self.m, scale=self.scale)

    def exact(self):
        xh = (self.y - self.mean) * self.rstd
        a = xh * self.gamma
        pre = a + self.beta
        ok = bool((pre == 0).any()) and bool((a * pre < 0).any())       # zeros, and sign changes by beta
        ok = ok and (self.m & (self.m - 1)) == 0
        worst = 0.0
        for act in (ACT_NONE, ACT_RELU):
            dp, _ = _bn_dpre(self.y, self.dout, self.gamma, self.beta, self.mean, self.rstd, self.keep, act,
                             self.scale, F64)
            for t in (dp, dp * xh):
                o, w = sum_is_exact(t, 0)
                ok, worst = ok and o, max(worst, w)
            db, dg = dp.sum(0), (dp * xh).sum(0)
            inner = dp - db / self.m - xh * dg / self.m
            ok = ok and all(is_f32(t) for t in (xh * dg, db / self.m, xh * dg / self.m, dp - db / self.m, inner,
                                                self.gamma * self.rstd * inner))
        return bool(ok), worst
