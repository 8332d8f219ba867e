"""tests/_norm_refs.py against independent evaluations (torch.nn.functional.layer_norm /
batch_norm and autograd, in float64), and the proof that the bars of tests/test_gpu_norm_exact.py
bite: a small numpy model of each kernel family in f32 arithmetic -- LayerNorm by rows (8
sequential values per lane, then a tree over the 64 lanes), BatchNorm by rows_per chunks with the
first-row shift and the double-precision combine -- written here from the header and taken from no
kernel, passes the bit-exact problems and the per-row / per-column float64 bars on the inputs the
GPU tests use, and fifteen deliberately wrong copies of it do not (CPU only)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _misc_refs as MR
import _norm_refs as R
from _norm_refs import ACT_NONE, ACT_RELU, ACT_TANH, BF16, F32, F64

f32 = np.float32


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("m,p", [(5, 0.0), (37, 0.3)])
def test_ln_refs_are_torch(m, p):
    g = torch.Generator().manual_seed(m)
    C = R.LN_C
    x, br, dy = (torch.randn(m, C, generator=g, dtype=F64) for _ in range(3))
    gamma, beta = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    keep, scale = R.keep_mask(3, 4, m, C, p), R.drop_scale(p)
    xr, brr, gr, ber = (t.clone().requires_grad_(True) for t in (x, br, gamma, beta))
    s = xr + (brr * keep * scale if keep is not None else brr)
    eps = R.f32w(1e-5)
    yr = F.layer_norm(s, (C,), gr, ber, eps=eps)
    yr.backward(dy)
    y, mean, rstd = R.ref_ln_fwd(x, br, keep, gamma, beta, 1e-5, scale=scale)
    prior = [torch.randn(C, generator=g, dtype=F64) for _ in range(3)]
    dx, dbr, dg, db, dd = R.ref_ln_bwd(dy, x, br, keep, gamma, mean, rstd, 0.5, *prior, scale=scale)

    def rel(a, b):
        return ((a - b).abs().max() / b.abs().max()).item()
    sd = s.detach()
    assert rel(y, yr.detach()) < 1e-12 and rel(mean, sd.mean(1)) < 1e-12
    assert rel(rstd, 1 / torch.sqrt(sd.var(1, unbiased=False) + eps)) < 1e-12
    assert rel(dx, xr.grad) < 1e-12 and rel(dbr, brr.grad) < 1e-12
    assert rel(dg, 0.5 * prior[0] + gr.grad) < 1e-12 and rel(db, 0.5 * prior[1] + ber.grad) < 1e-12
    assert rel(dd, 0.5 * prior[2] + brr.grad.sum(0)) < 1e-12
    dg0 = R.ref_ln_bwd(dy, x, br, keep, gamma, mean, rstd, 0.0, *prior, scale=scale)[2]
    assert rel(dg0, gr.grad) < 1e-12                          # grad_beta 0 ignores the prior
    # ln_combine = LN of x + bias + the slab sum
    parts = torch.randn(4, m, C, generator=g, dtype=F64)
    yc = R.ref_ln_combine(x, parts, beta, gamma, beta, 1e-5)
    assert rel(yc, F.layer_norm(x + beta + parts.sum(0), (C,), gamma, beta, eps=eps)) < 1e-12
    # the float32 evaluation is the same function, a float32 away
    y32 = R.ref_ln_fwd(x.float(), br.float(), keep, gamma.float(), beta.float(), 1e-5, scale=scale, dtype=F32)[0]
    assert y32.dtype == F32 and 0 < rel(y32.double(), y) < 1e-4


@pytest.mark.parametrize("m,c,act", [(9, 16, ACT_TANH), (70, 40, ACT_RELU)])
def test_bn_refs_are_torch(m, c, act):
    g = torch.Generator().manual_seed(m + c)
    y = torch.randn(m, c, generator=g, dtype=F64) * 3 + 1.5
    dout = torch.randn(m, c, generator=g, dtype=F64)
    gamma, beta = torch.randn(c, generator=g, dtype=F64), 0.3 * torch.randn(c, generator=g, dtype=F64)
    res = torch.randn(m, c + 8, generator=g, dtype=F64)
    rm0, rv0 = torch.randn(c, generator=g, dtype=F64), torch.rand(c, generator=g, dtype=F64) + 0.5
    p = 0.2
    keep, scale = R.keep_mask(5, 6, m, c, p), R.drop_scale(p)
    eps, mom = R.f32w(1e-5), R.f32w(0.1)

    def rel(a, b):
        return ((a - b).abs().max() / b.abs().max()).item()
    for training in (True, False):
        yr, gr, ber = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
        rm, rv = rm0.clone(), rv0.clone()
        z = F.batch_norm(yr, rm, rv, gr, ber, training=training, momentum=mom, eps=eps)
        z = z.relu() if act == ACT_RELU else z.tanh()
        o = z * keep * scale + res[:, :c]
        o.backward(dout)
        out, mean, rstd, nrm, nrv = R.ref_bn_fwd(y, gamma, beta, keep, res, act, 1e-5, 0.1, rm0, rv0, training,
                                                 scale=scale)
        assert rel(out, o.detach()) < 1e-12 and rel(nrm, rm) < 1e-12 and rel(nrv, rv) < 1e-12
        if training:
            assert rel(mean, y.mean(0)) < 1e-12 and rel(rstd, 1 / torch.sqrt(y.var(0, unbiased=False) + eps)) < 1e-12
        dy, dg, db = R.ref_bn_bwd(y, dout, gamma, beta, mean, rstd, keep, act, training, m, scale=scale)
        assert rel(dy, yr.grad) < 1e-12 and rel(dg, gr.grad) < 1e-12 and rel(db, ber.grad) < 1e-12
        assert torch.equal(out, R.ref_bn_apply(y, mean, rstd, gamma, beta, keep, res, act, scale=scale))
    # chunk moments / sums recombine to the whole
    out, mean, rstd, _, _ = R.ref_bn_fwd(y, gamma, beta, keep, res, act, 1e-5, 0.1, rm0, rv0, True, scale=scale)
    mu, m2, rs = R.ref_bn_combine(R.ref_bn_chunk_moments(y, 8), 8, m, 1e-5)
    assert rel(mu, mean) < 1e-12 and rel(rs, rstd) < 1e-12 and rel(m2, ((y - mean) ** 2).sum(0)) < 1e-12
    sums = R.ref_bn_bwd_chunk_sums(y, dout, gamma, beta, mean, rstd, keep, act, 8, scale=scale)
    dy, dg, db = R.ref_bn_bwd(y, dout, gamma, beta, mean, rstd, keep, act, True, m, scale=scale)
    assert rel(sums[:, 0].sum(0), db) < 1e-12 and rel(sums[:, 1].sum(0), dg) < 1e-12
    # M = 1: the reference, not torch (which refuses it), defines it: variance 0 in both places
    o1 = R.ref_bn_fwd(y[:1], gamma, beta, None, None, ACT_NONE, 1e-5, 0.1, rm0, rv0, True)
    assert torch.equal(o1[1], y[0]) and torch.allclose(o1[0][0], beta) and rel(o1[4], (1 - mom) * rv0) < 1e-12
    assert R.bn_rows_per(2056) == 8 and R.bn_rows_per(4100) == 16 and R.bn_rows_per(12800) == 32
    assert R.bn_rows_per(16320) == 32 and R.bn_rows_per(16384) == 64 and R.bn_rows_per(1) == 8


def test_worst_ratio_by_is_per_slice():
    """One bad row among good ones: the whole-tensor rule lets it through when another row's
    float32 error is large, the per-row rule does not."""
    ref = torch.ones(4, 8, dtype=F64)
    r32 = ref.clone()
    r32[0, 0] += 1e-3                       # a row whose float32 evaluation is poor
    got = ref.clone()
    got[2, 5] += 2e-3                       # an error in another row
    assert MR.worst_ratio(got, ref, r32) < 1
    ratio, row = R.worst_ratio_by(got, ref, r32)
    assert ratio > 1000 and row == 2
    assert R.worst_ratio_by(got.t(), ref.t(), r32.t(), dim=0) == (ratio, 2)
    got[2, 5] = float("nan")
    assert R.worst_ratio_by(got, ref, r32)[0] == float("inf")


# ------------------------------------------------------------------ the kernel model
def keepf(keep, scale, shape, shift=0):
    """f32 dropout factors; shift: the mask hashed one element further on (a mutant)."""
    if keep is None:
        return np.ones(shape, f32)
    k = keep.numpy().reshape(-1)
    if shift:
        k = np.concatenate([k[shift:], k[:shift]])
    return np.where(k.reshape(shape), f32(scale), f32(0))


def wave_sum(v):
    """[M, 512] f32 -> [M]: 8 sequential adds per lane, then a halving tree over the 64 lanes."""
    v = v.reshape(v.shape[0], 64, 8)
    s = np.zeros(v.shape[:2], f32)
    for j in range(8):
        s = s + v[:, :, j]
    while s.shape[1] > 1:
        s = s[:, ::2] + s[:, 1::2]
    return s[:, 0]


def seq_sum(v, groups):
    """Column sums of [M, C] f32 as `groups` strided partial sums added in order."""
    acc = np.zeros((groups, v.shape[1]), f32)
    for r in range(v.shape[0]):
        acc[r % groups] = acc[r % groups] + v[r]
    t = np.zeros(v.shape[1], f32)
    for gi in range(groups):
        t = t + acc[gi]
    return t


def n32(t):
    return None if t is None else t.float().numpy()


def ln_fwd_model(x, branch, keep, gamma, beta, eps, scale=1.0, mut=None):
    s = n32(x).copy()
    if branch is not None:
        s = s + n32(branch) * keepf(keep, scale, s.shape)
    C = f32(s.shape[1])
    mean = wave_sum(s) / C
    if mut == "one_pass":
        var = wave_sum(s * s) / C - mean * mean
    else:
        d = s - mean[:, None]
        var = wave_sum(d * d) / C
    rstd = (f32(1) / np.sqrt(var + f32(eps))).astype(f32)
    y = (s - mean[:, None]) * rstd[:, None] * n32(gamma) + n32(beta)
    return y, mean, rstd


def ln_bwd_model(dy, x, branch, keep, gamma, mean, rstd, grad_beta, prior, scale=1.0, mut=None):
    """Rows in work-groups of ceil(M / nb) rows; the work-groups' column partials summed in order."""
    s, dy = n32(x).copy(), n32(dy)
    M, Cn = s.shape
    kf = keepf(keep, scale, s.shape, shift=1 if mut == "keep_shift" else 0)
    if branch is not None:
        s = s + n32(branch) * kf
    C = f32(Cn - 1 if mut == "c_minus_1" else Cn)
    rs = n32(rstd)[:, None]
    xh = (s - n32(mean)[:, None]) * rs
    gd = n32(gamma) * dy
    c1, c2 = wave_sum(gd) / C, wave_sum(gd * xh) / C
    ds = rs * (gd - c1[:, None] - xh * c2[:, None])
    dbr = ds * kf
    if mut == "keep_on_dx":
        ds, dbr = dbr, ds
    live = np.ones(M, bool)
    if mut == "skip_last_row":
        live[-1] = False
        ds[-1] = dbr[-1] = 0
    nb = R.ln_bwd_blocks(M)
    outs = []
    for terms, p0 in ((dy * xh, prior[0]), (dy, prior[1]), (dbr, prior[2])):
        parts = [seq_sum(terms[b::nb][live[b::nb]], 1) for b in range(nb)]
        if mut == "drop_partial":
            parts = parts[:-1]
        v = seq_sum(np.stack(parts), 4) if parts else np.zeros(Cn, f32)
        gb = 0.0 if mut == "grad_beta_ignored" else grad_beta
        outs.append(f32(gb) * n32(p0) + v if gb != 0 else v)
    return (ds, dbr, *outs)


def bn_moments_model(y, rows_per, mut=None):
    """[R, 2, C] chunk (mean, M2) from f32 sums shifted by the chunk's first row k.  The mean is
    kept as the pair (k, S1 / n) of f32 values (returned here as their float64 sum), which the
    combine rounds to one f32, or adds in double for a column whose mean dwarfs its spread."""
    v = n32(y)
    out = []
    for r0 in range(0, v.shape[0], rows_per):
        ch = v[r0:r0 + rows_per]
        k = np.zeros_like(ch[0]) if mut == "no_shift" else ch[0]
        d = ch - k
        s1, s2, n = seq_sum(d, 4), seq_sum(d * d, 4), f32(ch.shape[0])
        mean = k + s1 / n if mut == "no_shift" else k.astype(np.float64) + s1 / n
        out.append(np.stack([mean, np.maximum(s2 - s1 * s1 / n, f32(0))]))
    return np.stack(out)


def bn_finalize_model(part, rows_per, M, eps, mom, rm0, rv0, mut=None, counts=None):
    """The double-precision combine; counts: the chunks' row counts (default: rows_per, a short
    last chunk)."""
    part = part.astype(np.float64)
    if counts is None:
        counts = [min(rows_per, M - r0) for r0 in range(0, M, rows_per)]
        if mut == "short_chunk_full":
            counts[-1] = rows_per
    n = np.array(counts, np.float64)[:, None]

    def combine(means):
        mu = (n * means).sum(0) / M
        return mu, (part[:, 1] + n * (means - mu) ** 2).sum(0)
    mu, m2 = combine(part[:, 0].astype(f32).astype(np.float64))      # each chunk mean as one f32
    ill = mu * mu * M > 64 * m2                                         # |mean| > 8 sigma: in double
    if mut != "abs_mean_f32" and ill.any():
        mu_x, m2_x = combine(part[:, 0])
        mu, m2 = np.where(ill, mu_x, mu), np.where(ill, m2_x, m2)
    var = m2 / M
    unb = var if (M == 1 or mut == "biased_running") else m2 / (M - 1)
    mo = float(f32(mom))
    a, b = (mo, 1 - mo) if mut == "momentum_swapped" else (1 - mo, mo)
    return (mu.astype(f32), (1 / np.sqrt(var + float(f32(eps)))).astype(f32),
            (a * rm0.double().numpy() + b * mu).astype(f32), (a * rv0.double().numpy() + b * unb).astype(f32))


def act_model(act, v):
    return np.maximum(v, f32(0)) if act == ACT_RELU else (np.tanh(v).astype(f32) if act == ACT_TANH else v)


def bn_apply_model(y, mean, rstd, gamma, beta, keep, res, act, scale=1.0):
    z = act_model(act, (n32(y) - mean) * rstd * n32(gamma) + n32(beta))
    z = z * keepf(keep, scale, z.shape)
    return z + n32(res)[:, :z.shape[1]] if res is not None else z


def bn_fwd_model(y, gamma, beta, keep, res, act, eps, mom, rm0, rv0, rows_per, scale=1.0, mut=None):
    M = y.shape[0]
    mean, rstd, rm, rv = bn_finalize_model(bn_moments_model(y, rows_per, mut), rows_per, M, eps, mom, rm0, rv0, mut)
    return bn_apply_model(y, mean, rstd, gamma, beta, keep, res, act, scale), mean, rstd, rm, rv


def bn_bwd_model(y, dout, gamma, beta, mean, rstd, keep, act, training, m_total, rows_per, scale=1.0, mut=None,
                 sums=None):
    v, g, mu, rs = n32(y), n32(gamma), n32(mean), n32(rstd)
    xh = (v - mu) * rs
    pre = xh * g + n32(beta)
    z = act_model(act, pre)
    if act == ACT_RELU:
        grad = ((xh * g if mut == "relu_from_input" else z) > 0).astype(f32)
    else:
        grad = f32(1) - z * z if act == ACT_TANH else np.ones_like(z)
    dp = n32(dout) * keepf(keep, scale, z.shape) * grad
    chunks = [(seq_sum(dp[r0:r0 + rows_per], 4), seq_sum((dp * xh)[r0:r0 + rows_per], 4))
              for r0 in range(0, v.shape[0], rows_per)]
    db, dg = seq_sum(np.stack([c[0] for c in chunks]), 4), seq_sum(np.stack([c[1] for c in chunks]), 4)
    sb, sg = (db, dg) if sums is None else sums
    inv = f32(1) / f32(v.shape[0] if mut == "local_m" else m_total)
    if training or mut == "eval_subtracts":
        dy = g * rs * (dp - sb * inv - xh * sg * inv)
    else:
        dy = g * rs * dp
    return dy, dg, db


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def eq(model, ref64, dtype=F32):
    """The exact bar: the model's f32 result, cast to the output type, equals the reference cast."""
    return torch.equal(torch.from_numpy(np.asarray(model, f32)).to(dtype), ref64.to(dtype))


# ------------------------------------------------------------------ the bars on model and mutants
LN_BWD_MUTANTS = ["c_minus_1", "keep_on_dx", "keep_shift", "drop_partial", "skip_last_row", "grad_beta_ignored"]


def _ln_bwd_exact_ok(pr, mut):
    got = ln_bwd_model(pr.dy, pr.x, pr.branch, pr.keep, pr.gamma, pr.mean, pr.rstd, pr.grad_beta, pr.prior, pr.scale, mut)
    return all(eq(g, r, pr.dtype if i < 2 else F32) for i, (g, r) in enumerate(zip(got, pr.ref())))


@pytest.mark.parametrize("m", [5, 37, 272])
def test_ln_bwd_exact_bar_bites(m):
    """test_ln_bwd_exact's problem (p = 0.5, branch, grad_beta = 0.5): the model is bit-equal in
    f32 and bf16, each LayerNorm-backward mutant is not."""
    for dtype in (F32, BF16):
        pr = R.ln_bwd_exact(m, dtype, 0.5, True, 0.5)
        assert _ln_bwd_exact_ok(pr, None)
        for mut in LN_BWD_MUTANTS:
            assert not _ln_bwd_exact_ok(pr, mut), f"{mut} passes the exact LayerNorm backward at m = {m}"
    pr = R.ln_bwd_exact(m, F32, 0.0, False, 0.0)
    assert _ln_bwd_exact_ok(pr, None)


def test_ln_bwd_exact_fallback():
    """Mixed rstd where the predicate allows it (small M), rstd = 1 at 4100 rows, always exact."""
    assert (R.ln_bwd_exact(272, F32, 0.5, True).rstd != 1).any()
    for m in (3100, 4100):
        for p, br in ((0.5, True), (0.0, True), (0.0, False)):
            for gb in (0.0, 1.0, 0.5):
                assert R.ln_bwd_exact(m, F32, p, br, gb).exact()[0]
    assert not (R.ln_bwd_exact(4100, F32, 0.0, True).rstd != 1).any()
    assert not R.LnBwdExact(4100, F32, 0.0, True, 0.0, True).exact()[0]


def test_ln_fwd_exact_and_random_bars():
    """The model is bit-equal on the exact forward problems (and on ln_combine's), passes the
    per-row bar on test_ln_random_per_row's rows, and the one-pass variance (which the exact
    problem cannot see: its squares are exact) fails that bar on the rows with a large mean."""
    for p, br, splits in ((0.5, True, 0), (0.0, False, 0), (0.0, False, 16)):
        pr = R.LnFwdExact(37, p, br, splits)
        assert pr.exact()[0]
        if splits:
            x = torch.from_numpy(n32(pr.x) + (n32(pr.bias) + n32(pr.parts).sum(0)))
            ref = R.ref_ln_combine(pr.x, pr.parts, pr.bias, pr.gamma, pr.beta, pr.EPS)
        else:
            x, ref = pr.x, R.ref_ln_fwd(pr.x, pr.branch, pr.keep, pr.gamma, pr.beta, pr.EPS, scale=pr.scale)[0]
        y, mean, rstd = ln_fwd_model(x, pr.branch, pr.keep, pr.gamma, pr.beta, pr.EPS, pr.scale)
        assert eq(y, ref) and eq(y, ref, BF16) and eq(mean, pr.K) and eq(rstd, torch.full((37,), 0.5, dtype=F64))
    m, p = 37, 0.1
    x, br, gamma, beta, dy, kind = R.ln_random(m, F32, m)
    keep, scale = R.keep_mask(5, 17, m, R.LN_C, p), R.drop_scale(p)
    r64 = R.ref_ln_fwd(x, br, keep, gamma, beta, 1e-5, scale=scale)
    r32 = R.ref_ln_fwd(x, br, keep, gamma, beta, 1e-5, scale=scale, dtype=F32)
    got = ln_fwd_model(x, br, keep, gamma, beta, 1e-5, scale)
    assert R.worst_ratio_by(t64(got[0]), r64[0], r32[0])[0] <= 1
    worst = {}
    R.by_kind(worst, "mean", t64(got[1]), r64[1], r32[1], kind)
    R.by_kind(worst, "rstd", t64(got[2]), r64[2], r32[2], kind)
    assert max(v[0] for v in worst.values()) <= 1, worst
    bad = ln_fwd_model(x, br, keep, gamma, beta, 1e-5, scale, "one_pass")
    ratio, row = R.worst_ratio_by(t64(bad[0]), r64[0], r32[0])
    assert ratio > 1 and kind[row] == 1
    # the backward model on the same rows, with the model's statistics
    mean, rstd = torch.from_numpy(got[1]), torch.from_numpy(got[2])
    prior = [torch.zeros(R.LN_C)] * 3
    b64 = R.ref_ln_bwd(dy, x, br, keep, gamma, mean, rstd, scale=scale)
    b32 = R.ref_ln_bwd(dy, x, br, keep, gamma, mean, rstd, scale=scale, dtype=F32)
    gb = ln_bwd_model(dy, x, br, keep, gamma, mean, rstd, 0.0, prior, scale)
    assert R.worst_ratio_by(t64(gb[0]), b64[0], b32[0])[0] <= 1
    assert R.worst_ratio_by(t64(gb[1]), b64[1], b32[1])[0] <= 1
    assert all(MR.worst_ratio(t64(gb[i]), b64[i], b32[i]) <= 1 for i in (2, 3, 4))
    # one zeroed row fails the per-row bar, at that row
    y1 = got[0].copy()
    y1[11] = 0
    assert R.worst_ratio_by(t64(y1), r64[0], r32[0])[1] == 11 and R.worst_ratio_by(t64(y1), r64[0], r32[0])[0] > 1


BN_FWD_MUTANTS_EXACT = ["biased_running", "momentum_swapped"]


@pytest.mark.parametrize("m,c", [(64, 80), (136, 512), (4096, 8)])
@pytest.mark.parametrize("design", [1, 2])
def test_bn_fwd_exact_bar_bites(m, c, design):
    """test_bn_train_fwd_exact's problem: the model's mean, rstd, running statistics (and design
    1's out) are bit-equal; a biased running variance and a swapped momentum are not."""
    pr = R.BnFwdExact(m, c, design, 0.5, True, c + 8)
    assert pr.exact()[0]
    ref = pr.ref(ACT_RELU)

    def ok(mut):
        got = bn_fwd_model(pr.y, pr.gamma, pr.beta, pr.keep, pr.res, ACT_RELU, pr.EPS, pr.MOM, pr.rm0, pr.rv0,
                           pr.rows_per, pr.scale, mut)
        return all(eq(got[i], ref[i]) for i in ((0, 1, 2, 3, 4) if design == 1 else (1, 2, 3, 4)))
    assert ok(None)
    for mut in BN_FWD_MUTANTS_EXACT:
        assert not ok(mut), f"{mut} passes the exact BatchNorm forward"


@pytest.mark.parametrize("m,c", [(8, 8), (64, 80), (1024, 520)])
def test_bn_bwd_exact_bar_bites(m, c):
    """test_bn_bwd_exact's problem: the model is bit-equal in training and eval; the relu gradient
    taken from the input's sign and an eval backward that subtracts the batch terms are not."""
    pr = R.BnBwdExact(m, c, 0.5)
    assert pr.exact()[0]
    rp = R.bn_rows_per(m)

    def ok(training, mut):
        got = bn_bwd_model(pr.y, pr.dout, pr.gamma, pr.beta, pr.mean, pr.rstd, pr.keep, ACT_RELU, training, m, rp,
                           pr.scale, mut)
        return all(eq(g, r) and eq(g, r, BF16) for g, r in zip(got, pr.ref(ACT_RELU, training)))
    assert ok(True, None) and ok(False, None)
    assert not ok(True, "relu_from_input") and not ok(False, "relu_from_input")
    assert not ok(False, "eval_subtracts")


def _bn_random_ratios(m, c, act, mut):
    SEED, SITE, p = 7, 33, 0.2
    y, gamma, beta, dout, res, rm0, rv0, kind = R.bn_random(m, c, F32, m + c + act)
    keep, scale = R.keep_mask(SEED, SITE, m, c, p), R.drop_scale(p)
    args = (y, gamma, beta, keep, res, act, 1e-5, 0.1, rm0, rv0, True)
    r64, r32 = R.ref_bn_fwd(*args, scale=scale), R.ref_bn_fwd(*args, scale=scale, dtype=F32)
    got = bn_fwd_model(y, gamma, beta, keep, res, act, 1e-5, 0.1, rm0, rv0, R.bn_rows_per(m), scale, mut)
    worst = {"out": R.worst_ratio_by(t64(got[0]), r64[0], r32[0], dim=0, kind=kind, pool=R.bn_pool(m))}
    for i, n in ((1, "mean"), (2, "rstd"), (3, "run_mean"), (4, "run_var")):
        R.by_kind(worst, n, t64(got[i]), r64[i], r32[i], kind)
    mean, rstd = torch.from_numpy(got[1]), torch.from_numpy(got[2])
    bargs = (y, dout, gamma, beta, mean, rstd, keep, act, True, m)
    b64, b32 = R.ref_bn_bwd(*bargs, scale=scale), R.ref_bn_bwd(*bargs, scale=scale, dtype=F32)
    gb = bn_bwd_model(*bargs, R.bn_rows_per(m), scale)
    worst["dy"] = R.worst_ratio_by(t64(gb[0]), b64[0], b32[0], dim=0, kind=kind, pool=R.bn_pool(m))
    R.by_kind(worst, "dgamma", t64(gb[1]), b64[1], b32[1], None)
    R.by_kind(worst, "dbeta", t64(gb[2]), b64[2], b32[2], None)
    return worst


@pytest.mark.parametrize("m,c,act", [(1, 8, ACT_RELU), (7, 8, ACT_TANH), (9, 8, ACT_NONE), (2051, 8, ACT_TANH),
                                     (333, 80, ACT_NONE)])
def test_bn_random_bar_bites(m, c, act):
    """test_bn_random's inputs: the model passes every per-column bar (without any tanh term: it
    evaluates tanh in f32); chunk moments without the first-row shift fail on the columns at
    mean 1e3 x std, and a short last chunk weighted as a full one fails wherever there is one.

    Chunk means rounded to one f32 in every column (abs_mean_f32) fail too, on rstd of the columns at mean
    1e3 x std wherever there is more than one chunk: the rounding, up to ulp(1e3) / 2 = 3e-5,
    enters the combine's between-chunk term n_c (mean_c - mean)^2 to first order, which no f32
    two-pass evaluation does (ratios 62.6 at 9 x 8, 15.4 at 333 x 80, 4.9 at 2051 x 8).  The
    kernel stored its chunk means that way until these tests showed it."""
    worst = _bn_random_ratios(m, c, act, None)
    assert max(v[0] for v in worst.values()) <= 1, {k: v for k, v in worst.items() if v[0] > 1}
    if m > R.bn_rows_per(m):
        bad = _bn_random_ratios(m, c, act, "abs_mean_f32")
        assert bad["rstd kind 0"][0] > 1
    if m > 1:
        bad = _bn_random_ratios(m, c, act, "no_shift")
        assert bad["out"][0] > 1 and bad["out"][1] in (0, 2) and bad["rstd kind 0"][0] > 100
    if m % R.bn_rows_per(m):
        bad = _bn_random_ratios(m, c, act, "short_chunk_full")
        assert bad["mean kind 2"][0] > 1 and bad["out"][0] > 1


def test_syncbn_bar_bites():
    """Three ranks of unequal rows (test_syncbn_three_ranks): dy from the global sums and
    1 / m_total passes the per-column bar on every rank; 1 / M from the rank's own rows fails."""
    c, act, Ms = 80, ACT_RELU, (96, 1201, 7)
    m = sum(Ms)
    y, gamma, beta, dout, _, rm0, rv0, kind = R.bn_random(m, c, F32, c + act)
    mean, rstd = (t.float() for t in R.ref_bn_fwd(y, gamma, beta, None, None, act, 1e-5, 0.1, rm0, rv0, True)[1:3])
    bargs = (y, dout, gamma, beta, mean, rstd, None, act, True, m)
    b64, b32 = R.ref_bn_bwd(*bargs), R.ref_bn_bwd(*bargs, dtype=F32)
    off = [0, Ms[0], Ms[0] + Ms[1], m]
    local = [bn_bwd_model(y[off[r]:off[r + 1]], dout[off[r]:off[r + 1]], gamma, beta, mean, rstd, None, act, True, m, 8)
             for r in range(3)]
    sums = (local[0][2] + local[1][2] + local[2][2], local[0][1] + local[1][1] + local[2][1])
    for r in range(3):
        sl = slice(off[r], off[r + 1])
        for mut, passes in ((None, True), ("local_m", False)):
            dy = bn_bwd_model(y[sl], dout[sl], gamma, beta, mean, rstd, None, act, True, m, 8, mut=mut, sums=sums)[0]
            assert (R.worst_ratio_by(t64(dy), b64[0][sl], b32[0][sl], dim=0, kind=kind, pool=R.bn_pool(Ms[r]))[0] <= 1) == passes, (r, mut)
