"""Every kernel of csrc/layernorm.hip and csrc/batchnorm.hip
against the float64 references of tests/_norm_refs.py (validated
on the CPU, with mutants, by tests/test_norm_refs.py), through the C ABI so that every field of
tt2_ln_args / tt2_bn_args can be set (grad_beta, training = 0, out_dtype, res_dtype, stats_rows).

  * bit-exact problems (torch.equal to the float64 reference cast to the output type): inputs
    whose every product is an f32 value and whose every sum has sum |terms| / resolution < 2^24,
    asserted by the builders' predicates before each launch; a skipped, doubled or misplaced row,
    chunk, partial or divisor has no tolerance to hide behind;
  * random, ill-conditioned inputs held per LayerNorm row and per BatchNorm column:
    |got - ref64| <= max(4 x the float32-CPU error of the same reference over that row / column,
    2 ulp of the output type) (_norm_refs.worst_ratio_by <= 1).  The float32 error is the row's
    (column's) own; only a BatchNorm tensor of fewer than 16 rows takes the worst over its columns
    of the same kind (_norm_refs.bn_pool says why).  Per-row / per-column scalars (mean, rstd,
    running statistics) are held with _misc_refs.worst_ratio over the rows / columns of one kind,
    dgamma / dbeta / dbias over the whole vector; the ratios are printed (pytest -s);
  * every output NaN-filled inside guard bands, inputs followed by NaN rows, and the argument
    rejections leaving the poison untouched."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import _misc_refs as MR  # noqa: E402
import _norm_refs as R  # noqa: E402
from _norm_refs import ACT_NONE, ACT_RELU, ACT_TANH, BF16, F16, F32, F64  # noqa: E402
from tt2 import _lib, ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")
GR = 3          # guard rows of a 2-D buffer (a row is C % 8 == 0 elements: a multiple of 16 bytes)
G1 = 4          # guard elements of a 1-D f32 buffer: 16 bytes
LC = R.LN_C


class Guarded:
    """A NaN-filled device buffer with guard bands (rows of a 2-D output, 16 bytes of a 1-D one)
    on both sides of the view `v` a kernel is given."""

    def __init__(self, shape, dtype=F32):
        self.g = GR if len(shape) == 2 else G1
        self.n = shape[0]
        self.buf = torch.full((shape[0] + 2 * self.g,) + tuple(shape[1:]), NAN, dtype=dtype, device=DEV)
        self.v = self.buf[self.g:self.g + self.n]

    def ptr(self):
        return self.v.data_ptr()

    def check(self, what):
        b = self.buf.float().cpu()
        assert not torch.isnan(b[self.g:self.g + self.n]).any(), f"{what}: NaN left inside the logical extent"
        assert torch.isnan(b[:self.g]).all() and torch.isnan(b[self.g + self.n:]).all(), f"{what}: guard written"

    def untouched(self, what):
        assert torch.isnan(self.buf.float().cpu()).all(), f"{what}: written"

    def cpu(self):
        return self.v.cpu()


KEEP = []   # every device input and workspace of the running test: the args structs hold raw pointers


@pytest.fixture(autouse=True)
def _keep_inputs_alive():
    yield
    torch.cuda.synchronize()
    KEEP.clear()


def inp(t, dtype=F32):
    """t on the device in `dtype`, followed by NaN (GR rows of a 2-D input, G1 elements of a 1-D
    one): a read past the end reaches the kernel's sums.  Kept alive until the test ends."""
    if t is None:
        return None
    g = GR if t.dim() == 2 else G1
    buf = torch.full((t.shape[0] + g,) + tuple(t.shape[1:]), NAN, dtype=dtype, device=DEV)
    buf[:t.shape[0]] = t.to(dtype).to(DEV)
    KEEP.append(buf)
    return buf[:t.shape[0]]


def P(t):
    return None if t is None else (t.ptr() if isinstance(t, Guarded) else t.data_ptr())


def same(got, ref64, what):
    """got (a Guarded output) is bit-equal to the float64 reference cast to its type."""
    got.check(what)
    g = got.cpu()
    r = ref64.to(g.dtype)
    bad = (g.double() != r.double()).nonzero()
    assert torch.equal(g, r), f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: " \
                              f"{g[tuple(bad[0])].item()} != {r[tuple(bad[0])].item()}"


SEEDS = {}


def seed_tensor(seed):
    if seed not in SEEDS:
        SEEDS[seed] = torch.tensor([seed], dtype=torch.int32, device=DEV)
    return SEEDS[seed]


def set_drop(a, seed, site, p):
    ops._drop_into(a, ops.Drop(seed_tensor(seed), site, p) if p > 0 else ops.NO_DROP)


def stream():
    return _lib.stream_ptr()


def wsbuf(nbytes):
    KEEP.append(torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=DEV))
    return KEEP[-1]


# ================================================================ LayerNorm
def ln_args(dtype, m, c=LC, **f):
    a = _lib.LnArgs()
    a.m, a.c, a.dtype = m, c, {F32: _lib.DT_F32, BF16: _lib.DT_BF16}[dtype]
    for k, v in f.items():
        setattr(a, k, P(v) if k in ("x", "branch", "dy", "y", "dx", "dbranch", "gamma", "beta", "mean", "rstd",
                                    "dgamma", "dbeta", "dbias") else v)
    return a


def ln_ws(a, nbytes=None):
    need = _lib.lib().tt2_layernorm_bwd_workspace_size(C.byref(a))
    buf = wsbuf(need if nbytes is None else nbytes)
    a.workspace, a.ws_bytes = buf.data_ptr(), (need if nbytes is None else nbytes)
    return buf


class LnBwdRun:
    """One tt2_layernorm_bwd call on an _norm_refs problem: device inputs, poisoned outputs whose
    parameter gradients start as the problem's integer priors, and the args."""

    def __init__(self, pr, dtype, want_dbranch=True, want_dbias=True, defer=False):
        self.pr, m = pr, pr.m
        has_br = pr.branch is not None
        if getattr(pr, "_dev", None) is None:   # the inputs go up once per problem
            pr._dev = [inp(t, dtype) for t in (pr.dy, pr.x, pr.branch)] + [inp(t) for t in (pr.gamma, pr.mean, pr.rstd)]
        dy, x, br, gamma, mean, rstd = pr._dev
        self.dx = Guarded((m, LC), dtype)
        self.dbr = Guarded((m, LC), dtype) if has_br and want_dbranch else None
        self.vec = [Guarded((LC,)) for _ in range(3)]
        if not (has_br and want_dbias):
            self.vec[2] = None
        for v, p0 in zip(self.vec, pr.prior):
            if v is not None and pr.grad_beta != 0:
                v.v.copy_(p0.float())
        self.a = ln_args(dtype, m, dy=dy, x=x, branch=br, gamma=gamma, mean=mean, rstd=rstd, dx=self.dx,
                         dbranch=self.dbr, dgamma=self.vec[0], dbeta=self.vec[1], dbias=self.vec[2],
                         grad_beta=pr.grad_beta, defer_finalize=int(defer))
        if has_br:
            set_drop(self.a, pr.SEED, pr.SITE, pr.p)
        self.ws = ln_ws(self.a)

    def launch(self, prev=None):
        self.a.finalize_prev = C.addressof(prev.a) if prev is not None else None
        _lib.check(_lib.lib().tt2_layernorm_bwd(C.byref(self.a), stream()), "tt2_layernorm_bwd")

    def check_exact(self, what):
        dx, dbr, dg, db, dd = self.pr.ref()
        if self.pr.m:
            same(self.dx, dx, what + " dx")
            if self.dbr is not None:
                same(self.dbr, dbr, what + " dbranch")
        for v, r, n in zip(self.vec, (dg, db, dd), ("dgamma", "dbeta", "dbias")):
            if v is not None:
                same(v, r, f"{what} {n}")


LN_BWD_CFG = [  # p, branch, dbranch, dbias
    (0.5, True, True, True), (0.0, True, False, True), (0.5, True, True, False), (0.0, False, False, False)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("m", [1, 5, 37, 272, 785, 3100, 4100])
def test_ln_bwd_exact(m, dtype):
    """1, 1, 3, 17, 50, 194 and 256 work-groups: the unrolled loops and tails of ln_bwd_finalize
    (r + 48 < nb) and ln_fin_col (r + 192 < nb), and from 3100 rows a second row per wave.  dx,
    dbranch, dgamma, dbeta and dbias are bit-equal to float64 through the immediate finalize,
    tt2_layernorm_bwd_finalize, a chained finalize_prev inside another call's launch and a chained
    call with m = 0; grad_beta 0 / 1 / 0.5 on integer priors; with and without branch, dbranch,
    dbias and dropout."""
    assert R.ln_bwd_blocks(m) == {1: 1, 5: 1, 37: 3, 272: 17, 785: 50, 3100: 194, 4100: 256}[m]
    nxt = R.ln_bwd_exact(37, dtype, 0.5, True, 0.0, seed=9)
    for p, has_br, want_dbr, want_db in LN_BWD_CFG:
        pr = R.ln_bwd_exact(m, dtype, p, has_br)
        for gb in (0.0, 1.0, 0.5):
            pr.with_grad_beta(gb)
            what = f"ln_bwd m={m} p={p} branch={has_br} grad_beta={gb} mixed_rstd={bool((pr.rstd != 1).any())}"
            r = LnBwdRun(pr, dtype, want_dbr, want_db)
            r.launch()
            r.check_exact(what + " immediate")
            r = LnBwdRun(pr, dtype, want_dbr, want_db, defer=True)
            r.launch()
            _lib.check(_lib.lib().tt2_layernorm_bwd_finalize(C.byref(r.a), stream()), "finalize")
            r.check_exact(what + " standalone")
            r = LnBwdRun(pr, dtype, want_dbr, want_db, defer=True)
            r.launch()
            n = LnBwdRun(nxt, dtype)
            n.launch(prev=r)
            r.check_exact(what + " chained")
            n.check_exact(what + " the chaining call")
            r = LnBwdRun(pr, dtype, want_dbr, want_db, defer=True)
            r.launch()
            z = ln_args(dtype, 0, finalize_prev=C.addressof(r.a))
            zws = ln_ws(z)   # noqa: F841  (held until the launch is checked)
            _lib.check(_lib.lib().tt2_layernorm_bwd(C.byref(z), stream()), "tt2_layernorm_bwd m=0")
            r.check_exact(what + " chained from m = 0")


def hold_rsqrt(got, expect64, what):
    """rsqrtf of a power of four: asserted exact (see test_ln_fwd_exact's docstring)."""
    g = got.cpu().double()
    assert torch.equal(g, expect64), \
        f"{what}: rsqrtf(4^k) is not exactly 2^-k on this device (worst {((g - expect64).abs() / expect64).max():.3e} " \
        f"relative): hold rstd to 2 ulp and the outputs by the float64 bar with the device's rstd instead"


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("m", [1, 5, 37, 272])
def test_ln_fwd_exact(m, dtype):
    """Rows half K + 1 and half K - 1, eps = 3: mean = K bit for bit, variance + eps = 4.
    rsqrtf(4.0f) == 0.5 exactly on gfx950 (MI355X, measured by this test: rstd is asserted equal,
    as are tt2_ln_combine's outputs and eval-mode BatchNorm's rstd at 4, 16 and 64), so y is
    bit-exact too.  With branch and dropout 0.5, branch without dropout, and branch = None with
    mean = rstd = None (y alone is written)."""
    for p, has_br, want_stats in ((0.5, True, True), (0.0, True, True), (0.0, False, False), (0.0, False, True)):
        pr = R.LnFwdExact(m, p, has_br)
        assert pr.exact()[0]
        what = f"ln_fwd m={m} p={p} branch={has_br} stats={want_stats}"
        y = Guarded((m, LC), dtype)
        mean, rstd = (Guarded((m,)), Guarded((m,))) if want_stats else (None, None)
        a = ln_args(dtype, m, x=inp(pr.x, dtype), branch=inp(pr.branch, dtype), gamma=inp(pr.gamma), beta=inp(pr.beta),
                    y=y, mean=mean, rstd=rstd, eps=pr.EPS)
        if has_br:
            set_drop(a, pr.SEED, pr.SITE, p)
        _lib.check(_lib.lib().tt2_layernorm_fwd(C.byref(a), stream()), what)
        ry, rmean, rrstd = R.ref_ln_fwd(pr.x, pr.branch, pr.keep, pr.gamma, pr.beta, pr.EPS, scale=pr.scale)
        assert torch.equal(rmean, pr.K) and torch.equal(rrstd, torch.full((m,), 0.5, dtype=F64))
        if want_stats:
            same(mean, rmean, what + " mean")
            rstd.check(what + " rstd")
            hold_rsqrt(rstd, rrstd, what + " rstd")
        same(y, ry, what + " y")


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("splits", [1, 2, 4, 8, 16])
def test_ln_combine_exact(splits, dtype):
    """y = LN(x + bias + sum of the S slabs) with integer slabs, bias and x making each row K +- 1
    (eps = 3): bit-equal to float64 for M = 1, 3, 64 (rsqrtf(4) exact: see test_ln_fwd_exact)."""
    for m in (1, 3, 64):
        pr = R.LnFwdExact(m, splits=splits)
        assert pr.exact()[0]
        y = Guarded((m, LC), dtype)
        x, parts = inp(pr.x, dtype), inp(pr.parts.reshape(splits * m, LC))
        bias, gamma, beta = inp(pr.bias), inp(pr.gamma), inp(pr.beta)
        rc = _lib.lib().tt2_ln_combine(x.data_ptr(), parts.data_ptr(), splits, bias.data_ptr(), gamma.data_ptr(),
                                       beta.data_ptr(), y.ptr(), m, LC, pr.EPS, _lib.dt(x), stream())
        _lib.check(rc, "tt2_ln_combine")
        ref = R.ref_ln_combine(x.cpu(), pr.parts, pr.bias, pr.gamma, pr.beta, pr.EPS)
        same(y, ref, f"ln_combine S={splits} m={m}")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("m,p", [(37, 0.0), (600, 0.1)])
def test_ln_random_per_row(m, p, dtype):
    """Forward and backward on ill-conditioned rows, each row held on its own (y, dx, dbranch:
    worst_ratio_by rows; mean and rstd: worst_ratio over the rows of one kind; dgamma, dbeta,
    dbias: worst_ratio).  The backward is given the device's own mean and rstd, as is its
    reference.  Worst ratios on the MI355X: y 0.78, mean 0.45, rstd 0.28, dx 0.50, dbranch 0.62,
    dgamma 0.25, dbeta 0.34, dbias 0.30."""
    SEED, SITE = 5, 17
    x, br, gamma, beta, dy, kind = R.ln_random(m, dtype, m)
    keep, scale = R.keep_mask(SEED, SITE, m, LC, p), R.drop_scale(p)
    y, mean, rstd = Guarded((m, LC), dtype), Guarded((m,)), Guarded((m,))
    xd, brd, dyd, gd, bd = inp(x, dtype), inp(br, dtype), inp(dy, dtype), inp(gamma), inp(beta)
    a = ln_args(dtype, m, x=xd, branch=brd, gamma=gd, beta=bd, y=y, mean=mean, rstd=rstd, eps=1e-5)
    set_drop(a, SEED, SITE, p)
    _lib.check(_lib.lib().tt2_layernorm_fwd(C.byref(a), stream()), "tt2_layernorm_fwd")
    r64 = R.ref_ln_fwd(x, br, keep, gamma, beta, 1e-5, scale=scale)
    r32 = R.ref_ln_fwd(x, br, keep, gamma, beta, 1e-5, scale=scale, dtype=F32)
    for o in (y, mean, rstd):
        o.check("ln_fwd")
    worst = {"y": R.worst_ratio_by(y.cpu(), r64[0], r32[0], dtype)}
    for k in kind.unique().tolist():
        sel = kind == k
        worst[f"mean kind {k}"] = (MR.worst_ratio(mean.cpu()[sel], r64[1][sel], r32[1][sel]), k)
        worst[f"rstd kind {k}"] = (MR.worst_ratio(rstd.cpu()[sel], r64[2][sel], r32[2][sel]), k)
    # backward, with the device's statistics
    mean_d, rstd_d = mean.cpu(), rstd.cpu()
    dx, dbr = Guarded((m, LC), dtype), Guarded((m, LC), dtype)
    vec = [Guarded((LC,)) for _ in range(3)]
    prior = [torch.randn(LC, generator=torch.Generator().manual_seed(i)) for i in range(3)]
    for v, p0 in zip(vec, prior):
        v.v.copy_(p0)
    b = ln_args(dtype, m, dy=dyd, x=xd, branch=brd, gamma=gd, mean=inp(mean_d), rstd=inp(rstd_d), dx=dx, dbranch=dbr,
                dgamma=vec[0], dbeta=vec[1], dbias=vec[2], grad_beta=0.5)
    set_drop(b, SEED, SITE, p)
    ws = ln_ws(b)   # noqa: F841
    _lib.check(_lib.lib().tt2_layernorm_bwd(C.byref(b), stream()), "tt2_layernorm_bwd")
    b64 = R.ref_ln_bwd(dy, x, br, keep, gamma, mean_d, rstd_d, 0.5, *prior, scale=scale)
    b32 = R.ref_ln_bwd(dy, x, br, keep, gamma, mean_d, rstd_d, 0.5, *prior, scale=scale, dtype=F32)
    for o in [dx, dbr] + vec:
        o.check("ln_bwd")
    worst["dx"] = R.worst_ratio_by(dx.cpu(), b64[0], b32[0], dtype)
    worst["dbranch"] = R.worst_ratio_by(dbr.cpu(), b64[1], b32[1], dtype)
    for i, n in enumerate(("dgamma", "dbeta", "dbias")):
        worst[n] = (MR.worst_ratio(vec[i].cpu(), b64[2 + i], b32[2 + i]), -1)
    print(f"\nln random m={m} p={p} {dtype}: " + ", ".join(f"{k} {v[0]:.3f}@{v[1]}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v[0] <= 1, f"{k}: ratio {v[0]:.3f} at row / kind {v[1]}"


# ================================================================ BatchNorm
BN_PTRS = ("y", "dout", "res", "out", "dy", "gamma", "beta", "mean", "rstd", "run_mean", "run_var", "dgamma", "dbeta")
DT = {F32: _lib.DT_F32, BF16: _lib.DT_BF16}


def bn_args(dtype, m, c, **f):
    a = _lib.BnArgs()
    a.m, a.c, a.dtype = m, c, DT[dtype]
    a.eps, a.momentum, a.training = 1e-5, 0.1, 1
    for k, v in f.items():
        setattr(a, k, P(v) if k in BN_PTRS else v)
    return a


def bn_ws(a, chunks=None):
    """A workspace of the size the library asks for; chunks: the chunk count it must imply."""
    need = _lib.lib().tt2_batchnorm_workspace_size(C.byref(a))
    if chunks is not None:
        assert need == chunks * 2 * a.c * 4, f"{need} bytes: not {chunks} chunks of m = {a.m}"
    buf = wsbuf(need)
    a.workspace, a.ws_bytes = buf.data_ptr(), need
    return buf


def bn_fwd(a, what="tt2_batchnorm_fwd"):
    _lib.check(_lib.lib().tt2_batchnorm_fwd(C.byref(a), stream()), what)


def bn_bwd(a, what="tt2_batchnorm_bwd"):
    _lib.check(_lib.lib().tt2_batchnorm_bwd(C.byref(a), stream()), what)


BN_FWD_SHAPES = [(8, 8, 8), (64, 80, 8), (136, 512, 8), (2048, 2048, 8), (2056, 520, 8), (4096, 80, 16),
                 (16384, 8, 64)]


@pytest.mark.parametrize("design", [1, 2])
@pytest.mark.parametrize("m,c,rows_per", BN_FWD_SHAPES)
def test_bn_train_fwd_exact(m, c, rows_per, design):
    """Integer y of four K + 1 and four K - 1 per 8 rows, eps = 3: chunk moments exact in f32, the
    combine exact in double, variance + eps = 4 (design 1) -- mean, rstd and both running
    statistics bit-equal to the float64 reference with the float32 momentum widened; design 1
    also `out` (power-of-two gamma, integer beta, none / relu, dropout 0.5 / off, an integer f32
    and bf16 residual with res_ld = C + 8), in all four dtype x out_dtype pairs.  Design 2 (chunk
    means K +- 2) carries the variance through the combine; its `out` is held by
    test_bn_random.  The chunk count asserts the rows_per route (8 / 16 / 64)."""
    for dtype, out_dtype, res_dtype, p, act in ((F32, F32, F32, 0.5, ACT_RELU), (BF16, BF16, BF16, 0.0, ACT_NONE),
                                                (F32, BF16, BF16, 0.5, ACT_NONE), (BF16, F32, F32, 0.0, ACT_RELU),
                                                (BF16, BF16, None, 0.5, ACT_RELU)):
        pr = R.BnFwdExact(m, c, design, p, res_dtype is not None, c + 8)
        assert pr.rows_per == rows_per and pr.exact()[0]
        what = f"bn_fwd {m}x{c} design {design} {dtype}->{out_dtype} res {res_dtype} p={p} act={act}"
        out, mean, rstd = Guarded((m, c), out_dtype), Guarded((c,)), Guarded((c,))
        rm, rv = Guarded((c,)), Guarded((c,))
        rm.v.copy_(pr.rm0.float())
        rv.v.copy_(pr.rv0.float())
        a = bn_args(dtype, m, c, y=inp(pr.y, dtype), gamma=inp(pr.gamma), beta=inp(pr.beta), mean=mean, rstd=rstd,
                    run_mean=rm, run_var=rv, out=out, out_dtype=DT[out_dtype], act=act, eps=pr.EPS, momentum=pr.MOM,
                    res=inp(pr.res, res_dtype) if res_dtype else None, res_dtype=DT[res_dtype] if res_dtype else 0,
                    res_ld=pr.res_ld)
        set_drop(a, pr.SEED, pr.SITE, p)
        ws = bn_ws(a, m // rows_per)   # noqa: F841
        bn_fwd(a, what)
        ro, rmean, rrstd, rrm, rrv = pr.ref(act)
        same(mean, rmean, what + " mean")
        same(rstd, rrstd, what + " rstd")
        same(rm, rrm, what + " run_mean")
        same(rv, rrv, what + " run_var")
        if design == 1:
            assert torch.equal(rrstd, torch.full((c,), 0.5, dtype=F64))
            same(out, ro, what + " out")
        else:
            out.check(what + " out")


@pytest.mark.parametrize("c", [8, 80, 520, 2048])
@pytest.mark.parametrize("m", [8, 64, 1024, 4096])
def test_bn_bwd_exact(m, c):
    """Given integer mean and rstd in {0.5, 1}; dout in {-1, 0, 1}; none and relu with
    pre-activations exactly 0 and moved across 0 by beta; 1 / M exact: dgamma, dbeta and dy
    bit-equal, for all four <y, dout> type pairs, in training and in eval (training = 0: the
    unfused bn_bwd_finalize_kernel / bn_bwd_apply_kernel route), with dropout 0.5 and off."""
    probs = {}
    for (dtype, dd), p, act in (((F32, F32), 0.5, ACT_RELU), ((BF16, BF16), 0.0, ACT_RELU), ((F32, BF16), 0.5, ACT_NONE),
                                ((BF16, F32), 0.5, ACT_RELU)):
        if p not in probs:
            probs[p] = R.BnBwdExact(m, c, p)
            assert probs[p].exact()[0]
        pr = probs[p]
        ins = dict(y=inp(pr.y, dtype), dout=inp(pr.dout, dd), gamma=inp(pr.gamma), beta=inp(pr.beta),
                   mean=inp(pr.mean), rstd=inp(pr.rstd))
        for training in (1, 0):
            what = f"bn_bwd {m}x{c} y {dtype} dout {dd} p={p} act={act} training={training}"
            dy, dg, db = Guarded((m, c), dtype), Guarded((c,)), Guarded((c,))
            a = bn_args(dtype, m, c, dy=dy, dgamma=dg, dbeta=db, dout_dtype=DT[dd], act=act, training=training, **ins)
            set_drop(a, pr.SEED, pr.SITE, p)
            ws = bn_ws(a, (m + R.bn_rows_per(m) - 1) // R.bn_rows_per(m))   # noqa: F841
            bn_bwd(a, what)
            rdy, rdg, rdb = pr.ref(act, training)
            same(dg, rdg, what + " dgamma")
            same(db, rdb, what + " dbeta")
            same(dy, rdy, what + " dy")


@pytest.mark.parametrize("dtype,out_dtype", [(F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)])
@pytest.mark.parametrize("m,c", [(1, 8), (37, 80), (300, 520), (64, 2048)])
def test_bn_eval_fwd_exact(m, c, dtype, out_dtype):
    """training = 0 (bn_finalize_kernel's eval branch, bn_apply_kernel): integer running mean,
    run_var + eps in {4, 16, 64}: mean and rstd (rsqrtf of a power of four: exact on the MI355X,
    see test_ln_fwd_exact) and `out` bit-equal; the running statistics are not written."""
    g = torch.Generator().manual_seed(m + c)
    rm = torch.randint(-4, 5, (c,), generator=g).double()
    rv = torch.tensor([1.0, 13.0, 61.0], dtype=F64)[torch.randint(0, 3, (c,), generator=g)]
    y = rm[None] + 8 * torch.randint(-4, 5, (m, c), generator=g).double()
    gamma = torch.tensor([1.0, -2.0, 4.0], dtype=F64)[torch.randint(0, 3, (c,), generator=g)]
    beta = torch.randint(-3, 4, (c,), generator=g).double()
    res = torch.randint(-4, 5, (m, c + 8), generator=g).double()
    keep, scale = R.keep_mask(11, 12, m, c, 0.5), R.drop_scale(0.5)
    for act, with_res in ((ACT_RELU, True), (ACT_NONE, False)):
        what = f"bn eval fwd {m}x{c} {dtype}->{out_dtype} act={act}"
        out, mean, rstd = Guarded((m, c), out_dtype), Guarded((c,)), Guarded((c,))
        rmd, rvd = Guarded((c,)), Guarded((c,))
        rmd.v.copy_(rm.float())
        rvd.v.copy_(rv.float())
        a = bn_args(dtype, m, c, y=inp(y, dtype), gamma=inp(gamma), beta=inp(beta), mean=mean, rstd=rstd, run_mean=rmd,
                    run_var=rvd, out=out, out_dtype=DT[out_dtype], act=act, eps=3.0, training=0,
                    res=inp(res, BF16) if with_res else None, res_dtype=DT[BF16], res_ld=c + 8)
        set_drop(a, 11, 12, 0.5)
        bn_fwd(a, what)   # no workspace: eval needs none
        ro, rmean, rrstd, _, _ = R.ref_bn_fwd(y, gamma, beta, keep, res if with_res else None, act, 3.0, 0.1, rm, rv,
                                              False, scale=scale)
        assert R.is_f32(ro)
        same(mean, rmean, what + " mean")
        rstd.check(what + " rstd")
        hold_rsqrt(rstd, rrstd, what + " rstd")
        same(out, ro, what + " out")
        same(rmd, rm, what + " run_mean")
        same(rvd, rv, what + " run_var")


BN_RANDOM = ([(m, 8 if m % 2 else 80, act) for m, act in ((1, ACT_RELU), (7, ACT_TANH), (9, ACT_NONE), (2051, ACT_TANH),
                                                            (4100, ACT_RELU), (16389, ACT_TANH), (16389, ACT_RELU))]
             + [(333, 8, ACT_TANH), (333, 80, ACT_NONE), (333, 520, ACT_TANH), (333, 2048, ACT_RELU),
                (4100, 80, ACT_TANH), (16389, 80, ACT_NONE)])


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("m,c,act", BN_RANDOM)
def test_bn_random(m, c, act, dtype):
    """Training forward and backward, dropout 0.2 and a bf16 residual (res_ld = C + 16), M not a
    multiple of the chunk (rows_per 8 / 16 / 64 and their short last chunks), M = 1 (variance 0,
    running variance from the biased one: the reference, not torch, defines it), every column held
    on its own: out and dy by worst_ratio_by columns, mean / rstd / running statistics
    by worst_ratio over the columns of one kind (ill-conditioned, constant, ordinary), dgamma /
    dbeta by worst_ratio.  The backward and its reference are given the device's own mean and rstd.

    act = tanh: fast_tanh's absolute error is added to the bar as TANH_ABS * scale (forward) and
    propagated to first order (backward, tanh_bwd_extra).  Measured on the MI355X: fast_tanh alone
    (f32, ordinary columns, no residual, device statistics) errs by at most 2.48 x 2^-24 over this
    test's tanh shapes (the float32 reference by 2.01); allowed 4 x that rounded up to a power of
    two = 16 x 2^-24 (_norm_refs.TANH_ABS).  Over the whole `out` of these cases, with the bf16
    residual and the columns at mean 1e3 x std, the worst |out - ref64| / scale is 421 x 2^-24
    (`tanh abs`, pytest -s) where the float32 reference itself errs by 710 x 2^-24: that is the
    rounding of a mean near 1e3, not tanh.
    Worst ratios on the MI355X: out 0.61, mean 0.50, rstd 0.53, running mean / variance 0.25 /
    0.57, dy 0.49, dgamma 0.40, dbeta 0.39."""
    SEED, SITE, p = 7, 33, 0.2
    y, gamma, beta, dout, res, rm0, rv0, kind = R.bn_random(m, c, dtype, m + c + act)
    keep, scale = R.keep_mask(SEED, SITE, m, c, p), R.drop_scale(p)
    out, mean, rstd, rm, rv = Guarded((m, c), dtype), Guarded((c,)), Guarded((c,)), Guarded((c,)), Guarded((c,))
    rm.v.copy_(rm0)
    rv.v.copy_(rv0)
    yd, gd, bd = inp(y, dtype), inp(gamma), inp(beta)
    a = bn_args(dtype, m, c, y=yd, gamma=gd, beta=bd, mean=mean, rstd=rstd, run_mean=rm, run_var=rv, out=out,
                out_dtype=DT[dtype], act=act, res=inp(res, BF16), res_dtype=DT[BF16], res_ld=c + 16)
    set_drop(a, SEED, SITE, p)
    rp = R.bn_rows_per(m)
    ws = bn_ws(a, (m + rp - 1) // rp)   # noqa: F841
    bn_fwd(a)
    args = (y, gamma, beta, keep, res, act, 1e-5, 0.1, rm0, rv0, True)
    r64, r32 = R.ref_bn_fwd(*args, scale=scale), R.ref_bn_fwd(*args, scale=scale, dtype=F32)
    for o in (out, mean, rstd, rm, rv):
        o.check("bn_fwd")
    worst = {"out": R.worst_ratio_by(out.cpu(), r64[0], r32[0], dtype, dim=0, kind=kind, pool=R.bn_pool(m),
                                     extra_abs=R.TANH_ABS * scale if act == ACT_TANH else 0.0)}
    for i, (n, t) in enumerate((("mean", mean), ("rstd", rstd), ("run_mean", rm), ("run_var", rv))):
        R.by_kind(worst, n, t.cpu(), r64[1 + i], r32[1 + i], kind)
    if act == ACT_TANH and dtype == F32:
        print(f"\ntanh abs {m}x{c}: {((out.cpu().double() - r64[0]).abs().max() / scale / 2.0 ** -24).item():.2f} x 2^-24 "
              f"(f32 reference {((r32[0].double() - r64[0]).abs().max() / scale / 2.0 ** -24).item():.2f})")
    # backward with the device's statistics
    mean_d, rstd_d = mean.cpu(), rstd.cpu()
    dy, dg, db = Guarded((m, c), dtype), Guarded((c,)), Guarded((c,))
    b = bn_args(dtype, m, c, y=yd, dout=inp(dout, dtype), gamma=gd, beta=bd, mean=inp(mean_d), rstd=inp(rstd_d), dy=dy,
                dgamma=dg, dbeta=db, dout_dtype=DT[dtype], act=act)
    set_drop(b, SEED, SITE, p)
    ws2 = bn_ws(b, (m + rp - 1) // rp)   # noqa: F841
    bn_bwd(b)
    bargs = (y, dout, gamma, beta, mean_d, rstd_d, keep, act, True, m)
    b64, b32 = R.ref_bn_bwd(*bargs, scale=scale), R.ref_bn_bwd(*bargs, scale=scale, dtype=F32)
    for o in (dy, dg, db):
        o.check("bn_bwd")
    ex = R.tanh_bwd_extra(y, dout, gamma, beta, mean_d, rstd_d, keep, scale, m) if act == ACT_TANH else (0.0, None, None)
    worst["dy"] = R.worst_ratio_by(dy.cpu(), b64[0], b32[0], dtype, dim=0, extra_abs=ex[0], kind=kind, pool=R.bn_pool(m))
    R.by_kind(worst, "dgamma", dg.cpu(), b64[1], b32[1], None, ex[1])
    R.by_kind(worst, "dbeta", db.cpu(), b64[2], b32[2], None, ex[2])
    print(f"\nbn random {m}x{c} act={act} {dtype}: " + ", ".join(f"{k} {v[0]:.3f}@{v[1]}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v[0] <= 1, f"{k}: ratio {v[0]:.3f} at column / kind {v[1]}"


@pytest.mark.parametrize("dtype,m,c", [(F32, 333, 80), (BF16, 2051, 520)])
def test_bn_fwd_in_place(dtype, m, c):
    """out == y (the header allows it; the chunk means are then kept as absolute f32 values, since
    the apply overwrites the rows they would be relative to): on ordinary columns every output is
    bit-equal to the out-of-place call's, and the guard rows around the shared buffer stay NaN."""
    g = torch.Generator().manual_seed(m + c)
    y = (torch.randn(m, c, generator=g) * 3 + 1.5).to(dtype)
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    gd, bd = inp(gamma), inp(beta)
    got = {}
    for in_place in (False, True):
        outs = [Guarded((m, c), dtype)] + [Guarded((c,)) for _ in range(4)]
        out, mean, rstd, rm, rv = outs
        rm.v.zero_()
        rv.v.fill_(1.0)
        if in_place:
            out.v.copy_(y.to(DEV))
        a = bn_args(dtype, m, c, y=out if in_place else inp(y, dtype), gamma=gd, beta=bd, mean=mean, rstd=rstd,
                    run_mean=rm, run_var=rv, out=out, out_dtype=DT[dtype], act=ACT_RELU)
        assert (a.y == a.out) == in_place
        set_drop(a, 7, 33, 0.2)
        ws = bn_ws(a)   # noqa: F841
        bn_fwd(a)
        for o in outs:
            o.check(f"bn_fwd in_place={in_place}")
        got[in_place] = [o.cpu() for o in outs]
    for name, a_, b_ in zip(("out", "mean", "rstd", "run_mean", "run_var"), got[False], got[True]):
        assert torch.equal(a_, b_), f"{name}: the in-place forward differs from the out-of-place one"
    assert got[True][0].float().abs().sum() > 0


ILL_STATS = ("rstd kind 0", "run_var kind 0")


@pytest.mark.parametrize("m,c", [(9, 8), (333, 80), (2051, 8), (16389, 80)])
def test_bn_stats_of_ill_conditioned_columns(m, c):
    """rstd and the running variance of the two f32 columns at mean +-1e3 x std (bn_random), at
    the bar of every other statistic: max(4 x the float32-CPU error over the two columns, 2 ulp),
    from two chunks up to 257.

    These tests found the one defect of this file's kernels: bn_stats_kernel stored each chunk's
    mean as one absolute f32, rounded by up to ulp(1e3) / 2 = 3e-5, and the combine's
    between-chunk term n_c (mean_c - mean)^2 carried that rounding to first order (a two-pass
    float32 evaluation has no such term).  rstd / run_var missed this bar by 62.56 / 2.43 at
    9 x 8, 15.39 / 1.32 at 333 x 80 and 3.63 / 1.00 at 2051 x 8 on the MI355X; the numpy model of
    tests/test_norm_refs.py with abs_mean_f32 misses it by 62.56, 15.39 and 4.92 (its sums run in
    another order).  The chunk mean is now stored
    relative to the chunk's first row, which bn_fin64 re-reads; for a column with |mean| > 8 sigma
    it adds the two in double (other columns round the sum to f32 as before, bit for bit).
    Ratios on the MI355X now: 0.14 to 0.25."""
    y, gamma, beta, _, _, rm0, rv0, kind = R.bn_random(m, c, F32, m + c)
    out, mean, rstd, rm, rv = Guarded((m, c)), Guarded((c,)), Guarded((c,)), Guarded((c,)), Guarded((c,))
    rm.v.copy_(rm0)
    rv.v.copy_(rv0)
    a = bn_args(F32, m, c, y=inp(y), gamma=inp(gamma), beta=inp(beta), mean=mean, rstd=rstd, run_mean=rm, run_var=rv,
                out=out, act=ACT_NONE)
    ws = bn_ws(a)   # noqa: F841
    bn_fwd(a)
    args = (y, gamma, beta, None, None, ACT_NONE, 1e-5, 0.1, rm0, rv0, True)
    r64, r32 = R.ref_bn_fwd(*args), R.ref_bn_fwd(*args, dtype=F32)
    worst = {}
    R.by_kind(worst, "rstd", rstd.cpu(), r64[2], r32[2], kind)
    R.by_kind(worst, "run_var", rv.cpu(), r64[4], r32[4], kind)
    print(f"\nbn ill-conditioned stats {m}x{c}: " + ", ".join(f"{k} {worst[k][0]:.2f}" for k in ILL_STATS))
    for k in ILL_STATS:
        assert worst[k][0] <= 1, f"{k}: ratio {worst[k][0]:.2f}"


@pytest.mark.parametrize("R_", [1, 3, 5, 13, 17])
def test_bn_given_chunk_stats(R_):
    """stats = (buf, rows = 128) fed with the float64 reference's chunk moments (forward) and chunk
    sums (backward) rounded to f32, an uneven last chunk: bn_fin64 / bn_bsum64 alone (unrolled
    r + 12 < R loop and tail), against the float64 combine of the same f32 partials.  Worst ratio
    on the MI355X: 0.74 (out), 0.34 on the sums."""
    rows, c, act = 128, 80, ACT_RELU
    m = rows * (R_ - 1) + 77
    y, gamma, beta, dout, _, rm0, rv0, kind = R.bn_random(m, c, F32, R_)
    mom = R.ref_bn_chunk_moments(y, rows).float()
    assert mom.shape == (R_, 2, c)
    out, mean, rstd, rm, rv = Guarded((m, c)), Guarded((c,)), Guarded((c,)), Guarded((c,)), Guarded((c,))
    rm.v.copy_(rm0)
    rv.v.copy_(rv0)
    yd, gd, bd = inp(y), inp(gamma), inp(beta)
    sbuf = inp(mom.reshape(R_ * 2, c))
    a = bn_args(F32, m, c, y=yd, gamma=gd, beta=bd, mean=mean, rstd=rstd, run_mean=rm, run_var=rv, out=out, act=act,
                stats_rows=rows)
    assert _lib.lib().tt2_batchnorm_workspace_size(C.byref(a)) == R_ * 2 * c * 4
    a.workspace, a.ws_bytes = sbuf.data_ptr(), R_ * 2 * c * 4
    bn_fwd(a)
    worst = {}
    for dt_, store in ((F64, "64"), (F32, "32")):
        mu, m2, rs = R.ref_bn_combine(mom, rows, m, 1e-5, dtype=dt_)
        mo = torch.tensor(R.f32w(0.1), dtype=dt_)
        worst[store] = (mu, rs, (1 - mo) * rm0.to(dt_) + mo * mu, (1 - mo) * rv0.to(dt_) + mo * m2 / (m - 1))
    r64, r32 = worst.pop("64"), worst.pop("32")
    for i, (n, t) in enumerate((("mean", mean), ("rstd", rstd), ("run_mean", rm), ("run_var", rv))):
        t.check(n)
        R.by_kind(worst, n, t.cpu(), r64[i], r32[i], kind)
    mean_d, rstd_d = mean.cpu(), rstd.cpu()
    out.check("out")
    worst["out"] = R.worst_ratio_by(out.cpu(), R.ref_bn_apply(y, mean_d, rstd_d, gamma, beta, None, None, act),
                                    R.ref_bn_apply(y, mean_d, rstd_d, gamma, beta, None, None, act, dtype=F32), dim=0,
                                    kind=kind, pool=R.bn_pool(m))
    # backward: reference chunk sums in
    sums = R.ref_bn_bwd_chunk_sums(y, dout, gamma, beta, mean_d, rstd_d, None, act, rows).float()
    dy, dg, db = Guarded((m, c)), Guarded((c,)), Guarded((c,))
    b = bn_args(F32, m, c, y=yd, dout=inp(dout), gamma=gd, beta=bd, mean=inp(mean_d), rstd=inp(rstd_d), dy=dy, dgamma=dg,
                dbeta=db, act=act, stats_rows=rows)
    s2 = inp(sums.reshape(R_ * 2, c))
    b.workspace, b.ws_bytes = s2.data_ptr(), R_ * 2 * c * 4
    bn_bwd(b)
    for o in (dy, dg, db):
        o.check("bn_bwd")
    sb64, sg64 = sums[:, 0].double().sum(0), sums[:, 1].double().sum(0)
    sb32, sg32 = sums[:, 0].sum(0), sums[:, 1].sum(0)
    R.by_kind(worst, "dbeta", db.cpu(), sb64, sb32, None)
    R.by_kind(worst, "dgamma", dg.cpu(), sg64, sg32, None)
    bargs = (y, dout, gamma, beta, mean_d, rstd_d, None, act, True, m)
    worst["dy"] = R.worst_ratio_by(dy.cpu(), R.ref_bn_bwd(*bargs, sums=(sb64, sg64))[0],
                                   R.ref_bn_bwd(*bargs, sums=(sb32, sg32), dtype=F32)[0], dim=0, kind=kind, pool=R.bn_pool(m))
    print(f"\nbn given stats R={R_}: " + ", ".join(f"{k} {v[0]:.3f}@{v[1]}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v[0] <= 1, f"{k}: ratio {v[0]:.3f} at column / kind {v[1]}"


class SimSync:
    """One simulated rank (the style of test_gpu_syncbn.py): exchange() records this rank's slots
    and adds the other ranks' recorded ones, which is what the SUM all-reduce does."""

    def __init__(self, world, rank, others=()):
        self.world, self.rank, self.others = world, rank, list(others)
        self.buf = torch.zeros((4 * world + 2) * 2048 + 4, device=DEV)
        self.sent = None

    def buffer(self, nbytes):
        return self.buf[:(nbytes + 3) // 4]

    def exchange(self, slots):
        self.sent = slots.clone()
        for o in self.others:
            slots += o


@pytest.mark.parametrize("c,act,Ms", [(80, ACT_RELU, (96, 1201, 7)), (520, ACT_TANH, (213, 64, 300))])
def test_syncbn_three_ranks(c, act, Ms):
    """Three simulated ranks with unequal rows: every rank's out, mean, rstd, running statistics
    and dy against the float64 reference of the concatenated rows, per column; each rank's
    dgamma / dbeta are its own rows' sums.  rstd of the columns at mean 1e3 x std missed the bar
    by 16.3 (213 + 64 + 300 rows) while a rank's mean crossed the exchange as one f32; it now
    travels as an f32 pair (hi, lo).  Worst ratio on the MI355X: 0.55 (out)."""
    W, m = 3, sum(Ms)
    y, gamma, beta, dout, _, rm0, rv0, kind = R.bn_random(m, c, F32, c + act)
    off = [0, Ms[0], Ms[0] + Ms[1], m]
    gd, bd = gamma.to(DEV), beta.to(DEV)
    ys = [y[off[r]:off[r + 1]].to(DEV).contiguous() for r in range(W)]
    ds = [dout[off[r]:off[r + 1]].to(DEV).contiguous() for r in range(W)]

    def fwd(r, sync):
        o = torch.empty(Ms[r], c, device=DEV)
        mean, rstd = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        rm, rv = rm0.to(DEV), rv0.to(DEV)
        ops.batchnorm_fwd(ys[r], gd, bd, mean, rstd, rm, rv, o, Ms[r], c, act, True, sync=sync)
        return o, mean, rstd, rm, rv

    def bwd(r, mean, rstd, sync):
        dy = torch.empty(Ms[r], c, device=DEV)
        dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        ops.batchnorm_bwd(ys[r], ds[r], gd, bd, mean, rstd, dy, dg, db, Ms[r], c, act, sync=sync)
        return dy, dg, db

    pre = []
    for r in range(W):
        s = SimSync(W, r)
        fwd(r, s)
        pre.append(s.sent)
    got = [fwd(r, SimSync(W, r, [pre[o] for o in range(W) if o != r])) for r in range(W)]
    args = (y, gamma, beta, None, None, act, 1e-5, 0.1, rm0, rv0, True)
    r64, r32 = R.ref_bn_fwd(*args), R.ref_bn_fwd(*args, dtype=F32)
    worst = {}
    ex = R.TANH_ABS if act == ACT_TANH else 0.0
    for r in range(W):
        assert all(torch.equal(got[r][i], got[0][i]) for i in (1, 2, 3, 4))   # same slots, same order
        worst[f"out rank {r}"] = R.worst_ratio_by(got[r][0].cpu(), r64[0][off[r]:off[r + 1]], r32[0][off[r]:off[r + 1]],
                                                  dim=0, extra_abs=ex, kind=kind, pool=R.bn_pool(Ms[r]))
    for i, n in ((1, "mean"), (2, "rstd"), (3, "run_mean"), (4, "run_var")):
        R.by_kind(worst, n, got[0][i].cpu(), r64[i], r32[i], kind)
    mean_d, rstd_d = got[0][1], got[0][2]
    preb = []
    for r in range(W):
        s = SimSync(W, r)
        bwd(r, mean_d, rstd_d, s)
        preb.append(s.sent)
    gb = [bwd(r, mean_d, rstd_d, SimSync(W, r, [preb[o] for o in range(W) if o != r])) for r in range(W)]
    bargs = (y, dout, gamma, beta, mean_d.cpu(), rstd_d.cpu(), None, act, True, m)
    b64, b32 = R.ref_bn_bwd(*bargs), R.ref_bn_bwd(*bargs, dtype=F32)
    exb = R.tanh_bwd_extra(y, dout, gamma, beta, mean_d.cpu(), rstd_d.cpu(), None, 1.0, m) if act == ACT_TANH else None
    for r in range(W):
        sl = slice(off[r], off[r + 1])
        worst[f"dy rank {r}"] = R.worst_ratio_by(gb[r][0].cpu(), b64[0][sl], b32[0][sl], dim=0, kind=kind, pool=R.bn_pool(Ms[r]),
                                                 extra_abs=exb[0][sl] if exb else 0.0)
        largs = (y[sl], dout[sl], gamma, beta, mean_d.cpu(), rstd_d.cpu(), None, act, True, m)
        l64, l32 = R.ref_bn_bwd(*largs), R.ref_bn_bwd(*largs, dtype=F32)
        lex = R.tanh_bwd_extra(y[sl], dout[sl], gamma, beta, mean_d.cpu(), rstd_d.cpu(), None, 1.0, m) if exb else (None,) * 3
        R.by_kind(worst, f"dgamma rank {r}", gb[r][1].cpu(), l64[1], l32[1], None, lex[1])
        R.by_kind(worst, f"dbeta rank {r}", gb[r][2].cpu(), l64[2], l32[2], None, lex[2])
    print(f"\nsyncbn {Ms}x{c} act={act}: " + ", ".join(f"{k} {v[0]:.3f}@{v[1]}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v[0] <= 1, f"{k}: ratio {v[0]:.3f} at column / kind {v[1]}"


# ================================================================ rejections
def _rejected(fn, a, outs, what):
    rc = fn(C.byref(a), stream())
    torch.cuda.synchronize()
    assert rc != 0, f"{what}: accepted"
    assert _lib.lib().tt2_last_error(), f"{what}: no error message"
    for o in outs:
        o.untouched(what)


def _ln_reject_args(dtype=F32, m=8, c=LC):
    g = torch.Generator().manual_seed(1)
    t = [inp(torch.randn(m, c, generator=g), dtype) for _ in range(3)]
    v = [inp(torch.randn(c, generator=g)) for _ in range(2)]
    s = [inp(torch.rand(m, generator=g) + 0.5) for _ in range(2)]
    outs = dict(y=Guarded((m, c), dtype), dx=Guarded((m, c), dtype), dbranch=Guarded((m, c), dtype), dgamma=Guarded((c,)),
                dbeta=Guarded((c,)), dbias=Guarded((c,)))
    return t, v, s, outs


def test_ln_rejections():
    """C != 512 (LayerNorm forward, backward and ln_combine), ln_combine with 3 splits or f32,
    dbias without a branch, a short workspace, finalize_prev on the same workspace: an error each,
    every poisoned output untouched.  m = 0: accepted, nothing written."""
    L = _lib.lib()
    for c in (504, 520):
        (x, br, dy), (gamma, beta), (mean, rstd), o = _ln_reject_args(c=c)
        a = ln_args(F32, 8, c=c, x=x, branch=br, gamma=gamma, beta=beta, y=o["y"], eps=1e-5)
        _rejected(L.tt2_layernorm_fwd, a, o.values(), f"layernorm_fwd c={c}")
        a = ln_args(F32, 8, c=c, x=x, branch=br, dy=dy, gamma=gamma, mean=mean, rstd=rstd, dx=o["dx"], dbranch=o["dbranch"],
                    dgamma=o["dgamma"], dbeta=o["dbeta"], dbias=o["dbias"])
        ws = ln_ws(a)   # noqa: F841
        _rejected(L.tt2_layernorm_bwd, a, o.values(), f"layernorm_bwd c={c}")
    (x, br, dy), (gamma, beta), (mean, rstd), o = _ln_reject_args()
    full = dict(x=x, branch=br, dy=dy, gamma=gamma, mean=mean, rstd=rstd, dx=o["dx"], dbranch=o["dbranch"],
                dgamma=o["dgamma"], dbeta=o["dbeta"], dbias=o["dbias"])
    a = ln_args(F32, 8, **dict(full, branch=None, dbranch=None))
    ws = ln_ws(a)
    _rejected(L.tt2_layernorm_bwd, a, o.values(), "dbias without a branch")
    a = ln_args(F32, 8, **full)
    need = L.tt2_layernorm_bwd_workspace_size(C.byref(a))
    ws = ln_ws(a, need - 4)
    _rejected(L.tt2_layernorm_bwd, a, o.values(), "short workspace")
    a.workspace = None
    a.ws_bytes = need
    _rejected(L.tt2_layernorm_bwd, a, o.values(), "null workspace")
    prev = ln_args(F32, 8, defer_finalize=1, **full)
    ws = ln_ws(prev)
    a = ln_args(F32, 8, finalize_prev=C.addressof(prev), **full)
    a.workspace, a.ws_bytes = prev.workspace, prev.ws_bytes
    _rejected(L.tt2_layernorm_bwd, a, o.values(), "finalize_prev sharing the workspace")
    notdef = ln_args(F32, 8, defer_finalize=0, **full)
    ws2 = ln_ws(notdef)   # noqa: F841
    a = ln_args(F32, 8, finalize_prev=C.addressof(notdef), **full)
    ws3 = ln_ws(a)   # noqa: F841
    _rejected(L.tt2_layernorm_bwd, a, o.values(), "finalize_prev of a call that was not deferred")
    # m = 0: accepted, nothing written
    a = ln_args(F32, 0, **full)
    ws = ln_ws(a)   # noqa: F841
    assert L.tt2_layernorm_bwd(C.byref(a), stream()) == 0
    f = ln_args(F32, 0, x=x, branch=br, gamma=gamma, beta=beta, y=o["y"], eps=1e-5)
    assert L.tt2_layernorm_fwd(C.byref(f), stream()) == 0
    torch.cuda.synchronize()
    for v in o.values():
        v.untouched("m = 0")
    # ln_combine
    for dtype, splits, c, m, ok in ((BF16, 3, LC, 4, False), (F32, 2, LC, 4, False), (BF16, 2, 504, 4, False),
                                    (F16, 2, 520, 4, False), (BF16, 2, LC, 0, True)):
        g = torch.Generator().manual_seed(2)
        xx, part = inp(torch.randn(4, c, generator=g), dtype), inp(torch.randn(16 * 4, c, generator=g))
        bb, gg, be = (inp(torch.randn(c, generator=g)) for _ in range(3))
        y = Guarded((4, c), dtype)
        rc = L.tt2_ln_combine(xx.data_ptr(), part.data_ptr(), splits, bb.data_ptr(), gg.data_ptr(), be.data_ptr(), y.ptr(),
                              m, c, 1e-5, {F32: 0, BF16: 1, F16: 2}[dtype], stream())
        torch.cuda.synchronize()
        assert (rc == 0) == ok, f"ln_combine {dtype} splits={splits} c={c} m={m}: rc {rc}"
        y.untouched(f"ln_combine {dtype} splits={splits} c={c} m={m}")


def test_bn_rejections():
    """C = 12 (not a multiple of 8), C = 2056 (> 2048), res_ld = 84, a pointer offset by 4 bytes,
    the sync entry points with m = 0: an error each, every poisoned output untouched; m = 0 on
    tt2_batchnorm_fwd / _bwd: accepted, nothing written."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(3)

    def case(m, c, ld=None):
        ld = ld or c
        cc = c + 8
        ins = dict(y=inp(torch.randn(8, cc, generator=g))[:, :c], dout=inp(torch.randn(8, cc, generator=g)),
                   gamma=inp(torch.randn(cc, generator=g)), beta=inp(torch.randn(cc, generator=g)),
                   res=inp(torch.randn(8, ld + 8, generator=g)))
        outs = dict(out=Guarded((8, cc)), dy=Guarded((8, cc)), mean=Guarded((cc,)), rstd=Guarded((cc,)),
                    run_mean=Guarded((cc,)), run_var=Guarded((cc,)), dgamma=Guarded((cc,)), dbeta=Guarded((cc,)))
        a = bn_args(F32, m, c, act=ACT_RELU, res_ld=ld, **ins, **outs)
        wsb = wsbuf(1 << 20)
        a.workspace, a.ws_bytes = wsb.data_ptr(), 1 << 20
        return a, outs, (ins, wsb)

    for c, ld, off, what in ((12, None, None, "C = 12"), (2056, None, None, "C = 2056"), (80, 84, None, "res_ld = 84"),
                             (80, None, "y", "y + 4 bytes"), (80, None, "out", "out + 4 bytes"),
                             (80, None, "mean", "mean + 4 bytes"), (80, None, "dy", "dy + 4 bytes"),
                             (80, None, "gamma", "gamma + 4 bytes")):
        a, outs, hold = case(8, c, ld)
        if off:
            setattr(a, off, getattr(a, off) + 4)
        _rejected(L.tt2_batchnorm_fwd, a, outs.values(), "batchnorm_fwd " + what)
        _rejected(L.tt2_batchnorm_bwd, a, outs.values(), "batchnorm_bwd " + what)
    a, outs, hold = case(8, 80)
    a.ws_bytes = L.tt2_batchnorm_workspace_size(C.byref(a)) - 4
    _rejected(L.tt2_batchnorm_fwd, a, outs.values(), "batchnorm_fwd short workspace")
    _rejected(L.tt2_batchnorm_bwd, a, outs.values(), "batchnorm_bwd short workspace")
    a, outs, hold = case(0, 80)
    sync = torch.zeros(6 * 80 + 4, device=DEV)
    a.sync_buf, a.sync_world, a.sync_rank = sync.data_ptr(), 1, 0
    for fn in (L.tt2_batchnorm_fwd_stats, L.tt2_batchnorm_fwd_apply, L.tt2_batchnorm_bwd_stats, L.tt2_batchnorm_bwd_apply):
        _rejected(fn, a, outs.values(), "sync entry point with m = 0")
    assert not sync.any().item()
    assert L.tt2_batchnorm_fwd(C.byref(a), stream()) == 0 and L.tt2_batchnorm_bwd(C.byref(a), stream()) == 0
    torch.cuda.synchronize()
    for v in outs.values():
        v.untouched("m = 0")
