"""CPU: the host side of the LayerNorm, BatchNorm, reduction, embedding, loss, optimizer and repack
entry points (csrc/layernorm.hip, batchnorm.hip, reduce.hip, embed.hip, loss.hip, optim.hip,
repack.hip, comm_standin.hip): every request they refuse with TT2_E_INVALID before a launch, every
zero-size request they answer with TT2_OK without one, and their size queries against the formulas of
include/tt2_capi.h.  test_capi_trim.py's pattern: _lib.load(), no device, no compute calls (there is
no GPU here, and a launch would fail otherwise than with E_INVALID)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    import os
    from tt2 import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build_lib
        build_lib.build()
    return _lib


@pytest.fixture(scope="module")
def mem():
    """Host memory the refused calls may point at (never read: they are refused before a launch);
    the address is 64-B aligned."""
    buf = (ctypes.c_char * 8192)()
    base = ctypes.addressof(buf)
    p = (base + 63) & ~63
    return buf, p


def _clone(a, **kw):
    b = type(a).from_buffer_copy(a)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _refused(lib, L, call, name):
    """call() is refused with E_INVALID and the message names `name`; an unrelated refused call first,
    so that the message read afterwards belongs to the call under test."""
    E = lib.E_INVALID
    assert L.tt2_dtw(None, None) == E and b"tt2_dtw" in L.tt2_last_error()
    assert call() == E
    assert name.encode() in L.tt2_last_error(), (name, L.tt2_last_error())


def _ln(lib, p, **kw):
    a = lib.LnArgs()
    a.x = a.branch = a.dy = a.y = a.dx = a.dbranch = a.gamma = a.beta = a.mean = a.rstd = p
    a.dgamma = a.dbeta = a.dbias = a.workspace = p
    a.ws_bytes = 2 ** 62
    a.m, a.c, a.dtype, a.eps = 64, 512, lib.DT_BF16, 1e-5
    return _clone(a, **kw)


def _bn(lib, p, **kw):
    a = lib.BnArgs()
    a.y = a.dout = a.out = a.dy = a.gamma = a.beta = a.mean = a.rstd = a.run_mean = a.run_var = p
    a.dgamma = a.dbeta = a.workspace = a.sync_buf = p
    a.ws_bytes = 2 ** 62
    a.m, a.c, a.dtype, a.out_dtype, a.dout_dtype, a.training = 100, 512, lib.DT_BF16, lib.DT_BF16, lib.DT_BF16, 1
    a.eps, a.momentum, a.sync_world, a.sync_rank = 1e-5, 0.1, 2, 1
    return _clone(a, **kw)


def test_e_invalid_value(lib):
    assert lib.E_INVALID == -1


def test_layernorm_refusals_and_zero_sizes(lib, mem):
    L = lib.load()
    _, p = mem
    ln = lambda **kw: _ln(lib, p, **kw)
    for c in (0, 256, 511, 513, 1024):
        _refused(lib, L, lambda: L.tt2_layernorm_fwd(ctypes.byref(ln(c=c)), None), "tt2_layernorm")
        _refused(lib, L, lambda: L.tt2_layernorm_bwd(ctypes.byref(ln(c=c)), None), "tt2_layernorm")
    need = L.tt2_layernorm_bwd_workspace_size(ctypes.byref(ln()))
    assert need == 4 * 3 * 512 * 4
    for kw in (dict(workspace=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(branch=None),
               dict(m=0, workspace=None)):
        _refused(lib, L, lambda: L.tt2_layernorm_bwd(ctypes.byref(ln(**kw)), None), "tt2_layernorm_bwd")
    # finalize_prev: not deferred, another c, no workspace, or the workspace this call overwrites
    def chained(q, **kw):
        a = ln(**kw)
        a.finalize_prev = ctypes.addressof(q)
        return L.tt2_layernorm_bwd(ctypes.byref(a), None)
    other = p + 4096
    for q in (ln(defer_finalize=0, workspace=other), ln(defer_finalize=1, workspace=other, c=256),
              ln(defer_finalize=1, workspace=None), ln(defer_finalize=1, m=1)):
        _refused(lib, L, lambda: chained(q), "tt2_layernorm_bwd")
        _refused(lib, L, lambda: chained(q, m=0), "tt2_layernorm_bwd")
    for kw in (dict(defer_finalize=0), dict(defer_finalize=1, workspace=None), dict(defer_finalize=0, m=0)):
        _refused(lib, L, lambda: L.tt2_layernorm_bwd_finalize(ctypes.byref(ln(**kw)), None),
                 "tt2_layernorm_bwd_finalize")
    assert L.tt2_layernorm_fwd(ctypes.byref(ln(m=0)), None) == 0
    assert L.tt2_layernorm_fwd(ctypes.byref(ln(m=0, dtype=lib.DT_F32, branch=None)), None) == 0
    assert L.tt2_layernorm_bwd_finalize(ctypes.byref(ln(m=0, defer_finalize=1)), None) == 0


def test_ln_combine_refusals_and_zero_sizes(lib, mem):
    L = lib.load()
    _, p = mem

    def rc(x=p, part=p, splits=8, bias=p, gamma=p, beta=p, y=p, m=4, c=512, dtype=None):
        return L.tt2_ln_combine(x, part, splits, bias, gamma, beta, y, m, c, 1e-5,
                                lib.DT_BF16 if dtype is None else dtype, None)

    refused = [dict(c=256), dict(c=0), dict(c=1024), dict(dtype=lib.DT_F32), dict(dtype=7),
               dict(splits=3), dict(splits=0), dict(splits=32), dict(splits=-1), dict(splits=3, dtype=lib.DT_F16)]
    refused += [{k: None} for k in ("x", "part", "bias", "gamma", "beta", "y")]
    for kw in refused:
        _refused(lib, L, lambda: rc(**kw), "tt2_ln_combine")
    _refused(lib, L, lambda: rc(m=0, c=256), "tt2_ln_combine")
    _refused(lib, L, lambda: rc(m=0, x=None), "tt2_ln_combine")
    _refused(lib, L, lambda: rc(m=0, dtype=lib.DT_F32), "tt2_ln_combine")
    assert rc(m=0) == 0 and rc(m=0, dtype=lib.DT_F16) == 0 and rc(m=-1) == 0
    assert rc(m=0, splits=3) == 0   # the rows are looked at first: nothing to combine


def test_batchnorm_refusals_and_zero_sizes(lib, mem):
    L = lib.load()
    _, p = mem
    bn = lambda **kw: _bn(lib, p, **kw)
    need = L.tt2_batchnorm_workspace_size(ctypes.byref(bn()))
    layout = [dict(c=12), dict(c=511), dict(c=2056), dict(c=4096), dict(res=p, res_ld=4), dict(res=p, res_ld=513)]
    layout += [{k: p + 8} for k in ("y", "out", "res", "dout", "dy", "gamma", "beta", "mean", "rstd", "dgamma", "dbeta")]
    layout += [dict(y=p + 2), dict(gamma=p + 4)]
    for fn, name in ((L.tt2_batchnorm_fwd, "tt2_batchnorm_fwd"), (L.tt2_batchnorm_bwd, "tt2_batchnorm_bwd")):
        for kw in [dict(workspace=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)] + layout:
            _refused(lib, L, lambda: fn(ctypes.byref(bn(**kw)), None), name)
        for kw in (dict(m=0), dict(m=-3), dict(m=0, c=12), dict(m=0, workspace=None), dict(m=0, training=0)):
            assert fn(ctypes.byref(bn(**kw)), None) == 0, (name, kw)
    # the evaluation forward needs no workspace, its layout rules hold all the same; the backward always needs one
    for kw in layout:
        _refused(lib, L, lambda: L.tt2_batchnorm_fwd(ctypes.byref(bn(training=0, workspace=None, **kw)), None),
                 "tt2_batchnorm_fwd")
    _refused(lib, L, lambda: L.tt2_batchnorm_bwd(ctypes.byref(bn(training=0, workspace=None)), None),
             "tt2_batchnorm_bwd")
    # chunk statistics from a GEMM epilogue: the workspace is sized by stats_rows
    need256 = L.tt2_batchnorm_workspace_size(ctypes.byref(bn(m=1000, stats_rows=256)))
    assert need256 == 4 * 2 * 512 * 4
    for fn, name in ((L.tt2_batchnorm_fwd, "tt2_batchnorm_fwd"), (L.tt2_batchnorm_bwd, "tt2_batchnorm_bwd")):
        _refused(lib, L, lambda: fn(ctypes.byref(bn(m=1000, stats_rows=256, ws_bytes=need256 - 1)), None), name)


def test_sync_batchnorm_refusals(lib, mem):
    L = lib.load()
    _, p = mem
    bn = lambda **kw: _bn(lib, p, **kw)
    need = L.tt2_batchnorm_workspace_size(ctypes.byref(bn()))
    refused = [dict(m=0), dict(m=-1), dict(training=0), dict(sync_rank=2), dict(sync_rank=3), dict(sync_rank=-1),
               dict(sync_world=0, sync_rank=0), dict(sync_world=1, sync_rank=1), dict(sync_buf=None),
               dict(sync_buf=p + 4), dict(sync_buf=p + 8), dict(workspace=None), dict(ws_bytes=need - 1),
               dict(c=12), dict(c=4096), dict(res=p, res_ld=12), dict(y=p + 8), dict(dbeta=p + 8),
               dict(m=0, training=0), dict(m=0, sync_buf=None)]
    for name in ("tt2_batchnorm_fwd_stats", "tt2_batchnorm_fwd_apply", "tt2_batchnorm_bwd_stats",
                 "tt2_batchnorm_bwd_apply"):
        fn = getattr(L, name)
        for kw in refused:
            _refused(lib, L, lambda: fn(ctypes.byref(bn(**kw)), None), name)


def test_reduce_embed_cast_refusals_and_zero_sizes(lib, mem):
    L = lib.load()
    _, p = mem
    r = lib.ReduceArgs()
    r.src = r.dst = p
    r.ld, r.rows, r.cols, r.beta = 16, 100, 0, 0.0
    assert L.tt2_reduce_rows(ctypes.byref(r), None) == 0
    assert L.tt2_reduce_rows(ctypes.byref(_clone(r, cols=-5)), None) == 0
    assert L.tt2_reduce_rows(ctypes.byref(_clone(r, cols=0, src=None, dst=None)), None) == 0

    def colsum(m=1000, n=80, ws=p, ws_bytes=2 ** 62, dtype=None):
        return L.tt2_colsum(p, lib.DT_BF16 if dtype is None else dtype, n, m, n, p, 0.0, ws, ws_bytes, None)

    for m, n in ((1000, 80), (1, 1), (12800, 2048), (31, 64), (33, 65)):
        need = L.tt2_colsum_workspace_size(m, n)
        for dt in (lib.DT_BF16, lib.DT_F32):
            _refused(lib, L, lambda: colsum(m, n, ws_bytes=need - 1, dtype=dt), "tt2_colsum")
        _refused(lib, L, lambda: colsum(m, n, ws_bytes=0), "tt2_colsum")
    assert colsum(n=0) == 0 and colsum(n=0, ws=None, ws_bytes=0) == 0 and colsum(n=-1, ws_bytes=0) == 0

    ids = dout = dtable = p
    for dt in (lib.DT_BF16, lib.DT_F32):
        assert L.tt2_embedding_bwd(ids, dout, dtable, 100, 512, 0, 0, dt, None) == 0
        assert L.tt2_embedding_bwd(ids, dout, dtable, 100, 512, -1, 0, dt, None) == 0
        assert L.tt2_embedding_bwd(ids, dout, dtable, 100, 0, 40, 0, dt, None) == 0
    for m, n in ((0, 80), (80, 0), (0, 0)):
        for sdt, ddt in ((lib.DT_F32, lib.DT_BF16), (lib.DT_BF16, lib.DT_F32), (lib.DT_F16, lib.DT_F16)):
            assert L.tt2_cast2d(p, sdt, 80, p, ddt, 80, m, n, None) == 0
    assert L.tt2_cast2d(None, lib.DT_F32, 0, None, lib.DT_F32, 0, 0, 0, None) == 0
    assert L.tt2_conv_weight_flip(p, p + 4096, 0, 512, 5, lib.DT_BF16, None) == 0
    assert L.tt2_conv_weight_flip(p, p + 4096, 512, 512, 0, lib.DT_F32, None) == 0
    assert L.tt2_step_bump(None, None, None) == 0


def test_posenc_loss_adam_refusals(lib, mem):
    L = lib.load()
    _, p = mem
    a = lib.PeArgs()
    a.x = a.dout = a.out = a.dx = a.alpha = a.pe = a.dalpha = a.workspace = p
    a.ws_bytes = 2 ** 62
    a.m, a.c, a.t, a.dtype = 128, 512, 64, lib.DT_BF16
    need = L.tt2_posenc_bwd_workspace_size()
    for kw in (dict(workspace=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(c=12), dict(c=511), dict(c=1),
               dict(m=2 ** 22, c=512), dict(m=2 ** 31 - 1, c=8), dict(dtype=lib.DT_F32, c=4)):
        _refused(lib, L, lambda: L.tt2_posenc_bwd(ctypes.byref(_clone(a, **kw)), None), "tt2_posenc_bwd")

    l = lib.LossArgs()
    l.heads = l.mel_after = l.target = l.mel_len = l.loss_out = l.g_heads = l.g_after = l.workspace = p
    l.ws_bytes = 2 ** 62
    l.heads_ld, l.batch, l.t, l.n_mels, l.grad_dtype, l.pos_weight, l.grad_scale = 96, 2, 50, 80, lib.DT_BF16, 5.0, 1.0
    need = L.tt2_loss_workspace_size()
    for kw in (dict(heads_ld=80), dict(heads_ld=0), dict(n_mels=96), dict(workspace=None), dict(ws_bytes=need - 1),
               dict(ws_bytes=0), dict(grad_dtype=lib.DT_F32, ws_bytes=need - 1)):
        _refused(lib, L, lambda: L.tt2_tts_loss(ctypes.byref(_clone(l, **kw)), None), "tt2_tts_loss")

    d = lib.AdamArgs()
    d.params = d.grads = d.exp_avg = d.exp_avg_sq = d.shadow_bf16 = d.step = d.workspace = p
    d.ws_bytes = 2 ** 62
    d.n, d.lr, d.beta1, d.beta2, d.eps, d.clip_norm = 1024, 1e-3, 0.9, 0.98, 1e-9, 1.0
    need = L.tt2_adam_workspace_size()
    refused = [{k: p + 8} for k in ("params", "grads", "exp_avg", "exp_avg_sq")]
    refused += [dict(params=p + 4), dict(shadow_bf16=p + 4), dict(shadow_bf16=p + 2), dict(clip_norm=0.0, grads=p + 8),
                dict(workspace=None), dict(ws_bytes=need - 1), dict(ws_bytes=0),
                dict(norm_parts=p, norm_nparts=0), dict(norm_parts=p, norm_nparts=-1)]
    for kw in refused:
        _refused(lib, L, lambda: L.tt2_adam_step(ctypes.byref(_clone(d, **kw)), None), "tt2_adam_step")

    for g, n, parts, nparts in ((None, 16, p, 4), (p, 16, None, 4), (p, 16, p, 0), (p, 16, p, -1), (p, -1, p, 4),
                                (p + 4, 16, p, 4), (p + 8, 0, p, 4)):
        _refused(lib, L, lambda: L.tt2_sumsq_parts(g, n, parts, nparts, None), "tt2_sumsq_parts")
    for gate, op in ((None, 0), (None, 1), (p, 2), (p, -1)):
        _refused(lib, L, lambda: L.tt2_adam_gate(gate, p, op, None), "tt2_adam_gate")


def test_repack_and_standin_refusals(lib, mem):
    L = lib.load()
    _, p = mem
    q = p + 4096

    def jobs(n, **kw):
        arr = (lib.WflipJob * max(n, 1))()
        for j in range(max(n, 1)):
            arr[j].w, arr[j].wd, arr[j].cout, arr[j].cin, arr[j].k = p, q, 512, 512, 5
        for k, v in kw.items():
            setattr(arr[max(n, 1) - 1], k, v)   # the last job is the bad one
        return arr

    name = "tt2_conv_weight_flip_batch"
    for dt in (lib.DT_BF16, lib.DT_F32):
        _refused(lib, L, lambda: L.tt2_conv_weight_flip_batch(jobs(17), 17, dt, None), name)
        _refused(lib, L, lambda: L.tt2_conv_weight_flip_batch(None, 1, dt, None), name)
        for n in (1, 3, 16):
            for kw in (dict(cout=0), dict(cin=0), dict(k=0), dict(cout=-1), dict(w=None), dict(wd=None), dict(wd=p)):
                _refused(lib, L, lambda: L.tt2_conv_weight_flip_batch(jobs(n, **kw), n, dt, None), name)
        assert L.tt2_conv_weight_flip_batch(jobs(1), 0, dt, None) == 0
        assert L.tt2_conv_weight_flip_batch(None, 0, dt, None) == 0
        assert L.tt2_conv_weight_flip_batch(None, -1, dt, None) == 0

    name = "tt2_conv_weight_pack"
    for w, wp, dt in ((None, q, lib.DT_BF16), (p, None, lib.DT_BF16), (p, p, lib.DT_F32), (p, q, lib.DT_F16), (p, q, 9),
                      (p, q, -1)):
        _refused(lib, L, lambda: L.tt2_conv_weight_pack(w, wp, 512, 80, 5, dt, None), name)
    for cout, cin, k in ((0, 80, 5), (512, 0, 5), (512, 80, 0), (-1, 80, 5)):
        assert L.tt2_conv_weight_pack(p, q, cout, cin, k, lib.DT_BF16, None) == 0
        assert L.tt2_conv_weight_pack(None, None, cout, cin, k, lib.DT_F16, None) == 0   # sizes are looked at first

    name = "tt2_comm_standin"
    for src, scratch, seconds, wgs in ((None, q, 0.0, 8), (p, None, 0.0, 8), (p, q, 0.0, 0), (p, q, 0.0, -1),
                                       (p, q, 0.0, 1025), (p, q, -1e-9, 8), (p, q, 1.0001, 8), (p + 8, q, 0.0, 8),
                                       (p, q + 4, 0.0, 8)):
        _refused(lib, L, lambda: L.tt2_comm_standin(src, scratch, 4096, seconds, wgs, None, None), name)


def test_size_queries(lib, mem):
    """Against include/tt2_capi.h: TT2_BN_ROWS_PER_CHUNK 64, TT2_PE_BWD_BLOCKS / TT2_LOSS_BLOCKS /
    TT2_ADAM_NORM_BLOCKS 1024."""
    L = lib.load()
    _, p = mem
    for m in (0, 1, 15, 16, 17, 4095, 4096, 4097, 12800, 2 ** 31 - 16):
        for c in (512, 256, 0):
            got = L.tt2_layernorm_bwd_workspace_size(ctypes.byref(_ln(lib, p, m=m, c=c)))
            assert got == min(256, -(-m // 16)) * 3 * c * 4, (m, c)

    def bn_rows_per(m):   # at most 64 rows per chunk, halved down to 8 while that leaves fewer than 256 chunks
        rp = 64
        while rp > 8 and -(-m // rp) < 256:
            rp //= 2
        return rp

    for m in (0, 1, 7, 8, 9, 2048, 4080, 4081, 8160, 8161, 12800, 16320, 16321, 100000):
        for c in (8, 80, 512, 2048):
            for sr in (0, -1, 256, 64, 1000):
                got = L.tt2_batchnorm_workspace_size(ctypes.byref(_bn(lib, p, m=m, c=c, stats_rows=sr)))
                rp = sr if sr > 0 else bn_rows_per(m)
                assert got == -(-m // rp) * 2 * c * 4, (m, c, sr)
    assert [bn_rows_per(m) for m in (1, 4080, 4081, 8160, 8161, 16320, 16321)] == [8, 8, 16, 16, 32, 32, 64]
    for w, eff in ((0, 1), (-2, 1), (1, 1), (8, 8)):
        for c in (8, 80, 512, 2048):
            got = L.tt2_batchnorm_sync_size(ctypes.byref(_bn(lib, p, c=c, sync_world=w, sync_rank=0)))
            assert got == ((4 * eff + 2) * c + 4) * 4, (w, c)

    def colsum_chunks(m, n):   # about 1024 work groups of 64 columns, 32 or more rows each
        return max(1, min(max(1, 1024 // (-(-n // 64))), -(-m // 32)))

    for m, n in ((1, 1), (0, 5), (31, 64), (32, 64), (33, 65), (1000, 80), (12800, 512), (12800, 2048), (100000, 1),
                 (64, 70000), (2 ** 20, 81)):
        assert L.tt2_colsum_workspace_size(m, n) == colsum_chunks(m, n) * n * 4, (m, n)
    assert L.tt2_posenc_bwd_workspace_size() == 1024 * 4
    assert L.tt2_loss_workspace_size() == 1024 * 4 * 4
    assert L.tt2_adam_workspace_size() == (1024 + 16) * 4
