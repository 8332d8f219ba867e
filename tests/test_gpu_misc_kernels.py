"""Every kernel of csrc/reduce.hip, embed.hip, loss.hip, optim.hip and repack.hip on its own
against the float64 references of tests/_misc_refs.py
(validated on the CPU by tests/test_misc_refs.py), through tt2.ops (tt2_reduce_rows, which has
no wrapper, through the C ABI).

Two devices make a subtle error fail outright:
  * exact-arithmetic inputs: the reductions get small-integer inputs, dropout p = 0.5 (scale 2)
    and power-of-two divisors with sum |terms| < 2^24 (asserted), so every partial sum is exact in
    f32 in any order and the result must be torch.equal to the float64 reference cast to the
    output type: a skipped, doubled or misplaced element has no tolerance to hide behind;
  * poisoned outputs with guard bands: outputs are NaN-filled and larger than needed (trailing
    rows, and the columns between n and ld of strided ones); afterwards no NaN is left inside the
    logical extent and every guard element still is NaN.
The non-exact checks (dalpha and the loss on random inputs, the BCE terms) compare per element
against float64 and allow max(4 x the error of the same reference evaluated in float32 on the
CPU, 2 ulp of the output type): _misc_refs.worst_ratio <= 1, printed per test (pytest -s) and
noted in each test's docstring."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import _misc_refs as R  # noqa: E402
from tt2 import _lib, ops  # noqa: E402
from tt2_oracle import dropout_keep  # noqa: E402

DEV = "cuda"
NAN = float("nan")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16]
VOCAB = 80


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, lo, hi, *shape):
    """Integer-valued f32 in [lo, hi] (exact in bf16 / f16 too for |value| <= 256)."""
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def poison(rows, ld, dtype=F32, guard_rows=3):
    """NaN-filled [rows + guard_rows, ld] output buffer."""
    return torch.full((rows + guard_rows, ld), NAN, dtype=dtype, device=DEV)


def check_guard(buf, rows, cols, what=""):
    """buf[:rows, :cols] is fully written (no NaN) and everything else still NaN."""
    b = buf.float().cpu()
    assert not torch.isnan(b[:rows, :cols]).any(), f"{what}: NaN left inside the logical extent"
    assert torch.isnan(b[:rows, cols:]).all(), f"{what}: guard columns written"
    assert torch.isnan(b[rows:]).all(), f"{what}: guard rows written"


def poison1d(n, guard=3):
    """NaN-filled 1-D f32 buffer and its [guard, guard + n) view."""
    buf = torch.full((n + 2 * guard,), NAN, device=DEV)
    return buf, buf[guard:guard + n]


def check_guard1d(buf, n, guard=3, what=""):
    b = buf.cpu()
    assert not torch.isnan(b[guard:guard + n]).any(), f"{what}: NaN left inside the logical extent"
    assert torch.isnan(b[:guard]).all() and torch.isnan(b[guard + n:]).all(), f"{what}: guard written"


# ------------------------------------------------------------------ embedding
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [36, 512])
def test_embedding_fwd(dtype, c):
    """Bit-exact rows; ids -1 and vocab give exactly zero rows (the table row past vocab is NaN)."""
    g = gen(c)
    M = 300
    ids = torch.randint(0, VOCAB, (M,), generator=g)
    ids[:8] = torch.tensor([0, VOCAB - 1, -1, VOCAB, -1, VOCAB, VOCAB + 5, 0])
    table = torch.randn(VOCAB + 1, c, generator=g).to(dtype)
    table[VOCAB] = NAN
    out = poison(M, c, dtype)
    ops.embedding_fwd(ids.to(DEV), table.to(DEV), out, M, VOCAB)
    check_guard(out, M, c, "embedding_fwd")
    ref = R.ref_embedding_fwd(ids, table, VOCAB)
    assert torch.equal(out[:M].cpu(), ref)
    assert not out[:M].cpu()[(ids < 0) | (ids >= VOCAB)].any()


def _id_sets(g, M):
    """name -> ids: uniform; one id in every row (the match list fills whole chunks); an id that
    occurs only in the last rows (the last chunk); a quarter of the ids out of range."""
    uni = torch.randint(0, VOCAB, (M,), generator=g)
    late = torch.randint(0, VOCAB - 1, (M,), generator=g)
    late[late >= 9] += 1                      # no 9 ...
    late[M - 2:] = 9                          # ... but in the last two rows
    oor = uni.clone()
    bad = torch.rand(M, generator=g) < 0.25
    oor[bad] = torch.tensor([-1, VOCAB, 1000, -5])[torch.randint(0, 4, (int(bad.sum()),), generator=g)]
    return {"uniform": uni, "one_id": torch.full((M,), 5), "last_chunk_only": late, "out_of_range": oor}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,c", [(300, 36), (4096, 512), (4097, 520), (9000, 1030)])
def test_embedding_bwd(dtype, m, c):
    """One to three id chunks of 4096 rows and one to three column blocks of 512.  Integer dout:
    equal to the float64 sum; random dout: equal to the float32 sum in increasing row order (the
    header's promise); two runs bit-identical; the pad_idx row and unused rows exactly zero;
    dtable starts as NaN (every row is written, not accumulated)."""
    g = gen(m + c)
    d_int = ints(g, -2, 2, m, c)
    d_rnd = torch.randn(m, c, generator=g).to(dtype).float()
    assert 2.0 * m < R.EXACT_LIMIT              # a column's sum |terms| is at most 2 m
    d_int_d, d_rnd_d = d_int.to(dtype).to(DEV), d_rnd.to(dtype).to(DEV)
    for name, ids in _id_sets(g, m).items():
        ids_d = ids.to(DEV)
        for pad_idx in (0, 7):
            what = f"embedding_bwd {name} pad_idx={pad_idx}"
            dt = poison(VOCAB, c)
            ops.embedding_bwd(ids_d, d_int_d, dt, m, VOCAB, pad_idx)
            check_guard(dt, VOCAB, c, what)
            ref = R.ref_embedding_bwd(ids, d_int, VOCAB, pad_idx)
            assert torch.equal(dt[:VOCAB].cpu(), ref.float()), what
            absent = torch.ones(VOCAB, dtype=torch.bool)
            absent[ids[(ids >= 0) & (ids < VOCAB)]] = False
            absent[pad_idx] = True
            assert not dt[:VOCAB].cpu()[absent].any(), what

            dt1, dt2 = poison(VOCAB, c), poison(VOCAB, c)
            ops.embedding_bwd(ids_d, d_rnd_d, dt1, m, VOCAB, pad_idx)
            ops.embedding_bwd(ids_d, d_rnd_d, dt2, m, VOCAB, pad_idx)
            check_guard(dt1, VOCAB, c, what)
            assert torch.equal(dt1[:VOCAB], dt2[:VOCAB]), what
            assert torch.equal(dt1[:VOCAB].cpu(), R.ref_embedding_bwd_f32_ordered(ids, d_rnd, VOCAB, pad_idx)), what


# ------------------------------------------------------ positional encoding
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,t,c", [(3, 37, 512), (3, 37, 40), (5, 820, 512)])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_posenc_bwd(dtype, b, t, c, p):
    """dx bit-exact (a select and a scale by 2), dalpha exact on integer inputs and within the
    tolerance rule on random ones; (5, 820, 512) has more 8-element chunks than the 1024 x 256
    threads, so the grid-stride loop wraps.  Worst dalpha ratio measured on the MI355X: 0.75
    (1.5 ulp).  The random terms are positive; zero-mean ones (condition number 860 at (3, 37, 40))
    measured 1.36, where other float32 orders on the CPU alone differ by 5 to 10 ulp."""
    g = gen(b * t + c)
    M = b * t
    seed, site = 5, 9
    keep = torch.from_numpy(dropout_keep(seed, site, M * c, p)).view(M, c) if p > 0 else None
    scale = 1.0 / (1.0 - p)
    drop = ops.Drop(torch.tensor([seed], dtype=torch.int32, device=DEV), site, p) if p > 0 else ops.NO_DROP
    worst = 0.0
    for kind in ("int", "random"):
        if kind == "int":
            dout, pe = ints(g, -2, 2, M, c), ints(g, -1, 1, t + 3, c)
        else:
            # positive terms: the sum is well conditioned, as the rule's floor (2 ulp at the
            # reference's magnitude) presumes; under cancellation that floor is below the error of
            # any f32 summation order (signs are covered by the integer case)
            dout = torch.randn(M, c, generator=g).abs().to(dtype).float()
            pe = torch.rand(t + 3, c, generator=g)
        dx64, da64 = R.ref_posenc_bwd(dout, pe, t, keep, scale)
        dx = poison(M, c, dtype)
        dbuf, dalpha = poison1d(1)
        ops.posenc_bwd(dout.to(dtype).to(DEV), pe.to(DEV), dx, dalpha, M, t, drop=drop)
        check_guard(dx, M, c, "posenc_bwd dx")
        check_guard1d(dbuf, 1, what="posenc_bwd dalpha")
        assert torch.equal(dx[:M].cpu(), dx64.to(dtype)), kind
        if kind == "int":
            rows = torch.arange(M) % t
            assert float((dx64 * pe.double()[rows]).abs().sum()) < R.EXACT_LIMIT
            assert dalpha.item() == da64.item()
        else:
            _, da32 = R.ref_posenc_bwd(dout, pe, t, keep, scale, dtype=F32)
            worst = R.worst_ratio(dalpha, da64, da32)
            print(f"posenc_bwd {dtype} ({b},{t},{c}) p={p}: dalpha {R.describe(dalpha, da64, da32)}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("dtype", DTYPES)
def test_posenc_bwd_rejects_c_not_multiple_of_8(dtype):
    """C % 8 != 0 is TT2_E_INVALID before any launch: the outputs stay untouched."""
    M, T, c = 3 * 37, 37, 36
    dx = poison(M, c, dtype)
    dbuf, dalpha = poison1d(1)
    with pytest.raises(_lib.TT2Error):
        ops.posenc_bwd(torch.ones(M, c, dtype=dtype, device=DEV), torch.ones(T, c, device=DEV), dx, dalpha, M, T)
    torch.cuda.synchronize()
    assert torch.isnan(dx.float()).all() and torch.isnan(dbuf).all()


# ------------------------------------------------------ teacher forcing, cast
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,t,c", [(3, 37, 80), (2, 1, 80)])
def test_shift_right(dtype, b, t, c):
    mel = torch.randn(b, t, c, generator=gen(t))
    out = poison(b * t, c, dtype)
    ops.shift_right(mel.to(DEV), out, b, t, c)
    check_guard(out, b * t, c, "shift_right")
    assert torch.equal(out[:b * t].cpu(), R.ref_shift_right(mel).to(dtype))    # bf16 rounding included


@pytest.mark.parametrize("src_dtype", [F32, BF16, F16])
@pytest.mark.parametrize("dst_dtype", [F32, BF16, F16])
def test_cast2d(src_dtype, dst_dtype):
    """Strided cast (the decode path's use): src_ld != dst_ld != n, guard columns untouched."""
    m, n, sld, dld = 37, 81, 96, 88
    src = (torch.randn(m, sld, generator=gen(7)) * 100).to(src_dtype)
    dst = poison(m, dld, dst_dtype)
    ops.cast2d(src.to(DEV), sld, dst, dld, m, n)
    check_guard(dst, m, n, "cast2d")
    assert torch.equal(dst[:m, :n].cpu(), src[:, :n].to(dst_dtype))
    for mm, nn in ((0, n), (m, 0), (0, 0)):                  # m * n == 0: nothing happens
        dst = poison(m, dld, dst_dtype)
        ops.cast2d(src.to(DEV), sld, dst, dld, mm, nn)
        torch.cuda.synchronize()
        assert torch.isnan(dst.float()).all()


# ------------------------------------------------------------------- sums
def _strided_input(g, m, n, layout, dtype):
    """Logical [m, n] integer matrix inside a NaN-filled buffer: 'dense' (ld = n), 'ld+3' (rows not
    16-B aligned: the non-vector path), 'padded' (ld a multiple of 8 above n: 16-B rows whatever n),
    'offset' (base pointer one element off a 16-B boundary: the non-vector path)."""
    ld = {"dense": n, "ld+3": n + 3, "padded": (n + 7) // 8 * 8 + 8, "offset": (n + 7) // 8 * 8}[layout]
    off = 1 if layout == "offset" else 0
    x = ints(g, -2, 2, m, n)
    flat = torch.full((m * ld + off,), NAN)
    flat[off:].view(m, ld)[:, :n] = x
    flat = flat.to(dtype).to(DEV)
    return x, flat, flat[off:], ld


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", [(1, 1), (33, 7), (1000, 81), (2049, 512)])
@pytest.mark.parametrize("layout", ["dense", "ld+3", "padded", "offset"])
def test_colsum(dtype, m, n, layout):
    """Exact column sums with beta 0 / 1 / 0.5 on the 16-B vector path and the scalar one, N off
    the 8- and 64-column tiles; the columns between n and ld hold NaN and must not be read in."""
    g = gen(m + n)
    x, keepalive, xd, ld = _strided_input(g, m, n, layout, dtype)
    assert 2.0 * m + 8 < R.EXACT_LIMIT
    for beta in (0.0, 1.0, 0.5):
        d0 = ints(g, -8, 8, n)
        buf, dst = poison1d(n)
        if beta != 0:
            dst.copy_(d0)
        ops.colsum(xd, ld, m, n, dst, beta=beta)
        check_guard1d(buf, n, what=f"colsum beta={beta}")
        assert torch.equal(dst.cpu(), R.ref_colsum(x, beta, d0).float()), beta
    del keepalive


def test_colsum_short_workspace_is_rejected():
    L = _lib.lib()
    m, n = 1000, 81
    x = torch.ones(m, n, device=DEV)
    buf, dst = poison1d(n)
    need = L.tt2_colsum_workspace_size(m, n)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = L.tt2_colsum(x.data_ptr(), _lib.DT_F32, n, m, n, dst.data_ptr(), 0.0, ws.data_ptr(), need - 1,
                      _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and torch.isnan(buf).all()


def _reduce_rows(src, ld, rows, cols, dst, beta):
    a = _lib.ReduceArgs()
    a.src, a.dst, a.ld, a.rows, a.cols, a.beta = src.data_ptr(), dst.data_ptr(), ld, rows, cols, beta
    _lib.check(_lib.lib().tt2_reduce_rows(C.byref(a), _lib.stream_ptr()), "tt2_reduce_rows")


@pytest.mark.parametrize("rows,cols", [(1024, 1), (5, 3), (1000, 16), (37, 100)])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_reduce_rows(rows, cols, beta):
    """The narrow forms (cw 1 and 4: the Adam norm, dalpha), one full 16-column block and seven
    blocks with a ragged last one; ld > cols with NaN between; beta 1 accumulates."""
    g = gen(rows + cols)
    ld = cols + 5
    x = ints(g, -2, 2, rows, cols)
    src = torch.full((rows, ld), NAN)
    src[:, :cols] = x
    d0 = ints(g, -8, 8, cols)
    buf, dst = poison1d(cols)
    if beta != 0:
        dst.copy_(d0)
    assert 2.0 * rows + 8 < R.EXACT_LIMIT
    _reduce_rows(src.to(DEV), ld, rows, cols, dst, beta)
    check_guard1d(buf, cols, what="reduce_rows")
    assert torch.equal(dst.cpu(), R.ref_reduce_rows(x, beta, d0).float())


def test_reduce_rows_zero_cols_is_a_noop():
    buf, dst = poison1d(4)
    _reduce_rows(torch.ones(8, 4, device=DEV), 4, 8, 0, dst, 0.0)
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


@pytest.mark.parametrize("n", [0, 3, 4, 1027, 65541])
@pytest.mark.parametrize("nparts", [1, 7, 1024])
def test_sumsq_parts(n, nparts):
    """The partial sums add up exactly (float4 body, scalar tail, more blocks than elements);
    parts past nparts stay untouched."""
    g = ints(gen(n + nparts), -2, 2, n)
    assert 4.0 * n < R.EXACT_LIMIT
    buf, parts = poison1d(nparts, guard=5)
    ops.sumsq_parts(g.to(DEV), parts, nparts)
    check_guard1d(buf, nparts, guard=5, what="sumsq_parts")
    assert parts.double().sum().item() == R.ref_sumsq(g).item()


# ------------------------------------------------------------------- loss
def _run_loss(heads, after, target, mel_len, n_mels, heads_ld, gdtype, separate, gscale, misalign=False):
    """heads [M, heads_ld] etc. on the CPU -> (loss[4], g_heads, g_after) from the kernel, with
    every output poisoned and guarded.  misalign: the heads pointer 4 bytes off a 16-B boundary."""
    M = heads.shape[0]
    B, T = target.shape[:2]
    off = 1 if misalign else 0
    hflat = torch.empty(M * heads_ld + off)
    hflat[off:] = heads.reshape(-1)
    hd = hflat.to(DEV)[off:]
    g_heads = poison(M, heads_ld)
    g_after = poison(M, n_mels, gdtype)
    lbuf, loss = poison1d(4, guard=4)
    ops.tts_loss(hd, heads_ld, after.to(DEV), target.to(DEV), mel_len.to(torch.int32).to(DEV), loss, g_heads,
                 g_after, B, T, n_mels, pos_weight=5.0, grad_scale=gscale, separate_grads=separate)
    check_guard(g_heads, M, heads_ld, "tts_loss g_heads")
    check_guard(g_after, M, n_mels, "tts_loss g_after")
    check_guard1d(lbuf, 4, guard=4, what="tts_loss loss_out")
    return loss.cpu(), g_heads[:M].cpu(), g_after[:M].cpu()


def _int_loss_inputs(g, B, T, NM, hld, amp):
    M = B * T
    heads = torch.full((M, hld), NAN)                  # the columns above the stop logit are never read in
    heads[:, :NM] = ints(g, -amp, amp, M, NM)
    heads[:, NM] = ints(g, -30, 30, M)                 # the stable log-sigmoid matters out here
    return heads, ints(g, -amp, amp, M, NM), ints(g, -amp, amp, B, T, NM)


def _check_int_loss(what, heads, after, target, ml, NM, hld, gdtype, separate, gscale, misalign=False):
    """The exact assertions of the integer cases; returns the worst ratio of the BCE terms."""
    B, T = target.shape[:2]
    loss, gh, ga = _run_loss(heads, after, target, ml, NM, hld, gdtype, separate, gscale, misalign)
    l64, gh64, ga64 = R.ref_tts_loss(heads, after, target, ml, NM, 5.0, gscale, separate)
    l32, gh32, _ = R.ref_tts_loss(heads, after, target, ml, NM, 5.0, gscale, separate, dtype=F32)
    valid = (torch.arange(T)[None, :] < ml[:, None]).reshape(-1)
    tg = target.reshape(B * T, NM)
    sq = ((heads[:, :NM] - tg) ** 2 + (after - tg) ** 2)[valid]
    assert float(sq.sum()) < R.EXACT_LIMIT, what
    assert loss[1].item() == l64[1].item() and loss[2].item() == l64[2].item(), (what, loss, l64)
    assert torch.equal(ga, ga64.to(gdtype)), what
    assert torch.equal(ga.double(), ga64), what                    # (nothing lost to the bf16 store either)
    assert torch.equal(gh[:, :NM], gh64[:, :NM].float()), what
    assert not gh[~valid].any() and not ga[~valid].any(), what     # padded frames
    assert not gh[:, NM + 1:].any(), what                          # the columns above the stop logit
    assert loss[0].item() == (loss[1] + loss[2] + loss[3]).item(), what    # f32 sum, bit-exact
    assert torch.isfinite(loss).all() and torch.isfinite(gh).all(), what
    if not valid.any():
        assert not loss.any() and not gh.any() and not ga.any(), what
    print(f"{what}: stop gradient {R.describe(gh[:, NM], gh64[:, NM], gh32[:, NM])}, "
          f"bce {R.describe(loss[3], l64[3], l32[3])}")
    return max(R.worst_ratio(gh[:, NM], gh64[:, NM], gh32[:, NM]), R.worst_ratio(loss[3], l64[3], l32[3]))


LOSS_LENS = {"base": [40, 17, 0, 7], "all_zero": [0, 0, 0, 0], "past_T": [55, 17, 0, 7]}


@pytest.mark.parametrize("heads_ld,misalign", [(68, False), (65, False), (67, False), (68, True)])
@pytest.mark.parametrize("separate", [False, True])
@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("gdtype", DTYPES)
def test_tts_loss_exact(heads_ld, misalign, separate, gscale, gdtype):
    """n_mels = 64 and 64 valid frames (1 / (N n_mels) a power of two): the MSE terms, all of
    g_after and g_heads' mel columns exactly; the vec4 path (heads_ld 68) and the scalar one
    (heads_ld 65 / 67, or a heads pointer 4 bytes off); lengths of 0, all 0 and past T.
    Worst ratios measured on the MI355X: stop gradient 0.25, BCE mean 0.38."""
    B, T, NM = 4, 40, 64
    g = gen(heads_ld + 2 * misalign)
    heads, after, target = _int_loss_inputs(g, B, T, NM, heads_ld, 3)
    worst = 0.0
    for name, lens in LOSS_LENS.items():
        what = f"tts_loss ld={heads_ld} misalign={misalign} sep={separate} gs={gscale} {gdtype} {name}"
        worst = max(worst, _check_int_loss(what, heads, after, target, torch.tensor(lens), NM, heads_ld, gdtype,
                                           separate, gscale, misalign))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("path,b,t,heads_ld,lens", [
    ("vec4", 8, 1400, 96, [1400, 1400, 1400, 1400, 1024, 1024, 544, 0]),       # 8192 valid frames
    ("scalar", 4, 1024, 65, [1024, 512, 512, 0])])                             # 2048 valid frames
@pytest.mark.parametrize("gdtype", DTYPES)
def test_tts_loss_grid_stride_wrap(path, b, t, heads_ld, lens, gdtype):
    """More work items than the 1024 x 256 threads: 11200 x 24 four-column chunks on the vec4
    path, 4096 x 65 elements on the scalar one.  Worst ratios measured on the MI355X: stop
    gradient 0.25, BCE mean 0.27 (0.5 ulp).  This test found the finalize kernel adding its 64 lane
    sums serially: the BCE mean was 2.5 ulp off on the scalar case (ratio 1.27) and 2.8 ulp on the
    vec4 one (0.90); the sums now combine as a tree."""
    NM = 64
    assert (b * t * heads_ld // 4 if path == "vec4" else b * t * heads_ld) > 1024 * 256
    heads, after, target = _int_loss_inputs(gen(t), b, t, NM, heads_ld, 2)
    worst = _check_int_loss(f"tts_loss wrap {path} {gdtype}", heads, after, target, torch.tensor(lens), NM, heads_ld, gdtype,
                            False, 0.5)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("gdtype", DTYPES)
@pytest.mark.parametrize("separate", [False, True])
def test_tts_loss_production_shape(gdtype, separate):
    """n_mels 80 / heads_ld 96 (the model's shape) with random values: every loss term and every
    gradient element under the tolerance rule.  Worst ratios measured on the MI355X: losses
    0.39, g_heads 0.25, g_after 0.25."""
    B, T, NM, hld = 4, 40, 80, 96
    g = gen(80)
    heads = torch.randn(B * T, hld, generator=g) * 2
    after = torch.randn(B * T, NM, generator=g)
    target = torch.randn(B, T, NM, generator=g)
    ml = torch.tensor([40, 17, 1, 7])
    loss, gh, ga = _run_loss(heads, after, target, ml, NM, hld, gdtype, separate, 1.0)
    l64, gh64, ga64 = R.ref_tts_loss(heads, after, target, ml, NM, 5.0, 1.0, separate)
    l32, gh32, ga32 = R.ref_tts_loss(heads, after, target, ml, NM, 5.0, 1.0, separate, dtype=F32)
    ratios = {"loss": R.worst_ratio(loss, l64, l32), "g_heads": R.worst_ratio(gh, gh64, gh32),
              "g_after": R.worst_ratio(ga, ga64, ga32, gdtype)}
    print(f"tts_loss 80/96 {gdtype} sep={separate}: loss {R.describe(loss, l64, l32)}, g_heads "
          f"{R.describe(gh, gh64, gh32)}, g_after {R.describe(ga, ga64, ga32, gdtype)}")
    assert not gh[:, NM + 1:].any()
    assert max(ratios.values()) <= 1.0, ratios
