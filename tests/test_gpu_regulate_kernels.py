"""Length-regulator kernels (tt2_regulate_plan / _fwd / _bwd) against the references of
tests/_regulate_refs.py (GPU), by direct C-ABI calls on hand-built buffers.  Every comparison is bit
for bit: the plan in integers, the forward a copy of bits, the backward against the numpy float32
model that adds in ascending frame order -- on exact problems and on problems of mixed magnitude whose
result depends on the order (tests/test_regulate_refs.py asserts both premises and that this bar
rejects each of twelve mutants).

Buffers: every tensor is a strided region of a flat buffer between guard bands, the whole buffer
poisoned first (NaN for values, -77 for integers, 2^31 - 1 for durations, which therefore hold a huge
value in their pad columns and at and past key_len[b]).  The pad widths differ per buffer; in the
"odd" memory layout the leading dimensions are odd and the bases sit 4 bytes (src) and 12 or 6 bytes
(dst) off 16-byte alignment, so rows start at every alignment; in the "sliced" layout the tensors are
column slices of wider, 16-byte aligned buffers (the 16-byte chunk path where dim allows).  h rows that
no frame names are NaN, and so are dy rows at and past frames[b].  After a call every input buffer is
unchanged, every byte of an output buffer outside the tensor is unchanged, and outputs that were not
asked for are untouched."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _regulate_refs as R  # noqa: E402
from tt2 import _lib  # noqa: E402

GUARD = 64
SENT = -77
NP = {"f32": np.float32, "bf16": np.uint16}
DT = {"f32": _lib.DT_F32, "bf16": _lib.DT_BF16}


def poison(dtype):
    if dtype == np.int32:
        return SENT
    return np.float32(np.nan) if dtype == np.float32 else np.uint16(0x7FC1)


class Buf:
    """A strided tensor inside a flat poisoned buffer with guard bands, uploaded as raw integers."""

    def __init__(self, shape, dtype, strides, shift=0, fill=None, data=None):
        self.shape, self.dtype, self.strides, self.off = tuple(shape), np.dtype(dtype), tuple(strides), GUARD + shift
        n = 0 if 0 in self.shape else 1 + sum((s - 1) * st for s, st in zip(self.shape, self.strides))
        self.before = np.full(self.off + n + GUARD, poison(self.dtype.type) if fill is None else fill, dtype=self.dtype)
        if data is not None:
            self.region(self.before)[...] = np.asarray(data).astype(self.dtype, copy=False).reshape(self.shape)
        self.raw = {4: np.int32, 2: np.int16}[self.dtype.itemsize]
        self.dev = torch.from_numpy(self.before.view(self.raw).copy()).cuda()

    def region(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.off:], self.shape, tuple(s * self.dtype.itemsize for s in self.strides))

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.off * self.dtype.itemsize

    def fetch(self):
        return self.dev.cpu().numpy().view(self.dtype)

    def unchanged(self):
        return np.array_equal(R.bits(self.fetch()), R.bits(self.before))

    def result(self):
        """The tensor after the call; asserts that nothing outside it was written."""
        after = self.fetch().copy()
        out = self.region(after).copy()
        self.region(after)[...] = self.region(self.before)
        assert np.array_equal(R.bits(after), R.bits(self.before)), "written outside the tensor (pad columns or guard bands)"
        return out


def odd(n, pad):
    return n + pad + ((n + pad + 1) % 2)


def call(name, a, expect=0):
    L = _lib.lib()
    rc = getattr(L, name)(ctypes.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (name, rc, L.tt2_last_error())
    if expect:
        assert L.tt2_last_error().startswith(name.encode() + b":")


# ------------------------------------------------------------------------------------------- plan
def run_plan(p, want=("index", "frames", "total"), expect=0, **override):
    d, key_len, tx, n_out = p["durations"], p["key_len"], p["tx"], p["n_out"]
    B = len(d)
    dur = Buf((B, tx), np.int32, (odd(tx, 4), 1), fill=R.HUGE, data=d)
    ends = Buf((B, tx), np.int32, (odd(tx, 2), 1))
    index = Buf((B, n_out), np.int32, (odd(n_out, 6), 1), shift=1)
    frames, total = Buf((B,), np.int32, (1,)), Buf((B,), np.int32, (1,), shift=3)
    klen = Buf((B,), np.int32, (1,), data=key_len) if key_len is not None else None
    a = _lib.RegulatePlanArgs()
    a.durations, a.key_len, a.ends = dur.ptr, (klen.ptr if klen else None), ends.ptr
    a.index = index.ptr if "index" in want else None
    a.frames = frames.ptr if "frames" in want else None
    a.total = total.ptr if "total" in want else None
    a.dur_ld, a.ends_ld, a.index_ld = dur.strides[0], ends.strides[0], index.strides[0]
    a.batch, a.tx, a.n_out = B, tx, n_out
    for k, v in override.items():
        setattr(a, k, v)
    call("tt2_regulate_plan", a, expect)
    assert dur.unchanged() and (klen is None or klen.unchanged()), "an input was written"
    outs = {"ends": ends, "index": index, "frames": frames, "total": total}
    got = {}
    for k, buf in outs.items():
        if expect or (k != "ends" and k not in want):
            assert buf.unchanged(), f"{k} was not asked for (or the call was refused) and was written"
        else:
            got[k] = buf.result()
    return got


@pytest.mark.parametrize("n_out", R.PLAN_NOUT)
@pytest.mark.parametrize("tx", R.PLAN_TX)
def test_plan_bit_for_bit(tx, n_out):
    for p in R.plan_problems(tx, n_out):
        want = R.plan_ref(p["durations"], p["key_len"], tx, n_out)
        got = run_plan(p)
        assert R.reject(got, want) == [], (p["names"], p["key_len"])


def test_plan_optional_outputs_stay_untouched():
    p = R.plan_problems(65, 257)[0]
    want = R.plan_ref(p["durations"], p["key_len"], 65, 257)
    for asked in ((), ("index",), ("frames",), ("total",), ("frames", "total")):
        got = run_plan(p, want=asked)
        assert sorted(got) == sorted(("ends",) + asked)
        assert R.reject(got, {k: want[k] for k in got}) == [], asked


def test_plan_wide_index_takes_every_slice():
    """n_out beyond 64 slices of 1024 frames: every work group of an utterance loops."""
    tx, n_out = 300, 70001
    rng = np.random.default_rng(5)
    d = rng.integers(0, 500, size=(2, tx))
    p = {"durations": d, "key_len": [tx, 250], "tx": tx, "n_out": n_out}
    want = R.plan_ref(d, p["key_len"], tx, n_out)
    assert want["frames"][0] == n_out and 0 < want["frames"][1] < n_out
    assert R.reject(run_plan(p), want) == []


def test_plan_refusals_leave_the_outputs_untouched():
    p = R.plan_problems(65, 37)[1]
    E = _lib.E_INVALID
    for kw in (dict(tx=4097), dict(dur_ld=64), dict(ends_ld=10), dict(index_ld=36), dict(n_out=-1), dict(batch=-1),
               dict(durations=None), dict(ends=None)):
        assert run_plan(p, expect=E, **kw) == {}


# ------------------------------------------------------------------------------- forward / backward
@functools.lru_cache(maxsize=None)
def layout(name):
    return R.layout(name)


def strides3(rows, dim, mem, pad):
    """Row and batch strides (elements) and the base shift of a [B, rows, dim] tensor."""
    if mem == "sliced":                        # columns 8 .. 8 + dim of rows of a wider, aligned buffer
        ld = (dim + 7) // 8 * 8 + 8 * pad
        return ld, rows * ld + 16, 8
    ld = odd(dim, pad)
    return ld, rows * ld + 3, None


def run_rows(entry, src, mp, dst_rows, tx, n_out, dtype, mem, expect=0, src_null=False, map_null=False, override=None):
    """One tt2_regulate_fwd (mp = index) or _bwd (mp = ends) call: src [B, rows, dim] numpy of NP[dtype],
    mp [B, cols] int32 -> dst [B, dst_rows, dim]."""
    B, src_rows, dim = src.shape
    np_dt = NP[dtype]
    unit = 1 if dtype == "f32" else 2                      # elements in 4 bytes
    s_ld, s_bs, s_shift = strides3(src_rows, dim, mem, 1)
    d_ld, d_bs, d_shift = strides3(dst_rows, dim, mem, 2)
    sb = Buf(src.shape, np_dt, (s_bs, s_ld, 1), shift=unit if s_shift is None else s_shift, data=R.bits(src).view(np_dt))
    db = Buf((B, dst_rows, dim), np_dt, (d_bs, d_ld, 1), shift=3 if d_shift is None else d_shift)
    mb = Buf(mp.shape, np.int32, (odd(mp.shape[1], 2), 1), shift=1, data=mp)
    a = _lib.RegulateArgs()
    a.src, a.dst, a.map = (None if src_null else sb.ptr), db.ptr, (None if map_null else mb.ptr)
    a.src_ld, a.src_bs, a.dst_ld, a.dst_bs, a.map_ld = s_ld, s_bs, d_ld, d_bs, mb.strides[0]
    a.batch, a.tx, a.n_out, a.dim, a.dtype = B, tx, n_out, dim, DT[dtype]
    for k, v in (override or {}).items():
        setattr(a, k, v)
    if mem == "sliced":
        assert sb.ptr % 16 == 0 and db.ptr % 16 == 0
    else:
        assert sb.ptr % 16 == 4 and db.ptr % 16 in (12, 6)
    call(entry, a, expect)
    assert sb.unchanged() and mb.unchanged(), "an input was written"
    if expect:
        assert db.unchanged(), "a refused call wrote"
        return None
    return db.result()


CASES = [(lay, dim, dtype, mem) for lay in R.LAYOUTS for dim in R.DIMS for dtype in ("f32", "bf16")
         for mem in ("odd", "sliced")]


@pytest.mark.parametrize("lay,dim,dtype,mem", CASES)
def test_forward_is_a_copy_of_bits(lay, dim, dtype, mem):
    L = layout(lay)
    h = R.fwd_problem(L, dim, dtype)
    want = R.fwd_ref(h, L["plan"]["index"], L["tx"])
    got = run_rows("tt2_regulate_fwd", h, L["plan"]["index"], L["n_out"], L["tx"], L["n_out"], dtype, mem)
    assert R.reject({"y": got}, {"y": want}) == []


def test_forward_reads_nothing_out_of_bounds_whatever_index_holds():
    rng = np.random.default_rng(2)
    B, tx, n_out, dim = 2, 5, 300, 8
    h = rng.normal(size=(B, tx, dim)).astype(np.float32)
    index = rng.integers(-3, tx + 3, size=(B, n_out)).astype(np.int32)
    index[0, :4] = [R.INT32_MAX, R.INT32_MIN, tx, -1]
    want = R.fwd_ref(h, index, tx)
    assert not want[index >= tx].any() and not want[index < 0].any()
    for mem in ("odd", "sliced"):
        got = run_rows("tt2_regulate_fwd", h, index, n_out, tx, n_out, "f32", mem)
        assert R.reject({"y": got}, {"y": want}) == []


@pytest.mark.parametrize("kind", ["exact", "mixed"])
@pytest.mark.parametrize("lay,dim,dtype,mem", CASES)
def test_backward_bit_for_bit_against_the_float32_model(lay, dim, dtype, mem, kind):
    L = layout(lay)
    ends, n_out = L["plan"]["ends"], L["n_out"]
    if kind == "exact":
        dy = R.bwd_exact_problem(L, dim, dtype)
        assert R.is_exact(dy, ends, n_out, dtype)
    else:
        dy = R.bwd_mixed_problem(L, dim, dtype)
    want = R.bwd_model(dy, ends, n_out)
    got = run_rows("tt2_regulate_bwd", dy, ends, L["tx"], L["tx"], n_out, dtype, mem)
    assert R.reject({"dh": got}, {"dh": want}) == []
    if kind == "mixed" and dim == 8:                        # repeatability over two launches
        again = run_rows("tt2_regulate_bwd", dy, ends, L["tx"], L["tx"], n_out, dtype, mem)
        assert np.array_equal(R.bits(again), R.bits(got))


def test_backward_clamps_whatever_ends_holds():
    rng = np.random.default_rng(4)
    B, tx, n_out, dim = 2, 6, 50, 3
    dy = rng.normal(size=(B, n_out, dim)).astype(np.float32)
    ends = np.array([[-5, 10, 7, R.INT32_MAX, 20, R.INT32_MIN], [0, 0, 50, 51, 49, 50]], dtype=np.int32)
    want = R.bwd_model(dy, ends, n_out)
    got = run_rows("tt2_regulate_bwd", dy, ends, tx, tx, n_out, "f32", "odd")
    assert R.reject({"dh": got}, {"dh": want}) == []


def test_backward_of_one_hot_rows_is_the_transposed_forward():
    """E[n, t] = 1 where frame n belongs to phoneme t: the forward of the identity is E, the backward of
    the identity is its transpose."""
    d = np.array([[2, 0, 3, 1, 0, 0, 4], [0, 0, 9, 9, 9, 9, 9], [1, 1, 1, 1, 1, 1, 1]])
    tx, n_out = 7, 12
    p = R.plan_ref(d, [7, 7, 5], tx, n_out)
    B = len(d)
    eye_t = np.broadcast_to(np.eye(tx, dtype=np.float32), (B, tx, tx)).copy()
    eye_n = np.broadcast_to(np.eye(n_out, dtype=np.float32), (B, n_out, n_out)).copy()
    for mem in ("odd", "sliced"):
        y = run_rows("tt2_regulate_fwd", eye_t, p["index"], n_out, tx, n_out, "f32", mem)            # [B, n_out, tx]
        dh = run_rows("tt2_regulate_bwd", eye_n, p["ends"], tx, tx, n_out, "f32", mem)               # [B, tx, n_out]
        assert np.array_equal(R.bits(dh), R.bits(np.ascontiguousarray(y.transpose(0, 2, 1))))
        assert y.sum() == p["frames"].sum()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_zero_sizes(dtype):
    """fwd with tx = 0 zero-fills (src and map may be null); bwd with n_out = 0 writes +0 to every row;
    the sizes that need no launch leave everything untouched."""
    np_dt = NP[dtype]
    idx = np.zeros((2, 9), dtype=np.int32)
    for mem in ("odd", "sliced"):
        for null in (False, True):
            y = run_rows("tt2_regulate_fwd", np.zeros((2, 0, 8), np_dt), idx, 9, 0, 9, dtype, mem, src_null=null, map_null=null)
            assert y.shape == (2, 9, 8) and not R.bits(y).any()
            dh = run_rows("tt2_regulate_bwd", np.zeros((2, 0, 8), np_dt), np.zeros((2, 5), np.int32), 5, 5, 0, dtype, mem,
                          src_null=null, map_null=null)
            assert dh.shape == (2, 5, 8) and not R.bits(dh).any()
    y = run_rows("tt2_regulate_fwd", np.zeros((2, 4, 8), np_dt), idx, 9, 4, 9, dtype, "odd", override=dict(batch=0))
    assert (R.bits(y) == R.bits(np.array([poison(np_dt)]))[0]).all()
    dh = run_rows("tt2_regulate_bwd", np.zeros((2, 9, 8), np_dt), np.zeros((2, 4), np.int32), 4, 4, 9, dtype, "odd", override=dict(dim=0))
    assert (R.bits(dh) == R.bits(np.array([poison(np_dt)]))[0]).all()


def test_refusals_leave_the_outputs_untouched():
    L = layout("long")
    E = _lib.E_INVALID
    h = R.fwd_problem(L, 8, "f32")
    dy = R.bwd_exact_problem(L, 8, "f32")
    bad = (dict(dtype=_lib.DT_F16), dict(tx=4097), dict(src_ld=7), dict(dst_ld=7), dict(dim=-1), dict(batch=-2), dict(dst=None),
           dict(src=None), dict(map=None))
    for kw in bad + (dict(map_ld=L["n_out"] - 1),):
        assert run_rows("tt2_regulate_fwd", h, L["plan"]["index"], L["n_out"], L["tx"], L["n_out"], "f32", "sliced",
                        expect=E, override=kw) is None
    for kw in bad + (dict(map_ld=L["tx"] - 1),):
        assert run_rows("tt2_regulate_bwd", dy, L["plan"]["ends"], L["tx"], L["tx"], L["n_out"], "f32", "sliced",
                        expect=E, override=kw) is None
