"""Gaussian-upsampling kernels (tt2_gauss_upsample_fwd / _bwd) against the references of
tests/_upsample_refs.py (GPU), by direct C-ABI calls on hand-built buffers.

Exact problems (selector, uniform) are compared bit for bit on every output that is order-independent
in float32 (_upsample_refs.exact_outputs; tests/test_upsample_refs.py asserts the premises).  Random
problems (ESPnet-like, wide / sharp mix) are judged per frame row (y, lse) and per phoneme (dh row,
dcenter, dprec, dbias) against float64: the error over max(4 x the yardstick's own error on that row,
2 ulp of the row's scale) must not exceed 1, the yardstick being the numpy float32 evaluation for the
f32 kernels (and for lse, which is f32 arithmetic in both) and the bf16-rounding twin for the bf16
kernels; a yardstick's error on a row counts as no less than its RMS error relative to scale over
the utterance's rows (tests/test_upsample_refs.py shows that this bar rejects twelve mutants, also when
confined to one tile).  One allowance goes beyond that bar, derived in _upsample_refs and measured there
on the float32 reference: the absolute flush-to-zero term, 2^-126 times what a row's weights multiply.

Buffers: every tensor is a strided region of a flat buffer between guard bands, the whole buffer
poisoned with NaN first.  In the "odd" layout the leading dimensions are odd and the bases sit off
16-byte alignment (the element-by-element path); in the "sliced" layout the tensors are column slices
of wider, 16-byte aligned buffers (the 16-byte chunk path where dim allows).  B = 4 with a different
length case per utterance (full, interior, 0, above the bound) for q_len and key_len.  Everything the
contract does not read is NaN: rows of h and entries of center / prec / bias at and past Tx_b, rows of
dy, y and lse at and past Ty_b (the backward gets the forward's y and lse with those rows poisoned).
After a call every input buffer is unchanged, every byte of an output buffer outside the tensor is
unchanged, and outputs that were not asked for are untouched."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _upsample_refs as R  # noqa: E402
from tt2 import _lib  # noqa: E402

GUARD = 64
NP = {"f32": np.float32, "bf16": np.uint16}
DT = {"f32": _lib.DT_F32, "bf16": _lib.DT_BF16}
GRADS = ("dh", "dcenter", "dprec", "dbias")
NAN16 = np.uint16(0x7FC1)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


class Buf:
    """A strided tensor inside a flat NaN-poisoned buffer with guard bands, uploaded as raw integers."""

    def __init__(self, shape, dtype, strides, shift=0, data=None, fill=None):
        self.shape, self.dtype, self.strides, self.off = tuple(shape), np.dtype(dtype), tuple(strides), GUARD + shift
        n = 0 if 0 in self.shape else 1 + sum((s - 1) * st for s, st in zip(self.shape, self.strides))
        poison = {np.float32: np.float32(np.nan), np.uint16: NAN16, np.int32: np.int32(-77)}[self.dtype.type]
        self.before = np.full(self.off + n + GUARD, poison if fill is None else fill, dtype=self.dtype)
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
        return np.array_equal(bits(self.fetch()), bits(self.before))

    def result(self):
        """The tensor after the call; asserts that nothing outside it was written."""
        after = self.fetch().copy()
        out = self.region(after).copy()
        self.region(after)[...] = self.region(self.before)
        assert np.array_equal(bits(after), bits(self.before)), "written outside the tensor (pad columns or guard bands)"
        return out


def odd(n, pad):
    return n + pad + ((n + pad + 1) % 2)


def strides3(rows, dim, mem, pad):
    """Row and batch strides (elements) and the base shift of a [B, rows, dim] tensor."""
    if mem == "sliced":                        # columns 8 .. 8 + dim of rows of a wider, aligned buffer
        ld = (dim + 7) // 8 * 8 + 8 * pad
        return ld, rows * ld + 16, 8
    ld = odd(dim, pad)
    return ld, rows * ld + 3, None


def encode(x, dtype):
    """float64 values of `dtype` -> what the buffer holds."""
    return np.asarray(x, dtype=np.float32) if dtype == "f32" else R.bf16_bits(x)


def decode(x, dtype):
    return x.astype(np.float64) if dtype == "f32" else R.bf16_from_bits(x)


def mat(x, dtype, mem, pad, shift_odd, live=None):
    """Buf of a [B, rows, dim] float64 array; rows at and past live[b] are NaN."""
    B, rows, dim = x.shape
    ld, bs, shift = strides3(rows, dim, mem, pad)
    data = encode(x, dtype).copy()
    if live is not None:
        for b, n in enumerate(live):
            data[b, n:] = np.float32(np.nan) if dtype == "f32" else NAN16
    unit = 1 if dtype == "f32" else 2
    return Buf(x.shape, NP[dtype], (bs, ld, 1), shift=shift_odd * unit if shift is None else shift, data=data)


def vec(x, p_ld, live=None, shift=1):
    """Buf of a [B, cols] float64 array as f32; entries at and past live[b] are NaN."""
    data = np.asarray(x, dtype=np.float32).copy()
    if live is not None:
        for b, n in enumerate(live):
            data[b, n:] = np.nan
    return Buf(data.shape, np.float32, (p_ld, 1), shift=shift, data=data)


def call(name, a, expect=0):
    L = _lib.lib()
    rc = getattr(L, name)(ctypes.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (name, rc, L.tt2_last_error())
    if expect:
        assert L.tt2_last_error().startswith(name.encode() + b":")


def run(p, mem, want=GRADS, fwd_expect=0, bwd_expect=0, fwd_override=None, bwd_override=None):
    """tt2_gauss_upsample_fwd, then _bwd on what it left -> dict of float64 arrays (the outputs asked
    for; nothing of a refused call)."""
    dtype = p["dtype"]
    B, tx, dim = p["h"].shape
    n_out = p["dy"].shape[1]
    txs, tys = R.lengths(p)
    p_ld = odd(tx, 2) if mem == "odd" else (tx + 3) // 4 * 4 + 4
    hb = mat(p["h"], dtype, mem, 1, 1, live=txs)
    cb, pb = vec(p["center"], p_ld, txs), vec(p["prec"], p_ld, txs, shift=2)
    bb = vec(p["bias"], p_ld, txs, shift=3) if p["bias"] is not None else None
    ql = Buf((B,), np.int32, (1,), data=p["q_len"]) if p["q_len"] is not None else None
    kl = Buf((B,), np.int32, (1,), data=p["key_len"], shift=1) if p["key_len"] is not None else None
    yb = mat(np.zeros((B, n_out, dim)), dtype, mem, 2, 3, live=[0] * B)
    lse_ld = odd(n_out, 4)
    lb = Buf((B, n_out), np.float32, (lse_ld, 1), shift=1)
    inputs = [hb, cb, pb] + [x for x in (bb, ql, kl) if x is not None]

    a = _lib.GaussUpsampleArgs()
    a.h, a.center, a.prec, a.bias = hb.ptr, cb.ptr, pb.ptr, (bb.ptr if bb else None)
    a.q_len, a.key_len = (ql.ptr if ql else None), (kl.ptr if kl else None)
    a.y, a.lse = yb.ptr, lb.ptr
    a.h_ld, a.h_bs, a.y_ld, a.y_bs = hb.strides[1], hb.strides[0], yb.strides[1], yb.strides[0]
    a.p_ld, a.lse_ld = p_ld, lse_ld
    a.batch, a.tx, a.n_out, a.dim, a.dtype, a.offset = B, tx, n_out, dim, DT[dtype], p["offset"]
    if mem == "sliced":
        assert hb.ptr % 16 == 0 and yb.ptr % 16 == 0
    else:
        assert hb.ptr % 16 != 0 and yb.ptr % 16 != 0
    f = type(a).from_buffer_copy(a)
    for k, v in (fwd_override or {}).items():
        setattr(f, k, v)
    call("tt2_gauss_upsample_fwd", f, fwd_expect)
    assert all(x.unchanged() for x in inputs), "an input was written"
    if fwd_expect:
        assert yb.unchanged() and lb.unchanged(), "a refused call wrote"
        return {}
    y_raw, lse_raw = yb.result(), lb.result()
    out = {"y": decode(y_raw, dtype), "lse": lse_raw.astype(np.float64)}
    if want is None:
        return out

    # the backward reads the forward's y and lse; their rows at and past Ty_b are poisoned first
    y_in = mat(decode(y_raw, dtype), dtype, mem, 2, 3, live=tys)
    l_in = vec(lse_raw, lse_ld, tys)
    dyb = mat(p["dy"], dtype, mem, 3, 1, live=tys)
    dhb = mat(np.zeros((B, tx, dim)), dtype, mem, 1, 3, live=[0] * B)
    gv = {k: Buf((B, tx), np.float32, (p_ld, 1), shift=i) for i, k in enumerate(("dcenter", "dprec", "dbias"))}
    L = _lib.lib()
    need = L.tt2_gauss_upsample_bwd_workspace_size(B, tx, n_out, dim)
    ws = torch.full((need + 16,), 0x7F, dtype=torch.uint8, device="cuda")
    a.y, a.lse, a.dy = y_in.ptr, l_in.ptr, dyb.ptr
    a.y_ld, a.y_bs, a.dy_ld, a.dy_bs = y_in.strides[1], y_in.strides[0], dyb.strides[1], dyb.strides[0]
    a.dh = dhb.ptr if "dh" in want else None
    a.dh_ld, a.dh_bs = dhb.strides[1], dhb.strides[0]
    a.dcenter, a.dprec, a.dbias = (gv[k].ptr if k in want else None for k in ("dcenter", "dprec", "dbias"))
    a.workspace, a.workspace_bytes = (ws.data_ptr() + 15) // 16 * 16, need
    for k, v in (bwd_override or {}).items():
        setattr(a, k, v)
    call("tt2_gauss_upsample_bwd", a, bwd_expect)
    assert all(x.unchanged() for x in inputs + [y_in, l_in, dyb]), "an input was written"
    for k, buf in [("dh", dhb)] + list(gv.items()):
        if bwd_expect or k not in want:
            assert buf.unchanged(), f"{k} was not asked for (or the call was refused) and was written"
        else:
            out[k] = decode(buf.result(), dtype) if k == "dh" else buf.result().astype(np.float64)
    return out


MAKERS = {"selector": R.selector_problem, "uniform": R.uniform_problem, "espnet": R.espnet_problem, "mix": R.mix_problem}


@functools.lru_cache(maxsize=None)
def problem(kind, shape, dtype):
    """(problem, float64 reference, yardstick, scales), computed once and shared; never modified."""
    p = MAKERS[kind](*shape, dtype)
    return p, R.evaluate(p), R.yardstick(p), (R.scales(p), R.tiny(p))


def check_bar(p, out, ref, yard, sc, what):
    detail = {}
    ratios, pads = R.judge(p, out, ref=ref, yard=yard, sc=sc, detail=detail)
    print(what, " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    plain, _ = R.judge(p, out, ref=ref, yard=yard, sc=sc, pool=False)      # the row-by-row bar, for the record
    print("   row-by-row:", what, " ".join(f"{k} {v:.3f}" for k, v in plain.items()))
    for k, v in ratios.items():
        if not v <= 1.0:
            print("   worst row of", k, "(utterance, row, error, allowed, scale):", detail[k])
    assert not pads, (what, pads)
    assert all(r <= 1.0 for r in ratios.values()), (what, ratios)


CASES = [(shape, dtype, mem) for shape in R.SHAPES + R.EDGE_SHAPES for dtype in ("f32", "bf16") for mem in ("odd", "sliced")]


@pytest.mark.parametrize("kind", ["selector", "uniform"])
@pytest.mark.parametrize("shape,dtype,mem", CASES)
def test_exact_problems_bit_for_bit(shape, dtype, mem, kind):
    p, ref, yard, sc = problem(kind, shape, dtype)
    out = run(p, mem)
    want = R.exact_expected(p)
    exact = R.exact_outputs(p)
    for k in exact:
        assert np.array_equal(bits(encode(out[k], dtype if k in ("y", "dh") else "f32")),
                              bits(encode(want[k], dtype if k in ("y", "dh") else "f32"))), (k, "not the expected bits")
    check_bar(p, out, ref, yard, sc, f"{kind} {shape} {dtype} {mem}")


@pytest.mark.parametrize("kind", ["espnet", "mix"])
@pytest.mark.parametrize("shape,dtype,mem", CASES)
def test_random_problems_per_row_against_float64(shape, dtype, mem, kind):
    p, ref, yard, sc = problem(kind, shape, dtype)
    out = run(p, mem)
    check_bar(p, out, ref, yard, sc, f"{kind} {shape} {dtype} {mem}")
    if shape == (65, 33, 80):                               # repeatability over two launches
        again = run(p, mem)
        for k in R.OUTPUTS:
            assert np.array_equal(bits(np.float32(out[k])), bits(np.float32(again[k]))), k


def _take(p, rows):
    q = dict(p)
    for k in ("h", "dy", "center", "prec", "bias"):
        q[k] = None if p[k] is None else p[k][rows]
    q["q_len"], q["key_len"] = [p["q_len"][b] for b in rows], [p["key_len"][b] for b in rows]
    return q


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batch_position_independence(dtype):
    p = problem("mix", (65, 33, 80), dtype)[0]
    base = run(p, "sliced")
    rows = [2, 0, 3, 1]
    moved = run(_take(p, rows), "sliced")
    for k in R.OUTPUTS:
        assert np.array_equal(bits(np.float32(moved[k])), bits(np.float32(base[k][rows]))), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_nan_stays_inside_its_utterance(dtype):
    p = problem("mix", (65, 33, 80), dtype)[0]
    base = run(p, "odd")
    q = dict(p)
    q["h"], q["center"] = p["h"].copy(), p["center"].copy()
    q["h"][0, 1, 3] = np.nan                                 # utterance 0 is live, and so is utterance 1
    q["center"][0, 0] = np.nan
    got = run(q, "odd")
    for k in R.OUTPUTS:
        assert np.array_equal(bits(np.float32(got[k][1:])), bits(np.float32(base[k][1:]))), k
    assert np.isnan(got["y"][0]).any() and base["y"][1].any()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_each_subset_of_gradients_gives_the_bits_of_the_full_call(dtype):
    p = problem("mix", (65, 33, 80), dtype)[0]
    full = run(p, "sliced")
    for mask in range(1, 15):
        asked = tuple(k for i, k in enumerate(GRADS) if mask >> i & 1)
        got = run(p, "sliced", want=asked)
        assert sorted(got) == sorted(("y", "lse") + asked)
        for k in asked:
            assert np.array_equal(bits(np.float32(got[k])), bits(np.float32(full[k]))), (asked, k)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_zero_sizes(dtype):
    """fwd with tx = 0 writes +0 to y and lse; bwd with n_out = 0 writes +0 to every gradient; batch = 0
    touches nothing."""
    rng = np.random.default_rng(0)
    for mem in ("odd", "sliced"):
        p = {"h": np.zeros((4, 0, 8)), "dy": np.ones((4, 9, 8)), "center": np.zeros((4, 0)), "prec": np.zeros((4, 0)),
             "bias": None, "offset": 0.0, "q_len": R.length_cases(9), "key_len": None, "dtype": dtype}
        out = run(p, mem, want=None)
        assert out["y"].shape == (4, 9, 8) and not out["y"].any() and not np.signbit(out["y"]).any() and not out["lse"].any()
        p = {"h": rng.integers(-2, 3, size=(4, 5, 8)).astype(np.float64), "dy": np.zeros((4, 0, 8)), "center": np.ones((4, 5)),
             "prec": np.ones((4, 5)), "bias": np.ones((4, 5)), "offset": 1.0, "q_len": None, "key_len": R.length_cases(5, keys=True),
             "dtype": dtype}
        out = run(p, mem)
        for k in GRADS:
            assert out[k].shape[:2] == (4, 5) and not out[k].any() and not np.signbit(out[k]).any(), k
    p = problem("mix", (33, 5, 17), dtype)[0]
    got = run(p, "odd", fwd_override=dict(batch=0), want=None)
    assert np.isnan(got["y"]).all() and np.isnan(got["lse"]).all()          # still the poison


def test_refusals_leave_the_outputs_untouched():
    p = problem("mix", (33, 5, 17), "f32")[0]
    E = _lib.E_INVALID
    bad = (dict(dtype=_lib.DT_F16), dict(tx=4097), dict(dim=513), dict(h_ld=16), dict(y_ld=16), dict(p_ld=4), dict(lse_ld=32),
           dict(dim=-1), dict(batch=-2), dict(offset=-1.0), dict(offset=float("nan")), dict(offset=float("inf")),
           dict(center=None), dict(prec=None), dict(h=None))
    for kw in bad + (dict(y=None), dict(lse=None)):
        assert run(p, "sliced", fwd_expect=E, fwd_override=kw) == {}
    for kw in bad + (dict(dy_ld=16), dict(dh_ld=16), dict(dy=None), dict(y=None), dict(lse=None), dict(workspace=None),
                     dict(workspace_bytes=8), dict(dh=None, dcenter=None, dprec=None, dbias=None)):
        got = run(p, "sliced", bwd_expect=E, bwd_override=kw)
        assert sorted(got) == ["lse", "y"]
    ws_off = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    assert sorted(run(p, "sliced", bwd_expect=E, bwd_override=dict(workspace=ws_off.data_ptr() // 16 * 16 + 4))) == ["lse", "y"]
