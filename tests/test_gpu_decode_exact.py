"""The decode-step kernels held to exact and per-vector float64 bars (GPU): tt2_attn_decode,
tt2_kv_append, tt2_decode_emit (csrc/decode.hip) and the decode epilogues of the skinny GEMM
(csrc/gemm_skinny.hip: frame emit with its stop tracking, KV scatter, positional encoding, the
LayerNorm prologue).

The problems and judges are those of tests/_decode_refs.py (validated on the CPU by
tests/test_decode_refs.py, whose mutants prove that they reject a dropped, leaked or doubled key, a
missing merge factor, swapped heads, a neighbour's key_len, a rounded projection input and four
wrong stop rules):
  selector  exact arithmetic: o and the slabs bit-equal to the float64 reference, the selected key
            walking every seam of the 8-wave x 32-key x 2-buffer key walk
  uniform   q = 0: o = the mean of the visible V rows, bit-equal at a power-of-two count, else
            within 1 ulp (16-bit) / 4 f32 ulp (f32, slabs)
  random    every (batch, head) vector within 2x the twin's error (16-bit out), within
            max(4x the float32 CPU evaluations' error, 2 f32 ulp) for f32 and the slabs
at nk = 0 .. 520 (R.NK: every count at which the key walk takes another path), in bf16, f16 and
f32, with the decoder's strides: self (t_ptr, packed qkv, K | V halves of one cache), cross (ragged
key_len, K / V at a column offset of a buffer shared by the layers) and both counters with a tk
below them.  Every output is NaN-filled first, with guard rows, and guard columns wherever the
contract gives the output a row stride (the slabs, mel_seq, stop_seq, prev and ln_out are packed),
that must still be NaN afterwards; the rejections must leave the NaN untouched.  Each test prints its worst ratios
(pytest -s; <= 1 passes)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import _decode_refs as R  # noqa: E402
import _norm_refs as N  # noqa: E402
from _attn_refs import representable  # noqa: E402
from _decode_refs import BF16, D, F16, F32, F64  # noqa: E402
from test_gpu_attention_exact import Guarded  # noqa: E402
from test_gpu_norm_exact import Guarded as RowGuarded  # noqa: E402
from tt2 import _lib, ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")
T = R.T_MAX
B = R.BATCH
LAYERS, LAYER = 3, 1            # the cross form: K | V of layer 1 inside a [B, T, 3 * 2 HD] buffer
TAG = {BF16: "bf16", F16: "f16", F32: "f32"}
BITS = {BF16: torch.int16, F16: torch.int16, F32: torch.int32}


def dev(t, dtype):
    return t.to(dtype).to(DEV)


def i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


def pad_cols(t, dtype, pad=8):
    """t [R, Cn] on the device inside a [R, Cn + pad] buffer (ld = Cn + pad, junk in the padding)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), 3.0, dtype=dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(dtype).to(DEV)
    return buf


# ------------------------------------------------------------------ one tt2_attn_decode launch
class Launch:
    """p (a R.DecProblem) in the layout of `form`, every output guarded.  fuse: 'out' (plain),
    'wo' (slabs, no out), 'wo+out'.  stop: None, 'step' or 't_ptr' (which counter stop_len reads)."""

    def __init__(self, p, dtype, form, fuse="out", stop=None, ln=None):
        self.p, self.dtype = p, dtype
        Bn, H, Tn = p.shape
        HD = H * D
        g = torch.Generator().manual_seed(17)
        junk = lambda *sh: torch.randint(-3, 4, sh, generator=g).to(F64)          # noqa: E731
        kw = {}
        # the query (or the projection input)
        if p.wq is not None:
            self.q, q_ld = dev(ln.x if ln is not None else p.x, dtype), R.DM
            self.wq, self.bq = pad_cols(p.wq, dtype), dev(p.bq, F32)
            kw.update(wq=self.wq, wq_ld=R.DM + 8, bq=self.bq)
        elif form == "self":
            self.q, q_ld = dev(torch.cat([p.q.reshape(Bn, HD), junk(Bn, 2 * HD)], 1), dtype), 3 * HD
        else:
            self.q, q_ld = dev(p.q.reshape(Bn, HD), dtype), HD
        # keys and values
        kf, vf = p.k.reshape(Bn, Tn, HD), p.v.reshape(Bn, Tn, HD)
        if form == "self":
            self.kv = dev(torch.cat([kf, vf], 2), dtype)
            k, v, ld = self.kv, self.kv[:, :, HD:], 2 * HD
        else:
            wide = junk(Bn, Tn, LAYERS * 2 * HD)
            wide[:, :, LAYER * 2 * HD:LAYER * 2 * HD + HD], wide[:, :, LAYER * 2 * HD + HD:(LAYER + 1) * 2 * HD] = kf, vf
            self.kv = dev(wide, dtype)
            k, v, ld = self.kv[:, :, LAYER * 2 * HD:], self.kv[:, :, LAYER * 2 * HD + HD:], LAYERS * 2 * HD
        # the counters: min(tk, *t_ptr + 1, key_len[b]) must come to p.nk[b]
        top = max(p.nk)
        if form == "self":
            assert len(set(p.nk)) == 1
            tk, self.t_ptr, self.key_len = Tn, i32([top - 1]), None
        elif form == "cross":
            tk, self.t_ptr, self.key_len = Tn, None, i32(p.nk)
        elif top % 2 == 0:      # tk binds for the longest element, key_len for the others
            tk, self.t_ptr = top, i32([top + 1])
            self.key_len = i32([n if n < top else top + 5 for n in p.nk])
        else:                   # t_ptr binds for the longest element
            tk, self.t_ptr = min(Tn, top + 3), i32([top - 1])
            self.key_len = i32([n if n < top else top + 5 for n in p.nk])
        assert tk <= Tn and [min(tk, top + 9 if self.t_ptr is None else int(self.t_ptr) + 1,
                                 tk if self.key_len is None else int(self.key_len[b])) for b in range(Bn)] == list(p.nk)
        kw.update(t_ptr=self.t_ptr, key_len=self.key_len)
        if stop is not None:
            assert self.t_ptr is not None
            self.stop_len = i32([-5 if s else R.INT32_MAX for s in p.stopped])
            self.step = i32([0]) if stop == "step" else None
            kw.update(stop_len=self.stop_len, step=self.step)
        # outputs
        self.out = Guarded(Bn, HD, dtype) if "out" in fuse else None
        self.slab = None
        if "wo" in fuse:
            # the slab rows are packed ([H, B, HD], no row stride in the contract): guard rows only
            self.slab = RowGuarded((H * Bn, HD), F32)
            self.wo = pad_cols(p.wo, dtype)
            kw.update(wo=self.wo, wo_ld=HD + 8, slab=self.slab.v)
        self.ln_out = None
        if ln is not None:
            self.ln_out = RowGuarded((Bn, R.DM), dtype)
            self.ln_in = (dev(ln.parts.reshape(8 * Bn, R.DM), F32), dev(ln.bias, F32), dev(ln.gamma, F32), dev(ln.beta, F32))
            kw.update(ln=self.ln_in + (self.ln_out.v, ln.EPS))
        self.args = (self.q, k, v, None if self.out is None else self.out.body, q_ld, Tn * ld, ld, Tn * ld, ld,
                     0 if self.out is None else self.out.ld, Bn, H, tk)
        self.kw = dict(scale=p.scale, **kw)

    def run(self):
        Bn, H, _ = self.p.shape
        ops.attn_decode(*self.args, **self.kw)
        torch.cuda.synchronize()
        res = {"o": None, "slab": None}
        if self.out is not None:
            self.out.check("out")
            res["o"] = self.out.body.cpu().to(F64).reshape(Bn, H, D)
        if self.slab is not None:
            self.slab.check("slab")
            res["slab"] = self.slab.cpu().to(F64).reshape(H, Bn, H * D)
        if self.ln_out is not None:
            self.ln_out.check("ln_out")
        return res


def finish(what, fails, figs):
    print(f"\n{what}: {R.show(figs)}")
    assert not fails, (what, fails)


SUBFORMS = (("out", 8, False), ("wo", 8, False), ("wo+out", 4, False), ("wo", 8, True))     # (fuse, H, wq)


def _sub(fuse, H, wq):
    return f"{fuse}-H{H}{'-wq' if wq else ''}"


@pytest.mark.parametrize("case", R.cases(R.SELECTOR_ROT), ids=lambda c: c[0])
def test_attn_selector_exact(case):
    """o and every slab entry bit-equal to the float64 reference: plain out, the fused output
    projection (H = 8 without out, H = 4 with it), and the fused query + output projections.
    Measured on an MI355X: equal on all 16 cases x 4 forms."""
    cid, i, nk, form, dtype = case
    for j, (fuse, H, wq) in enumerate(SUBFORMS):
        p = R.selector_problem(H, nk, rot=i + 7 * j, wo="wo" in fuse, wq=wq)       # each form starts at another seam
        ref = R.assert_exact_selector(p, dtype)
        finish(f"selector {cid} {_sub(fuse, H, wq)}", *R.judge_selector(Launch(p, dtype, form, fuse).run(), ref, dtype))


@pytest.mark.parametrize("case", R.cases(R.UNIFORM_ROT), ids=lambda c: c[0])
def test_attn_uniform(case):
    """o = the mean of the visible V rows: equal to RN(mean) at a power-of-two count, within 1 ulp
    of it elsewhere (f32: 4 f32 ulp); slabs equal at a power-of-two count, within 4 f32 ulp.
    Measured on an MI355X, worst over the cases: o 0 ulp from RN(mean) in bf16 and f16, 0.50 ulp in
    f32; slabs 2.16 f32 ulp (2.15 on the CPU model of a lane-parallel sum in test_decode_refs.py)."""
    cid, i, nk, form, dtype = case
    for fuse, H, _ in SUBFORMS[:3]:
        p = R.uniform_problem(H, nk, wo="wo" in fuse)
        R.assert_exact_uniform(p)
        finish(f"uniform {cid} {_sub(fuse, H, False)}", *R.judge_uniform(Launch(p, dtype, form, fuse).run(), p, dtype))


@pytest.mark.parametrize("case", R.cases(R.RANDOM_ROT), ids=lambda c: c[0])
def test_attn_random_vectors(case):
    """Every (batch, head) vector of o and every (head, batch) row of the slabs on its own.
    Measured on an MI355X, worst vector over the cases and forms (<= 1 passes): o 0.50 in bf16 and
    f16 (the kernel's error is the one rounding of the twin), 0.28 in f32; slabs 0.29 (bf16), 0.24
    (f16), 0.27 (f32)."""
    cid, i, nk, form, dtype = case
    for fuse, H, wq in (("wo+out", 8, False), ("wo+out", 4, False), ("wo+out", 8, True)):
        p = R.random_problem(H, nk, dtype, wo=True, wq=wq, seed=i)
        ref, y32 = R.evaluate(p), R.float32_evaluations(p)
        out = Launch(p, dtype, form, fuse).run()
        finish(f"random {cid} {_sub(fuse, H, wq)}", *R.judge_random(out, ref, R.twin(p, dtype), y32, dtype))


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=TAG.get)
@pytest.mark.parametrize("stop", ["step", "t_ptr"])
def test_attn_stop_len(stop, dtype):
    """A finished utterance (*step >= stop_len[b], step defaulting to t_ptr) gets exact zeros in out
    and in every slab row; the others are the selector problem's exact answer."""
    for nk, form in (([257] * B, "self"), ([520, 9, 65], "both")):
        p = R.selector_problem(8, nk, rot=11, wo=True, stopped=[False, True, False])
        ref = R.assert_exact_selector(p, dtype)
        assert ref["o"][1].abs().max() == 0 and ref["slab"][:, 1].abs().max() == 0 and ref["o"][0].abs().max() > 0
        finish(f"stop_len via {stop} {form} {TAG[dtype]}",
               *R.judge_selector(Launch(p, dtype, form, "wo+out", stop=stop).run(), ref, dtype))


@pytest.mark.parametrize("dtype", [BF16, F16], ids=TAG.get)
def test_attn_ln_prologue_selector(dtype):
    """The selector problem through the fused residual combine + LayerNorm: ln_out bit-equal to the
    float64 LayerNorm (exact by construction) and the slabs of the attention behind it bit-equal
    to the float64 reference; a finished row still gets its ln_out."""
    for nk, stopped in (([513, 64, 0], None), ([257, 8, 520], [False, False, True])):
        ln, p = R.ln_selector_problem(nk, rot=7)
        p.stopped = stopped
        ref = R.assert_exact_selector(p, dtype)
        assert representable(ln.x, dtype)
        run = Launch(p, dtype, "both" if stopped else "cross", "wo", stop="step" if stopped else None, ln=ln)
        out = run.run()
        got = run.ln_out.cpu()
        assert torch.equal(got.to(F64), ln.y), "ln_out differs from the float64 LayerNorm"
        finish(f"ln prologue selector {nk} {TAG[dtype]}", *R.judge_selector(out, ref, dtype))


# ------------------------------------------------------------------ rejections
def _raw_args(dtype=BF16, H=8):
    """A valid tt2_attn_decode_args over small buffers, and everything it points to."""
    HD = H * D
    keep = {"q": torch.zeros(B, 3 * HD, dtype=dtype, device=DEV), "kv": torch.zeros(B, 16, 2 * HD, dtype=dtype, device=DEV),
            "out": torch.full((B, HD), NAN, dtype=dtype, device=DEV), "slab": torch.full((H, B, HD), NAN, device=DEV),
            "w": torch.zeros(512, 512, dtype=dtype, device=DEV), "f": torch.zeros(8 * B * 512, device=DEV),
            "ln_out": torch.full((B, 512), NAN, dtype=dtype, device=DEV), "t": i32([3])}
    a = _lib.AttnDecodeArgs()
    a.q, a.k, a.v = keep["q"].data_ptr(), keep["kv"].data_ptr(), keep["kv"][:, :, HD:].data_ptr()
    a.out = keep["out"].data_ptr()
    a.q_ld, a.k_bstride, a.k_ld, a.v_bstride, a.v_ld, a.o_ld = 3 * HD, 16 * 2 * HD, 2 * HD, 16 * 2 * HD, 2 * HD, HD
    a.t_ptr = keep["t"].data_ptr()
    a.batch, a.heads, a.head_dim, a.tk, a.dtype, a.scale = B, H, 64, 16, _lib.dt(keep["q"]), 0.125
    return a, keep


def _with_wq(a, keep):
    a.wq, a.wq_ld, a.bq, a.q_ld = keep["w"].data_ptr(), 512, keep["f"].data_ptr(), 512


def _with_wo(a, keep):
    a.wo, a.wo_ld, a.slab = keep["w"].data_ptr(), 512, keep["slab"].data_ptr()


def _with_ln(a, keep):
    _with_wq(a, keep)
    _with_wo(a, keep)
    f = keep["f"].data_ptr()
    a.ln_part, a.ln_bias, a.ln_gamma, a.ln_beta, a.ln_out, a.ln_eps = f, f, f, f, keep["ln_out"].data_ptr(), 1e-5


REJECTIONS = {
    "head_dim 32": lambda a, k: setattr(a, "head_dim", 32),
    "q_ld not 16 B": lambda a, k: setattr(a, "q_ld", a.q_ld + 4),
    "k_ld not 16 B": lambda a, k: setattr(a, "k_ld", a.k_ld + 4),
    "v_bstride not 16 B": lambda a, k: setattr(a, "v_bstride", a.v_bstride + 4),
    "wq with 4 heads": lambda a, k: (_with_wq(a, k), setattr(a, "heads", 4)),
    "wq_ld not 16 B": lambda a, k: (_with_wq(a, k), setattr(a, "wq_ld", 516)),
    "wo without slab": lambda a, k: (_with_wo(a, k), setattr(a, "slab", None)),
    "wo_ld not 16 B": lambda a, k: (_with_wo(a, k), setattr(a, "wo_ld", 516)),
    "wo with 9 heads": lambda a, k: (_with_wo(a, k), setattr(a, "heads", 9)),
    "stop_len without a counter": lambda a, k: (setattr(a, "stop_len", k["t"].data_ptr()), setattr(a, "t_ptr", None)),
    "ln with f32": None,                                       # built on an f32 baseline below
    "ln with 4 heads": lambda a, k: (_with_ln(a, k), setattr(a, "heads", 4)),
    "ln with q_ld 1536": lambda a, k: (_with_ln(a, k), setattr(a, "q_ld", 1536)),
    "null out without wo": lambda a, k: setattr(a, "out", None),
    "null q": lambda a, k: setattr(a, "q", None),
    "null k": lambda a, k: setattr(a, "k", None),
    "null v": lambda a, k: setattr(a, "v", None),
    "batch 0": lambda a, k: setattr(a, "batch", 0),
    "heads 0": lambda a, k: setattr(a, "heads", 0),
    "tk -1": lambda a, k: setattr(a, "tk", -1),
}


@pytest.mark.parametrize("what", list(REJECTIONS), ids=lambda s: s.replace(" ", "_"))
def test_attn_decode_rejections(what):
    """TT2_E_INVALID before any launch: out, the slabs and ln_out keep their NaN."""
    a, keep = _raw_args(F32 if what == "ln with f32" else BF16)
    if what == "ln with f32":
        _with_ln(a, keep)
    else:
        REJECTIONS[what](a, keep)
    rc = _lib.lib().tt2_attn_decode(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.E_INVALID, (what, rc)
    for n in ("out", "slab", "ln_out"):
        assert torch.isnan(keep[n]).all(), f"{what}: {n} written"


def test_attn_decode_baseline_is_accepted():
    """The baseline the rejections vary is itself a valid call (so each of them fails for its own reason)."""
    for fuse in (None, _with_wo, _with_ln):
        a, keep = _raw_args()
        if fuse:
            fuse(a, keep)
        assert _lib.lib().tt2_attn_decode(C.byref(a), _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert not torch.isnan(keep["out"]).any()


# ------------------------------------------------------------------ tt2_kv_append
class Cache:
    """A NaN-filled [B, t_max, c_ld] cache between NaN guard bands of one batch stride each."""

    def __init__(self, Bn, t_max, c_ld, dtype):
        self.shape, self.g = (Bn, t_max, c_ld), t_max * c_ld
        self.buf = torch.full((Bn * t_max * c_ld + 2 * self.g,), NAN, dtype=dtype, device=DEV)
        self.v = self.buf[self.g:self.g + Bn * t_max * c_ld].view(Bn, t_max, c_ld)

    def bits(self):
        return self.buf.view(BITS[self.buf.dtype]).cpu()


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=TAG.get)
def test_kv_append(dtype):
    """Row t, columns < n, becomes src bit for bit; every other element of the cache and of its
    guard bands stays NaN; t >= t_max writes nothing.  B n = 5000: 20 work groups, the last partly
    filled; n < c_ld, src_ld > n."""
    Bn, n, c_ld, src_ld, t_max = 5, 1000, 1032, 1016, 4
    g = torch.Generator().manual_seed(3)
    src = torch.randn(Bn, src_ld, generator=g).to(dtype).to(DEV)
    for t in (0, 1, t_max - 1, t_max, t_max + 3):
        cache = Cache(Bn, t_max, c_ld, dtype)
        ops.kv_append(src, src_ld, cache.v, t_max * c_ld, c_ld, n, Bn, i32([t]))
        torch.cuda.synchronize()
        want = Cache(Bn, t_max, c_ld, dtype)
        want.v.copy_(R.ref_kv_append(want.v.cpu(), src.cpu(), t, n))
        assert torch.equal(cache.bits(), want.bits()), f"t = {t}"
        assert int((~torch.isnan(cache.buf.float())).sum()) == (Bn * n if t < t_max else 0)


def test_kv_append_rejections():
    Bn, n, c_ld, t_max = 2, 64, 64, 2
    src = torch.zeros(Bn, n, dtype=BF16, device=DEV)
    t = i32([0])
    L = _lib.lib()
    for what, (s, c, tp, nn, bb, dt) in {
            "unknown dtype": (1, 1, 1, n, Bn, 7), "null src": (0, 1, 1, n, Bn, 1), "null cache": (1, 0, 1, n, Bn, 1),
            "null t_ptr": (1, 1, 0, n, Bn, 1), "n 0": (1, 1, 1, 0, Bn, 1), "batch 0": (1, 1, 1, n, 0, 1),
            "batch -1": (1, 1, 1, n, -1, 1)}.items():
        cache = Cache(Bn, t_max, c_ld, BF16)
        rc = L.tt2_kv_append(src.data_ptr() if s else None, n, cache.v.data_ptr() if c else None, t_max * c_ld, c_ld,
                             nn, bb, t.data_ptr() if tp else None, dt, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.E_INVALID, (what, rc)
        assert torch.isnan(cache.buf).all(), what


# ------------------------------------------------------------------ tt2_decode_emit and the skinny emit epilogue
NM, HLD = 80, 96


class EmitBuffers:
    """mel_seq, stop_seq, prev (NaN-filled, guarded), stop_len, t, seed, done on the device."""

    def __init__(self, Bn, prev_dtype, seed0=0xFFFFFFFE, with_seed=True, with_stop_len=True):
        self.B = Bn
        self.mel = RowGuarded((Bn * R.EMIT_TMAX, NM))
        self.stop = RowGuarded((Bn * R.EMIT_TMAX,))
        self.prev = RowGuarded((Bn, NM), prev_dtype)
        self.stop_len = i32([R.INT32_MAX] * Bn) if with_stop_len else None
        self.t = i32([0])
        self.seed = torch.tensor([seed0 - (1 << 32) if seed0 >= (1 << 31) else seed0], dtype=torch.int32, device=DEV) \
            if with_seed else None
        self.done = i32([0])

    def state(self):
        """The fields of R.emit_sequence's states, read back; the guards are checked on the way."""
        torch.cuda.synchronize()
        for gb, what in ((self.mel, "mel_seq"), (self.stop, "stop_seq"), (self.prev, "prev")):
            b = gb.buf.float().cpu()
            assert torch.isnan(b[:gb.g]).all() and torch.isnan(b[gb.g + gb.n:]).all(), f"{what}: guard written"
        return {"mel_seq": self.mel.cpu().view(self.B, R.EMIT_TMAX, NM),
                "stop_seq": self.stop.cpu().view(self.B, R.EMIT_TMAX),
                "prev": self.prev.cpu(), "stop_len": None if self.stop_len is None else self.stop_len.cpu(),
                "t": int(self.t), "seed": None if self.seed is None else int(self.seed) & 0xFFFFFFFF}


def _emit_heads(Bn, seed=0):
    """The scripted steps as f32 heads [B, HLD] (NaN past column n_mels: never read)."""
    coarse, fine, bias, want = R.emit_script(Bn)
    g = torch.Generator().manual_seed(seed)
    steps = []
    for s in range(coarse.shape[0] + 1):          # one more call past t_max + 1
        h = torch.full((Bn, HLD), NAN)
        h[:, :NM] = torch.randn(Bn, NM, generator=g)
        h[:, NM] = (coarse[min(s, R.EMIT_TMAX)] + fine[min(s, R.EMIT_TMAX)]).to(F32)
        steps.append(h)
    return steps, bias, want


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=TAG.get)
@pytest.mark.parametrize("variant", ["all", "no_seed", "no_stop_len", "no_stop_bias"])
def test_decode_emit_scripted(variant, dtype):
    """The scripted sequence (R.emit_script: a logit equal to the threshold, one just below it, a
    row that crosses twice, one lifted by stop_bias alone, one that never stops) over t_max = 4 and
    two calls past it: mel_seq, stop_seq, prev, stop_len, *t and *seed bit-equal to ref_emit after
    every call.  B (n_mels + 1) = 324 elements: two passes of the 256-thread loop."""
    Bn = 4
    steps, bias, want = _emit_heads(Bn)
    bufs = EmitBuffers(Bn, dtype, with_seed=variant != "no_seed", with_stop_len=variant != "no_stop_len")
    sb = None if variant == "no_stop_bias" else bias
    sbd = None if sb is None else sb.to(DEV)
    ref = R.emit_sequence(R.ref_emit, [h[:, :NM + 1] for h in steps], R.EMIT_TMAX, NM, sb,
                          None if bufs.stop_len is None else bufs.stop_len.cpu(), R.EMIT_THR,
                          None if bufs.seed is None else 0xFFFFFFFE, dtype)
    for s, h in enumerate(steps):
        hd = h.to(DEV)
        ops.decode_emit(hd, HLD, Bn, NM, R.EMIT_TMAX, bufs.mel.v, bufs.stop.v, bufs.prev.v, bufs.t, seed=bufs.seed,
                        stop_bias=sbd, stop_len=bufs.stop_len, stop_thr=R.EMIT_THR)
        bad = R.same_state(bufs.state(), ref[s])
        assert not bad, f"call {s}: {bad} differ from ref_emit"
    if variant == "all":
        assert torch.equal(ref[-1]["stop_len"], want) and ref[-1]["t"] == R.EMIT_TMAX and ref[-1]["seed"] == 2


def test_decode_emit_rejections():
    Bn = 2
    heads = torch.zeros(Bn, HLD, device=DEV)
    L = _lib.lib()
    ok = dict(heads=1, ld=HLD, b=Bn, nm=NM, tmax=R.EMIT_TMAX, mel=1, stop=1, prev=1, dt=1, t=1)
    for what, ch in {"null heads": dict(heads=0), "null mel_seq": dict(mel=0), "null stop_seq": dict(stop=0),
                     "null prev": dict(prev=0), "null t_ptr": dict(t=0), "batch 0": dict(b=0), "n_mels 0": dict(nm=0),
                     "t_max 0": dict(tmax=0), "heads_ld = n_mels": dict(ld=NM), "unknown prev_dtype": dict(dt=9)}.items():
        a = dict(ok, **ch)
        bufs = EmitBuffers(Bn, BF16)
        rc = L.tt2_decode_emit(heads.data_ptr() if a["heads"] else None, a["ld"], a["b"], a["nm"], a["tmax"],
                               bufs.mel.ptr() if a["mel"] else None, bufs.stop.ptr() if a["stop"] else None,
                               bufs.prev.ptr() if a["prev"] else None, a["dt"], bufs.t.data_ptr() if a["t"] else None,
                               bufs.seed.data_ptr(), None, bufs.stop_len.data_ptr(), 0.5, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.E_INVALID, (what, rc)
        for gb in (bufs.mel, bufs.stop, bufs.prev):
            gb.untouched(what)
        assert int(bufs.t) == 0 and int(bufs.seed) == -2 and int(bufs.stop_len[0]) == R.INT32_MAX


K_EMIT, FINE_COL = 512, 128      # k = 0 (wave 0's slice) carries the coarse logit, k = 128 (wave 1's) the fine part


def _emit_gemm_problem(m, seed=0):
    """W [81, 512], bias [81] and one A [m, 512] per call whose product is the scripted heads
    exactly: the mel columns are integer sums below 2^24; the stop column reads A[:, 0] (coarse) and
    A[:, 128] * 2^-13 (fine = 0 or -2^-25 as -2^-12 * 2^-13, both factors bf16 and f16 values)."""
    coarse, fine, bias_sb, want = R.emit_script(m)
    g = torch.Generator().manual_seed(100 + seed)
    W = torch.randint(-2, 3, (NM + 1, K_EMIT), generator=g).to(F64)
    W[:NM, 0] = W[:NM, FINE_COL] = 0
    W[NM] = 0
    W[NM, 0], W[NM, FINE_COL] = 1.0, 2.0 ** -13
    bias = torch.randint(-3, 4, (NM + 1,), generator=g).to(F64)
    bias[NM] = 0
    As = []
    for s in range(coarse.shape[0] + 1):
        A = torch.randint(-2, 3, (m, K_EMIT), generator=g).to(F64)
        A[:, 0], A[:, FINE_COL] = coarse[min(s, R.EMIT_TMAX)], fine[min(s, R.EMIT_TMAX)] * 2.0 ** 13
        As.append(A)
    return W, bias, As, bias_sb, want


@pytest.mark.parametrize("dtype", [BF16, F16], ids=TAG.get)
@pytest.mark.parametrize("m", [1, 17, 32, 33, 64])
def test_skinny_emit_equals_decode_emit(m, dtype):
    """The heads GEMM with the emit epilogue, stop fields included, against the same GEMM without
    it followed by tt2_decode_emit, on the scripted sequence: both sets of buffers bit-equal to each
    other and to ref_emit after every call, heads bit-equal to the exact product, *emit_done back
    at 0.  m = 1 .. 64: both row-block instantiations and ragged last blocks."""
    W, bias, As, sb, want = _emit_gemm_problem(m)
    assert representable(W, dtype) and all(representable(A, dtype) for A in As)
    heads64 = [A @ W.t() + bias for A in As]
    assert all(representable(h, F32) for h in heads64) and (W.abs().sum(1).max() * 2 + 3) < 2 ** 24
    Wd, bd, sbd = dev(W, dtype), dev(bias, F32), sb.to(DEV)
    fused, split = EmitBuffers(m, dtype), EmitBuffers(m, dtype)
    ref = R.emit_sequence(R.ref_emit, [h.to(F32) for h in heads64], R.EMIT_TMAX, NM, sb, fused.stop_len.cpu(), R.EMIT_THR,
                          0xFFFFFFFE, dtype)
    written = torch.arange(HLD - 8) <= NM
    for s, A in enumerate(As):
        Ad = dev(A, dtype)
        h1, h2 = Guarded(m, HLD - 8, F32), Guarded(m, HLD - 8, F32)
        assert h1.ld == HLD
        ops.gemm(Ad, Wd, h1.body, m, NM + 1, K_EMIT, K_EMIT, K_EMIT, HLD, bias=bd, variant=3,
                 emit=(fused.mel.v, fused.stop.v, fused.prev.v, fused.t, fused.seed, fused.done, NM, R.EMIT_TMAX,
                       sbd, fused.stop_len, R.EMIT_THR))
        ops.gemm(Ad, Wd, h2.body, m, NM + 1, K_EMIT, K_EMIT, K_EMIT, HLD, bias=bd, variant=3)
        ops.decode_emit(h2.body, HLD, m, NM, R.EMIT_TMAX, split.mel.v, split.stop.v, split.prev.v, split.t,
                        seed=split.seed, stop_bias=sbd, stop_len=split.stop_len, stop_thr=R.EMIT_THR)
        sf, ss = fused.state(), split.state()
        for hh in (h1, h2):
            hh.check("heads", written)
            assert torch.equal(hh.body[:, :NM + 1].cpu().to(F64), heads64[s]), \
                f"call {s}: heads differ from the exact product"
        assert not R.same_state(sf, ref[s]), f"call {s}: fused emit {R.same_state(sf, ref[s])} differ from ref_emit"
        assert not R.same_state(ss, ref[s]), f"call {s}: tt2_decode_emit {R.same_state(ss, ref[s])} differ from ref_emit"
        assert int(fused.done) == 0
    assert torch.equal(ref[-1]["stop_len"], want)


# ------------------------------------------------------------------ skinny KV scatter, PE, LN prologue
def _int_gemm(m, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    A, W = (torch.randint(-1, 2, sh, generator=g).to(F64) for sh in ((m, k), (n, k)))
    return A, W, torch.randint(-3, 4, (n,), generator=g).to(F64)


@pytest.mark.parametrize("dtype,m", [(BF16, 17), (F16, 33)], ids=["bf16-17", "f16-33"])
def test_skinny_kv_scatter_exact(dtype, m):
    """C = A W^T + bias exact (integers below 256); the cache row *kv_t becomes C[:, kv_col0:] bit
    for bit, everything else of the guarded cache stays NaN; t = t_max writes no cache row."""
    n, k, col0, t_max = 208, 512, 80, 3
    kv_ld = n - col0 + 8
    A, W, bias = _int_gemm(m, n, k, 5)
    ref = A @ W.t() + bias
    assert representable(ref, dtype) and ref.abs().max() < 256
    Ad, Wd, bd = dev(A, dtype), dev(W, dtype), dev(bias, F32)
    for t in (0, t_max - 1, t_max):
        Cg, cache = Guarded(m, n, dtype), Cache(m, t_max, kv_ld, dtype)
        ops.gemm(Ad, Wd, Cg.body, m, n, k, k, k, Cg.ld, bias=bd, kv=(cache.v, i32([t]), col0, t_max * kv_ld, kv_ld),
                 variant=3)
        torch.cuda.synchronize()
        Cg.check("C")
        assert torch.equal(Cg.body.cpu().to(F64), ref), f"t = {t}: C differs from the exact product"
        want = Cache(m, t_max, kv_ld, dtype)
        want.v.copy_(R.ref_kv_append(want.v.cpu(), ref[:, col0:].to(dtype), t, n - col0))
        assert torch.equal(cache.bits(), want.bits()), f"t = {t}: cache"


@pytest.mark.parametrize("dtype,m", [(BF16, 33), (F16, 17)], ids=["bf16-33", "f16-17"])
def test_skinny_pe_epilogue_exact(dtype, m):
    """C = A W^T + bias + alpha pe[*t] with alpha = 1 / 2 and a table of half-integers: exact in
    f32, rounded once at the store."""
    n, k, rows = 208, 512, 5
    A, W, bias = _int_gemm(m, n, k, 6)
    g = torch.Generator().manual_seed(8)
    table = torch.randint(-8, 9, (rows, n), generator=g).to(F64) / 2
    Ad, Wd, bd, td, al = dev(A, dtype), dev(W, dtype), dev(bias, F32), dev(table, F32), dev(torch.tensor([0.5]), F32)
    for t in (0, rows - 1):
        ref = A @ W.t() + bias + 0.5 * table[t]
        assert representable(ref, F32)
        Cg = Guarded(m, n, dtype)
        ops.gemm(Ad, Wd, Cg.body, m, n, k, k, k, Cg.ld, bias=bd, pe=(td, al, i32([t])), variant=3)
        torch.cuda.synchronize()
        Cg.check("C")
        assert torch.equal(Cg.body.cpu(), ref.to(dtype)), f"t = {t}"


@pytest.mark.parametrize("m", [1, 17, 32])
def test_skinny_ln_prologue(m):
    """h_out = LN(x + branch): bit-equal on the LnFwdExact design, per row under
    _norm_refs.worst_ratio_by on ln_random's ill-conditioned rows (the judge and constants of
    test_ln_random_per_row); C bit-equal to a second skinny GEMM on the stored h_out."""
    n, k = 81, N.LN_C
    g = torch.Generator().manual_seed(m)
    W = dev(torch.randn(n, k, generator=g) * 0.05, BF16)

    def run(x, br, gamma, beta, eps):
        h, Cg = RowGuarded((m, k), BF16), Guarded(m, n, BF16)
        xd, brd = dev(x, BF16), dev(br, BF16)
        ops.gemm(xd, W, Cg.body, m, n, k, k, k, Cg.ld, a_ln=(brd, dev(gamma, F32), dev(beta, F32), h.v, eps), variant=3)
        C2 = Guarded(m, n, BF16)
        ops.gemm(h.v, W, C2.body, m, n, k, k, k, C2.ld, variant=3)
        torch.cuda.synchronize()
        for o, what in ((h, "h_out"), (Cg, "C"), (C2, "C of the stored h_out")):
            o.check(what)
        assert torch.equal(Cg.buf.view(torch.int16).cpu(), C2.buf.view(torch.int16).cpu()), \
            "C differs from the GEMM of h_out"
        return h.cpu()

    pr = N.LnFwdExact(m, 0.0, True)
    assert pr.exact()[0]
    ry = N.ref_ln_fwd(pr.x, pr.branch, None, pr.gamma, pr.beta, pr.EPS)[0]
    assert torch.equal(run(pr.x, pr.branch, pr.gamma, pr.beta, pr.EPS), ry.to(BF16)), "exact design: h_out"
    x, br, gamma, beta, _, kind = N.ln_random(m, BF16, m)
    r64 = N.ref_ln_fwd(x, br, None, gamma, beta, 1e-5)
    r32 = N.ref_ln_fwd(x, br, None, gamma, beta, 1e-5, dtype=F32)
    ratio, row = N.worst_ratio_by(run(x, br, gamma, beta, 1e-5), r64[0], r32[0], BF16)
    print(f"\nskinny ln prologue m={m}: h_out {ratio:.3f}@{row}")       # MI355X: 0.250 at every m
    assert ratio <= 1, f"h_out: ratio {ratio:.3f} at row {row}"
