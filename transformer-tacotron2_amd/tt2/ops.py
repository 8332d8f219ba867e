"""Thin torch-tensor wrappers over the libtt2 C ABI (no compute in Python).

Every function takes preallocated output tensors and launches on the current
torch stream; nothing here allocates except ``Workspace.get`` outside capture.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib
from ._lib import GemmArgs, check, dt, lib, ptr, stream_ptr

# hipGraph capture mode of the training-step and decode-step graphs.  thread_local: RCCL's
# watchdog thread polls its work events during a capture, which a global-mode capture
# treats as a prohibited call (env TT2_CAPTURE_MODE: an A/B switch).
CAPTURE_MODE = os.environ.get("TT2_CAPTURE_MODE", "thread_local")


def drop_thr(p: float) -> int:
    """floor(p * 2^32) -- identical to the oracle's threshold."""
    return int(p * 4294967296.0) if p > 0 else 0


class Drop:
    """Dropout site descriptor: (device seed tensor uint32[1], site id, p)."""

    __slots__ = ("seed", "site", "p")

    def __init__(self, seed: torch.Tensor | None, site: int, p: float):
        self.seed, self.site, self.p = seed, site, p

    @property
    def active(self) -> bool:
        return self.seed is not None and self.p > 0

    def fields(self):
        if not self.active:
            return None, 0, 0, 1.0
        return self.seed.data_ptr(), self.site, drop_thr(self.p), 1.0 / (1.0 - self.p)


NO_DROP = Drop(None, 0, 0.0)


class Workspace:
    """Grow-only device scratch buffer (size it before graph capture)."""

    def __init__(self):
        self.buf: torch.Tensor | None = None

    def get(self, nbytes: int) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.TT2Error("workspace must be sized before graph capture")
            self.buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device="cuda")
        return self.buf


_WS = Workspace()


def gemm_args(a, b, c, m, n, k, lda, ldb, ldc, trans_a=False, trans_b=False, bias=None, res=None, ldr=0,
              gate=None, ldg=0, gate_scale=1.0, alpha=1.0, beta=0.0, act=0, drop: Drop = NO_DROP, splits=1,
              a_conv=None, b_conv=None, ws: Workspace | None = None, variant: int = 0, a_ksum=None,
              a_ksum_beta=0.0, a_ln=None, kv=None, pe=None, emit=None, main_only=False,
              defer_ws: bool = False, col_stats=None, bn_bwd=None) -> GemmArgs:
    """Build the tt2_gemm_args of one request (see tt2_capi.h).  defer_ws: only size the
    split-K workspace (ws_bytes); the caller places it."""
    L = lib()
    g = GemmArgs()
    g.a, g.b, g.c = a.data_ptr(), b.data_ptr(), c.data_ptr()
    g.bias = ptr(bias)
    g.res, g.gate = ptr(res), ptr(gate)
    g.lda, g.ldb, g.ldc, g.ldr, g.ldg = lda, ldb, ldc, ldr, ldg
    g.m, g.n, g.k = m, n, k
    g.dtype_in, g.dtype_out = dt(a), dt(c)
    if b.dtype != a.dtype:
        raise _lib.TT2Error("gemm: A and B dtypes differ")
    g.res_dtype = dt(res) if res is not None else 0
    g.gate_dtype = dt(gate) if gate is not None else 0
    if bias is not None and bias.dtype != torch.float32:
        raise _lib.TT2Error("gemm: bias must be f32")
    g.trans_a, g.trans_b = int(trans_a), int(trans_b)
    g.act = act
    g.alpha, g.beta, g.gate_scale = alpha, beta, gate_scale
    g.drop_seed, g.drop_site, g.drop_thr, g.drop_scale = drop.fields()
    if a_conv is not None:
        g.a_conv_t, g.a_conv_c, g.a_conv_pad = a_conv
    if b_conv is not None:
        g.b_conv_t, g.b_conv_c, g.b_conv_pad = b_conv
    g.kernel_variant = variant
    g.col_stats = ptr(col_stats)
    if bn_bwd is not None:   # a _lib.BnArgs (bn_bwd_args); kept alive on the args for the call
        g.bn_bwd = C.addressof(bn_bwd)
        g._bn_keep = bn_bwd
    g.a_ksum, g.a_ksum_beta = ptr(a_ksum), a_ksum_beta
    if a_ln is not None:
        br, gam, bet, out, eps = a_ln
        g.a_ln_branch, g.a_ln_gamma, g.a_ln_beta, g.a_ln_out, g.a_ln_eps = ptr(br), ptr(gam), ptr(bet), ptr(out), eps
    if kv is not None:
        cache, t_ptr, col0, bstride, ld = kv
        g.kv_cache, g.kv_t, g.kv_col0, g.kv_bstride, g.kv_ld = ptr(cache), ptr(t_ptr), col0, bstride, ld
    if pe is not None:
        table, alpha, t_ptr = pe
        g.pe_table, g.pe_alpha, g.pe_t = ptr(table), ptr(alpha), ptr(t_ptr)
    if emit is not None:
        mel_seq, stop_seq, prev, t_ptr, seed, done, n_mels, t_max = emit[:8]
        g.emit_mel, g.emit_stop, g.emit_prev = ptr(mel_seq), ptr(stop_seq), ptr(prev)
        g.emit_t, g.emit_seed, g.emit_done = ptr(t_ptr), ptr(seed), ptr(done)
        g.emit_nmels, g.emit_tmax = n_mels, t_max
        if len(emit) == 11:
            stop_bias, stop_len, stop_thr = emit[8:]
            g.emit_stop_bias, g.emit_stop_len, g.emit_stop_thr = ptr(stop_bias), ptr(stop_len), stop_thr
        elif len(emit) != 8:
            raise _lib.TT2Error("gemm: emit takes 8 or 11 fields")
    g.splits = max(1, splits)
    g.main_only = int(main_only)   # dev measurement: skip the split-K reduce
    if g.splits > 1:
        need = L.tt2_gemm_workspace_size(C.byref(g))
        g.ws_bytes = need
        if not defer_ws:
            g.workspace = (ws or _WS).get(need).data_ptr()
    return g


def gemm_stats_rows(a, b, c, m, n, k, lda, ldb, ldc, **kw) -> int:
    """Rows per chunk of this request's fused BatchNorm statistics (col_stats / bn_bwd): 64 on
    the 64 x 64 kernel, 256 on the 256 x 128 one, 0 when it cannot fuse them."""
    return int(lib().tt2_gemm_stats_rows(C.byref(gemm_args(a, b, c, m, n, k, lda, ldb, ldc, defer_ws=True, **kw))))


def gemm_algo_bytes(g) -> int:
    """Algorithmic HBM bytes of one GEMM request: each operand once (an implicit-im2col
    operand as its unique sequence rows, not the tap-expanded matrix), C once, and every
    epilogue input once (residual, gate, beta * C, the BatchNorm rows of a bn_bwd epilogue,
    bias)."""
    esz = 2 if g.dtype_in == _lib.DT_BF16 else 4
    sz = lambda d: 2 if d == _lib.DT_BF16 else 4  # noqa: E731
    mn = g.m * g.n
    a_b = esz * g.m * (g.a_conv_c if g.a_conv_t > 0 else g.k)
    b_b = esz * (g.k * g.b_conv_c if g.b_conv_t > 0 else g.n * g.k)
    out = a_b + b_b + sz(g.dtype_out) * mn
    if g.res:
        out += sz(g.res_dtype) * mn
    if g.gate:
        out += sz(g.gate_dtype) * mn
    if g.beta != 0.0:
        out += sz(g.dtype_out) * mn
    if g.bn_bwd:
        out += 2 * mn
    if g.bias:
        out += 4 * g.n
    return out


def gemm(a, b, c, m, n, k, lda, ldb, ldc, **kw):
    """C[m,n] = epi(alpha * sum_k A(m,k) B(n,k)); see tt2_capi.h tt2_gemm_args.
    a_ksum (f32 [m], bf16 trans_a only): a_ksum = a_ksum_beta * a_ksum + sum_k A(m,k).
    a_ln = (branch, gamma, beta, out, eps): multiply LN(A + branch), writing it to out (skinny path).
    kv = (cache, t_ptr, col0, bstride, ld): also store columns >= col0 to the KV cache at step *t_ptr.
    pe = (table, alpha, t_ptr): add alpha * table[*t_ptr] to every output row (skinny path).
    emit = (mel_seq, stop_seq, prev, t_ptr, seed, done, n_mels, t_max): the decode frame emit
    (see tt2_capi.h), which also advances *t_ptr; three more fields, (..., stop_bias, stop_len, stop_thr),
    set its stop handling (emit_stop_bias / emit_stop_len / emit_stop_thr; either tensor may be None).
    col_stats (f32, 2 * ceil(m / rows) * n, rows = gemm_stats_rows(...)): the stored C's column
    moments per chunk (mean, M2), for batchnorm_fwd(stats=(col_stats, rows)).
    bn_bwd (bn_bwd_args(...)): C is that BatchNorm backward's dout; its per-chunk sums go to the
    args' stats buffer, for batchnorm_bwd(stats=(buf, rows))."""
    L = lib()
    g = gemm_args(a, b, c, m, n, k, lda, ldb, ldc, **kw)
    if PROBE is not None:
        key = ("gemm", L.tt2_gemm_plan(C.byref(g)), g.trans_a, g.trans_b)
        algo_bytes = gemm_algo_bytes(g)
        PROBE.begin()
        check(L.tt2_gemm(C.byref(g), stream_ptr()), "tt2_gemm")
        PROBE.end(key, 2.0 * m * n * k, algo_bytes, [g])
        return c
    check(L.tt2_gemm(C.byref(g), stream_ptr()), "tt2_gemm")
    return c


def gemm_grouped(problems, ws: Workspace | None = None, fin=None, max_groups: int = 0):
    """One tt2_gemm_grouped launch (v7) over up to 8 requests, each a dict of gemm()
    arguments (a, b, c, m, n, k, lda, ldb, ldc + keywords); their split-K slabs get
    disjoint slices of one workspace.  fin: a deferred layernorm_bwd's returned LnArgs,
    completed in the group's reduce launch (tt2_gemm_grouped_fin).  max_groups > 0: at most
    that many work groups walk the items (tt2_gemm_grouped_ex)."""
    L = lib()
    finp = C.addressof(fin) if fin is not None else None
    arr = (GemmArgs * len(problems))()
    offs, total = [], 0
    for i, p in enumerate(problems):
        arr[i] = gemm_args(defer_ws=True, **p)
        offs.append(total)
        total += (arr[i].ws_bytes + 255) // 256 * 256
    if total:
        base = (ws or _WS).get(total).data_ptr()
        for i in range(len(problems)):
            if arr[i].splits > 1:
                arr[i].workspace = base + offs[i]
    if PROBE is not None:
        key = ("gemm_grouped", 13, arr[0].trans_a, arr[0].trans_b)
        flops = sum(2.0 * g.m * g.n * g.k for g in arr)
        ab = sum(gemm_algo_bytes(g) for g in arr)
        PROBE.begin()
        check(L.tt2_gemm_grouped_ex(arr, len(problems), finp, max_groups, stream_ptr()), "tt2_gemm_grouped")
        # work groups of the call, and its kernel dispatches (a capped grid goes out as consecutive
        # launches of at most the cap, rounded down to a multiple of 8: tt2_gemm_grouped_ex)
        items = sum(((g.m + 255) // 256) * ((g.n + 127) // 128) * max(1, g.splits) for g in arr)
        grid = min(items, max(8, max_groups // 8 * 8)) if max_groups > 0 else items
        PROBE.end(key, flops, ab, list(arr), wgs=items, disp=-(-items // grid))
        return
    check(L.tt2_gemm_grouped_ex(arr, len(problems), finp, max_groups, stream_ptr()), "tt2_gemm_grouped")


class LaunchProbe:
    """Times each GEMM's main kernel inside the step with libtt2's launch probe
    (tt2_probe_arm: eager, start / stop events at the kernel's own dispatch and completion,
    as rocprofv3 measures it; eager or captured, the kernel's own wall-clock span); used by
    bench.py for the live per-kernel roofline figure."""

    def __init__(self):
        self.rec = []
        self.wgs = {}    # key -> [work groups of each recorded grouped call]
        self.disp = {}   # key -> [kernel dispatches of each recorded call] (grouped: capped grids)
        self._s = None

    def begin(self):
        self._s = lib().tt2_probe_arm()
        if self._s < 0:
            check(self._s, "tt2_probe_arm")

    def end(self, key, flops, algo_bytes=0, args=None, wgs=None, disp=1):
        if wgs is not None:
            self.wgs.setdefault(key, []).append(wgs)
        self.disp.setdefault(key, []).append(disp)
        e = None
        saved = None
        if args is not None:   # a copy of the launch's tt2_gemm_args (array for a grouped launch)
            saved = (GemmArgs * len(args))()
            for i, g in enumerate(args):
                saved[i] = g
        self.rec.append((key, flops, self._s, e, algo_bytes, saved))

    def summary(self, span: bool = False):
        """{key: [launches, flops, seconds, algorithmic bytes]}.  Seconds are the dispatch
        events' (eager launches), or with `span` the kernels' own wall-clock spans (the only
        record of a launch inside a captured graph; reading one re-arms it for the next
        replay)."""
        torch.cuda.synchronize()
        out = {}
        L = lib()
        for key, flops, slot, _, ab, _ in self.rec:
            ms = L.tt2_probe_span_ms(slot) if span else L.tt2_probe_ms(slot)
            if ms < 0:
                msg = L.tt2_last_error()
                raise _lib.TT2Error(f"launch probe {slot} ({key}) recorded no {'span' if span else 'kernel'}"
                                    f"{' (' + msg.decode() + ')' if msg else ''}")
            d = out.setdefault(key, [0, 0.0, 0.0, 0.0])
            d[0] += 1
            d[1] += flops
            d[2] += ms * 1e-3
            d[3] += ab
        return out

    def close(self):
        lib().tt2_probe_reset()

    def replay_time(self, key, reps: int = 10) -> float:
        """Total device time of this variant's recorded launches, each re-launched
        `reps` times back-to-back between one event pair (amortises the
        per-launch dispatch gap that single-launch brackets include)."""
        L = lib()
        total = 0.0
        for k, _, _, _, _, saved in self.rec:
            if k != key or saved is None:
                continue
            torch.cuda.synchronize()
            for g in saved:
                g.main_only = 1      # the kernel alone (a split-K reduce is a different kernel)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                if len(saved) == 1 and k[0] == "gemm":
                    check(L.tt2_gemm(C.byref(saved[0]), stream_ptr()), "tt2_gemm(replay)")
                else:
                    check(L.tt2_gemm_grouped(saved, len(saved), stream_ptr()), "tt2_gemm_grouped(replay)")
            e.record()
            torch.cuda.synchronize()
            total += s.elapsed_time(e) * 1e-3 / reps
        return total


PROBE: LaunchProbe | None = None


# 0 = auto (v2 register-resident P), 1 = v1 (P through LDS); tests A/B both,
# TT2_ATTN_VARIANT lets bench/profiling runs compare them.
ATTN_VARIANT = int(os.environ.get("TT2_ATTN_VARIANT", "0"))


def _attn_common(q, k, v, q_ld, k_ld, v_ld, batch, heads, tq, tk, key_len, causal, scale):
    a = _lib.AttnArgs()
    a.variant = ATTN_VARIANT
    a.q, a.k, a.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    a.q_ld, a.k_ld, a.v_ld = q_ld, k_ld, v_ld
    if key_len is not None and key_len.dtype != torch.int32:
        raise _lib.TT2Error("attn: key_len must be int32")
    a.key_len = ptr(key_len)
    a.batch, a.heads, a.head_dim, a.tq, a.tk, a.causal = batch, heads, 64, tq, tk, int(causal)
    a.dtype = dt(q)
    a.scale = scale
    return a


def attn_fwd(q, k, v, out, lse, q_ld, k_ld, v_ld, o_ld, batch, heads, tq, tk, key_len=None, causal=False,
             scale=0.125):
    """out[b*tq+t, 64h:64h+64] = softmax(scale q k^T + mask) v ; lse [batch*heads, tq] (log2 domain)."""
    L = lib()
    a = _attn_common(q, k, v, q_ld, k_ld, v_ld, batch, heads, tq, tk, key_len, causal, scale)
    a.o_out, a.o_ld, a.lse = out.data_ptr(), o_ld, lse.data_ptr()
    check(L.tt2_attn_fwd(C.byref(a), stream_ptr()), "tt2_attn_fwd")
    return out


def attn_probs(q, k, lse, probs, q_ld, k_ld, batch, heads, tq, tk, key_len=None, causal=False, scale=0.125):
    """Attention probabilities [B*H, Tq, Tk] f32 of a forward already run (alignment diagnostics)."""
    a = _attn_common(q, k, k, q_ld, k_ld, k_ld, batch, heads, tq, tk, key_len, causal, scale)
    a.lse = lse.data_ptr()
    check(lib().tt2_attn_probs(C.byref(a), probs.data_ptr(), stream_ptr()), "tt2_attn_probs")
    return probs


def attn_bwd(q, k, v, o, dout, lse, delta, dq, dk, dv, q_ld, k_ld, v_ld, o_ld, do_ld, dq_ld, dk_ld, dv_ld,
             batch, heads, tq, tk, key_len=None, causal=False, scale=0.125, parts=0):
    """parts: 0 dQ and dK / dV, 1 dQ only, 2 dK / dV only (non-causal bf16; see tt2_attn_args)."""
    L = lib()
    a = _attn_common(q, k, v, q_ld, k_ld, v_ld, batch, heads, tq, tk, key_len, causal, scale)
    a.parts = parts
    a.o, a.dout, a.o_ld, a.do_ld = o.data_ptr(), dout.data_ptr(), o_ld, do_ld
    a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    a.dq_ld, a.dk_ld, a.dv_ld = dq_ld, dk_ld, dv_ld
    a.lse, a.delta = lse.data_ptr(), delta.data_ptr()
    check(L.tt2_attn_bwd(C.byref(a), stream_ptr()), "tt2_attn_bwd")


def _need(what, t, numel, dtype):
    if t.dtype != dtype or t.numel() < numel:
        raise _lib.TT2Error(f"{what}: needs {numel} elements of {dtype}, got {t.numel()} of {t.dtype}")


# The validators of the data-path wrappers (dtw .. regulate_*).  Each raises `err` with the op and the
# argument named: TT2Error by default, ValueError for regulate_* and forward_sum_*.

def _ld(t):
    """The leading dimension of a [..., rows, cols] view: its row stride, except that a single row's
    stride is arbitrary, so there any value that covers the row."""
    return t.stride(-2) if t.shape[-2] > 1 else max(t.stride(-2), t.shape[-1])


def _rows(who, name, t, dtype, rows=None, min_cols=0, err=_lib.TT2Error):
    """Check that t is a 2-D view of `dtype` with a contiguous last dim whose rows do not overlap, of
    `rows` rows (None: any) and at least min_cols columns; returns its leading dimension."""
    if t.dtype != dtype or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise err(f"{who}: {name} must be {dtype} [rows, cols] with a contiguous last dim, "
                  f"got {t.dtype} {tuple(t.shape)} of strides {t.stride()}")
    if (rows is not None and t.shape[0] != rows) or t.shape[1] < min_cols:
        raise err(f"{who}: {name} must be [{'any' if rows is None else rows}, >= {min_cols}], got {tuple(t.shape)}")
    ld = _ld(t)
    if ld < t.shape[1]:
        raise err(f"{who}: {name}'s rows overlap (stride {t.stride(0)} below {t.shape[1]} columns)")
    return ld


def _vec(who, name, t, n, dtype, exact=False, err=_lib.TT2Error):
    """Check that t (None: skipped) is contiguous, of `dtype`, and holds n elements: at least n in any
    shape, or with exact=True exactly [n]."""
    if t is None:
        return
    short = (t.dim() != 1 or t.shape[0] != n) if exact else t.numel() < n
    if t.dtype != dtype or short or not t.is_contiguous():
        raise err(f"{who}: {name} must be a contiguous {dtype} [{n}], got {t.dtype} {tuple(t.shape)}")


def _same_gpu(who, tensors, err=_lib.TT2Error):
    """Check that every tensor (None: skipped) is on one and the same GPU."""
    dev = None
    for t in tensors:
        if t is not None:
            dev = t.device if dev is None else dev
            if not t.is_cuda or t.device != dev:
                raise err(f"{who}: every tensor must be on the same GPU")


def _bind_workspace(g, need, ws):
    """Point g.workspace at `need` bytes of ws (None: the module's Workspace)."""
    if need:
        buf = (ws or _WS).get(need)
        g.workspace, g.workspace_bytes = buf.data_ptr(), buf.numel()


def _span(ld, rows, cols=64):
    """Elements a [rows, >= cols] tensor (or column-slice view of row stride ld) holds at least."""
    if rows > 0 and ld < cols:
        raise _lib.TT2Error(f"attn: leading dimension {ld} below the {cols} head columns")
    return rows * cols


def _attn_guide(what, rows, q_len, coef, sigma, guide_heads, batch, heads, tq):
    g = _lib.AttnGuide()
    _need(f"{what}: rows", rows, batch * heads * tq, torch.float32)
    if q_len is not None:
        _need(f"{what}: q_len", q_len, batch, torch.int32)
    if coef is not None:
        _need(f"{what}: coef", coef, 1, torch.float32)
    g.q_len, g.rows, g.coef, g.sigma, g.heads = ptr(q_len), rows.data_ptr(), ptr(coef), sigma, guide_heads
    return g


def attn_fwd_guided(q, k, v, out, lse, rows, q_ld, k_ld, v_ld, o_ld, batch, heads, tq, tk, key_len=None,
                    q_len=None, sigma=0.4, guide_heads=2, causal=False, scale=0.125):
    """attn_fwd that also stores g[n] = sum_t P[n, t] W[n, t] of the guided heads (h < guide_heads)
    into rows [batch*heads, tq] f32 (tt2_attn_guide); out and lse are attn_fwd's bit for bit."""
    L = lib()
    a = _attn_common(q, k, v, q_ld, k_ld, v_ld, batch, heads, tq, tk, key_len, causal, scale)
    hd = heads * 64
    cd = q.dtype
    _need("attn_fwd_guided: q", q, _span(q_ld, batch * tq, hd), cd)
    _need("attn_fwd_guided: k", k, _span(k_ld, batch * tk, hd), cd)
    _need("attn_fwd_guided: v", v, _span(v_ld, batch * tk, hd), cd)
    _need("attn_fwd_guided: out", out, _span(o_ld, batch * tq, hd), cd)
    _need("attn_fwd_guided: lse", lse, batch * heads * tq, torch.float32)
    if key_len is not None:
        _need("attn_fwd_guided: key_len", key_len, batch, torch.int32)
    g = _attn_guide("attn_fwd_guided", rows, q_len, None, sigma, guide_heads, batch, heads, tq)
    a.o_out, a.o_ld, a.lse = out.data_ptr(), o_ld, lse.data_ptr()
    check(L.tt2_attn_fwd_guided(C.byref(a), C.byref(g), stream_ptr()), "tt2_attn_fwd_guided")
    return out


def attn_bwd_guided(q, k, v, o, dout, lse, delta, dq, dk, dv, rows, coef, q_ld, k_ld, v_ld, o_ld, do_ld, dq_ld,
                    dk_ld, dv_ld, batch, heads, tq, tk, key_len=None, q_len=None, sigma=0.4, guide_heads=2,
                    causal=False, scale=0.125, parts=0):
    """attn_bwd of out + kappa * sum(rows): kappa is the device scalar coef (guided_attn_loss
    writes it), rows the guided forward's g buffer.  delta is left holding delta + kappa g."""
    L = lib()
    a = _attn_common(q, k, v, q_ld, k_ld, v_ld, batch, heads, tq, tk, key_len, causal, scale)
    hd = heads * 64
    cd = q.dtype
    for name, t, ld, n in (("q", q, q_ld, tq), ("k", k, k_ld, tk), ("v", v, v_ld, tk), ("o", o, o_ld, tq),
                           ("dout", dout, do_ld, tq), ("dq", dq, dq_ld, tq), ("dk", dk, dk_ld, tk),
                           ("dv", dv, dv_ld, tk)):
        _need(f"attn_bwd_guided: {name}", t, _span(ld, batch * n, hd), cd)
    _need("attn_bwd_guided: lse", lse, batch * heads * tq, torch.float32)
    _need("attn_bwd_guided: delta", delta, batch * heads * tq, torch.float32)
    if key_len is not None:
        _need("attn_bwd_guided: key_len", key_len, batch, torch.int32)
    if coef is None:
        raise _lib.TT2Error("attn_bwd_guided: coef required")
    g = _attn_guide("attn_bwd_guided", rows, q_len, coef, sigma, guide_heads, batch, heads, tq)
    a.parts = parts
    a.o, a.dout, a.o_ld, a.do_ld = o.data_ptr(), dout.data_ptr(), o_ld, do_ld
    a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    a.dq_ld, a.dk_ld, a.dv_ld = dq_ld, dk_ld, dv_ld
    a.lse, a.delta = lse.data_ptr(), delta.data_ptr()
    check(L.tt2_attn_bwd_guided(C.byref(a), C.byref(g), stream_ptr()), "tt2_attn_bwd_guided")


def guided_attn_loss(rows, term, coef, batch, heads, tq, tk, key_len=None, q_len=None, guide_heads=2, scale=10.0,
                     grad_scale=1.0, loss_out=None):
    """term = scale * sum(rows of the guided heads, all layers in `rows`) / N with
    N = len(rows) * guide_heads * sum_b Tx_b Ty_b; coef = scale * grad_scale / N (kappa of
    attn_bwd_guided); loss_out[0] += term.  N = 0: term = coef = 0, loss_out untouched."""
    if len(rows) > _lib.GUIDE_MAX_LAYERS:
        raise _lib.TT2Error(f"guided_attn_loss: at most {_lib.GUIDE_MAX_LAYERS} layers")
    a = _lib.GuideLossArgs()
    for i, r in enumerate(rows):
        _need(f"guided_attn_loss: rows[{i}]", r, batch * heads * tq, torch.float32)
        a.rows[i] = r.data_ptr()
    _need("guided_attn_loss: term", term, 1, torch.float32)
    _need("guided_attn_loss: coef", coef, 1, torch.float32)
    for name, t in (("key_len", key_len), ("q_len", q_len)):
        if t is not None:
            _need(f"guided_attn_loss: {name}", t, batch, torch.int32)
    if loss_out is not None:
        _need("guided_attn_loss: loss_out", loss_out, 1, torch.float32)
    a.key_len, a.q_len, a.loss_out, a.term, a.coef = ptr(key_len), ptr(q_len), ptr(loss_out), term.data_ptr(), \
        coef.data_ptr()
    a.n_layers, a.batch, a.heads, a.guide_heads, a.tq, a.tk = len(rows), batch, heads, guide_heads, tq, tk
    a.scale, a.grad_scale = scale, grad_scale
    check(lib().tt2_guided_attn_loss(C.byref(a), stream_ptr()), "tt2_guided_attn_loss")


def attn_align(qs, ks, lses, pmax, amax, q_ld, k_ld, batch, heads, tq, tk, key_len=None, q_len=None,
               causal=False, scale=0.125, variant=None):
    """pmax[i, b*heads+h, n] = max_t P[n, t] and amax[...] = its key index (lowest on ties; -1 and 0
    for rows past q_len or without a visible key) of len(qs) forwards already run, in one launch:
    qs[i], ks[i] (row strides q_ld, k_ld; ks[i] may be a column slice of one wide buffer) and the
    saved lses[i] of layer slot i (tt2_align_args).  Non-causal only."""
    n = len(qs)
    if n > _lib.GUIDE_MAX_LAYERS:
        raise _lib.TT2Error(f"attn_align: at most {_lib.GUIDE_MAX_LAYERS} layers")
    if len(ks) != n or len(lses) != n:
        raise _lib.TT2Error("attn_align: one q, k and lse per layer")
    a = _lib.AlignArgs()
    hd = heads * 64
    cd = qs[0].dtype if n else torch.bfloat16
    if cd not in (torch.bfloat16, torch.float32):
        raise _lib.TT2Error(f"attn_align: q / k must be bf16 or f32, got {cd}")
    for i in range(n):
        _need(f"attn_align: q[{i}]", qs[i], _span(q_ld, batch * tq, hd), cd)
        _need(f"attn_align: k[{i}]", ks[i], _span(k_ld, batch * tk, hd), cd)
        _need(f"attn_align: lse[{i}]", lses[i], batch * heads * tq, torch.float32)
        a.q[i], a.k[i], a.lse[i] = qs[i].data_ptr(), ks[i].data_ptr(), lses[i].data_ptr()
    _need("attn_align: pmax", pmax, n * batch * heads * tq, torch.float32)
    _need("attn_align: amax", amax, n * batch * heads * tq, torch.int32)
    for name, t in (("key_len", key_len), ("q_len", q_len)):
        if t is not None:
            _need(f"attn_align: {name}", t, batch, torch.int32)
    a.q_ld, a.k_ld, a.key_len, a.q_len = q_ld, k_ld, ptr(key_len), ptr(q_len)
    a.pmax, a.amax = pmax.data_ptr(), amax.data_ptr()
    a.n_layers, a.batch, a.heads, a.head_dim, a.tq, a.tk = n, batch, heads, 64, tq, tk
    a.dtype = _lib.DT_BF16 if cd == torch.bfloat16 else _lib.DT_F32
    a.causal, a.scale = int(causal), scale   # (causal: refused by the library, as the guided calls are)
    a.variant = ATTN_VARIANT if variant is None else variant
    check(lib().tt2_attn_align(C.byref(a), stream_ptr()), "tt2_attn_align")
    return pmax, amax


def align_durations(pmax, amax, focus, sel, sel_focus, durations, n_layers, batch, heads, tq, tk, key_len=None,
                    q_len=None, head=None):
    """From attn_align's output: focus[i, b, h] = mean of pmax over the valid rows, the chosen head
    per utterance into sel [batch, 2] = (layer slot, head) (head=None: the greatest focus; head=(slot,
    h): that one for every utterance), its focus into sel_focus [batch], and durations[b, t] = the
    number of valid rows of the chosen head whose amax is t (tt2_align_dur_args).  Deterministic."""
    if n_layers > _lib.GUIDE_MAX_LAYERS:
        raise _lib.TT2Error(f"align_durations: at most {_lib.GUIDE_MAX_LAYERS} layers")
    a = _lib.AlignDurArgs()
    _need("align_durations: pmax", pmax, n_layers * batch * heads * tq, torch.float32)
    _need("align_durations: amax", amax, n_layers * batch * heads * tq, torch.int32)
    _need("align_durations: focus", focus, n_layers * batch * heads, torch.float32)
    _need("align_durations: sel", sel, 2 * batch, torch.int32)
    _need("align_durations: sel_focus", sel_focus, batch, torch.float32)
    _need("align_durations: durations", durations, batch * tk, torch.int32)
    for name, t in (("key_len", key_len), ("q_len", q_len)):
        if t is not None:
            _need(f"align_durations: {name}", t, batch, torch.int32)
    a.pmax, a.amax, a.key_len, a.q_len = pmax.data_ptr(), amax.data_ptr(), ptr(key_len), ptr(q_len)
    a.focus, a.sel, a.sel_focus, a.durations = focus.data_ptr(), sel.data_ptr(), sel_focus.data_ptr(), \
        durations.data_ptr()
    a.n_layers, a.batch, a.heads, a.tq, a.tk = n_layers, batch, heads, tq, tk
    if head is None:
        a.mode = 0
    else:
        a.mode, a.sel_layer, a.sel_head = 1, int(head[0]), int(head[1])
    check(lib().tt2_align_durations(C.byref(a), stream_ptr()), "tt2_align_durations")
    return durations


def align_monotonic(qs, ks, lses, path, durations, logp, q_ld, k_ld, batch, heads, tq, tk, key_len=None,
                    q_len=None, sel=None, head=None, scale=0.125, variant=None, ws=None):
    """Monotonic alignment search (tt2_align_mono_args) over the raw scores of forwards already
    run: per utterance the monotone path through one head's scores with the greatest sum, into
    path [batch, tq] int32 (-1 past q_len), durations [batch, tk] int32 and logp [batch] f32 (mean
    ln P along the path).  The head is sel [batch, 2] = (layer slot, head) on the device, as
    align_durations writes it, or head=(slot, h) for every utterance.  variant: None / 0 auto (bf16:
    MFMA score producer, f32: plain), 1 the plain scalar-dot producer.  Deterministic."""
    n = len(qs)
    if not 1 <= n <= _lib.GUIDE_MAX_LAYERS:
        raise _lib.TT2Error(f"align_monotonic: 1..{_lib.GUIDE_MAX_LAYERS} layers")
    if len(ks) != n or len(lses) != n:
        raise _lib.TT2Error("align_monotonic: one q, k and lse per layer")
    if (sel is None) == (head is None):
        raise _lib.TT2Error("align_monotonic: give either sel or head")
    a = _lib.AlignMonoArgs()
    hd = heads * 64
    cd = qs[0].dtype
    if cd not in (torch.bfloat16, torch.float32):
        raise _lib.TT2Error(f"align_monotonic: q / k must be bf16 or f32, got {cd}")
    for i in range(n):
        _need(f"align_monotonic: q[{i}]", qs[i], _span(q_ld, batch * tq, hd), cd)
        _need(f"align_monotonic: k[{i}]", ks[i], _span(k_ld, batch * tk, hd), cd)
        _need(f"align_monotonic: lse[{i}]", lses[i], batch * heads * tq, torch.float32)
        a.q[i], a.k[i], a.lse[i] = qs[i].data_ptr(), ks[i].data_ptr(), lses[i].data_ptr()
    _need("align_monotonic: path", path, batch * tq, torch.int32)
    _need("align_monotonic: durations", durations, batch * tk, torch.int32)
    _need("align_monotonic: logp", logp, batch, torch.float32)
    for name, t in (("key_len", key_len), ("q_len", q_len)):
        if t is not None:
            _need(f"align_monotonic: {name}", t, batch, torch.int32)
    if sel is not None:
        _need("align_monotonic: sel", sel, 2 * batch, torch.int32)
    else:
        a.sel_layer, a.sel_head = int(head[0]), int(head[1])
    a.q_ld, a.k_ld, a.key_len, a.q_len, a.sel = q_ld, k_ld, ptr(key_len), ptr(q_len), ptr(sel)
    a.path, a.durations, a.logp = path.data_ptr(), durations.data_ptr(), logp.data_ptr()
    a.n_layers, a.batch, a.heads, a.head_dim, a.tq, a.tk = n, batch, heads, 64, tq, tk
    a.dtype = _lib.DT_BF16 if cd == torch.bfloat16 else _lib.DT_F32
    a.causal, a.scale = 0, scale
    a.variant = 0 if variant is None else variant
    L = lib()
    need = L.tt2_align_monotonic_workspace_size(batch, tq, tk)
    if need:
        buf = (ws or _WS).get(need)
        a.workspace, a.workspace_bytes = buf.data_ptr(), buf.numel()
    check(L.tt2_align_monotonic(C.byref(a), stream_ptr()), "tt2_align_monotonic")
    return path, durations, logp


def dtw(a, b, total, length, a_len=None, b_len=None, cols=None, path_a=None, path_b=None, ws=None):
    """Dynamic time warping (tt2_dtw_args) between a [B, Ta, C] and b [B, Tb, C'] f32 (row views
    with a contiguous last dim are fine) over the feature columns cols = (c0, c1), default (0, C):
    total [B] f32 = the accumulated Euclidean frame distance along the best path, length [B] int32
    = its number of cells, and, when both are given, path_a / path_b [B, Ta + Tb - 1] int32 = its
    cells in forward order (-1 past length).  a_len / b_len [B] int32 bound the rows used.  On the
    current stream, no host synchronisation.  Deterministic."""
    who = "dtw"
    for name, t in (("a", a), ("b", b)):
        if t.dtype != torch.float32 or t.dim() != 3 or (t.shape[2] > 1 and t.stride(2) != 1):
            raise _lib.TT2Error(f"{who}: {name} must be f32 [B, T, C] with a contiguous last dim")
        if t.shape[0] > 1 and t.shape[1] > 0 and t.stride(0) != t.shape[1] * t.stride(1):
            raise _lib.TT2Error(f"{who}: {name}'s utterances must follow one another (stride(0) = T * stride(1))")
    B, ta, tb = a.shape[0], a.shape[1], b.shape[1]
    if b.shape[0] != B:
        raise _lib.TT2Error(f"{who}: a and b differ in batch")
    c0, c1 = (0, a.shape[2]) if cols is None else (int(cols[0]), int(cols[1]))
    if not (0 <= c0 < c1 <= min(a.shape[2], b.shape[2])) or c1 - c0 > _lib.DTW_MAX_FEATS:
        raise _lib.TT2Error(f"{who}: cols {(c0, c1)} must lie in both tensors and span 1..{_lib.DTW_MAX_FEATS}")
    if (path_a is None) != (path_b is None):
        raise _lib.TT2Error(f"{who}: give both path_a and path_b or neither")
    _vec(who, "total", total, B, torch.float32)
    for name, t in (("length", length), ("a_len", a_len), ("b_len", b_len)):
        _vec(who, name, t, B, torch.int32)
    for name, t in (("path_a", path_a), ("path_b", path_b)):
        _vec(who, name, t, B * max(0, ta + tb - 1), torch.int32)
    _same_gpu(who, (a, b, total, length, a_len, b_len, path_a, path_b))
    g = _lib.DtwArgs()
    g.a, g.b, g.a_len, g.b_len = a.data_ptr(), b.data_ptr(), ptr(a_len), ptr(b_len)
    g.total, g.length, g.path_a, g.path_b = total.data_ptr(), length.data_ptr(), ptr(path_a), ptr(path_b)
    g.a_ld, g.b_ld = _ld(a), _ld(b)
    g.batch, g.ta, g.tb, g.c0, g.c1 = B, ta, tb, c0, c1
    L = lib()
    _bind_workspace(g, L.tt2_dtw_workspace_size(B, ta, tb, int(path_a is not None)), ws)
    check(L.tt2_dtw(C.byref(g), stream_ptr()), "tt2_dtw")
    return total, length


def yin(x, utt_stride, f0, lag, aper, energy, hop, tau_min, tau_max, sr, threshold, frames=None, cmnd=None):
    """YIN pitch and RMS energy (tt2_yin_args) of the frames of x, a contiguous f32 buffer of padded
    samples: frame (b, f) is the 1024 samples from b * utt_stride + f * hop.  f0 / aper / energy
    [B, T] f32 and lag [B, T] int32 are written; frames [B] int32 bounds the valid frames of each
    utterance (the others get f0 0, lag -1, aper 1, energy 0); cmnd [B, T, ld] f32, when given,
    receives d'(0 .. tau_max) of every valid frame.  On the current stream, no host
    synchronisation.  Deterministic."""
    who = "yin"
    if f0.dim() != 2:
        raise _lib.TT2Error(f"{who}: f0 must be [B, T]")
    B, T = f0.shape
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise _lib.TT2Error(f"{who}: x must be a contiguous f32 buffer")
    utt_stride, hop = int(utt_stride), int(hop)
    if B and T and (utt_stride < 0 or hop < 1 or (B - 1) * utt_stride + (T - 1) * hop + _lib.YIN_FRAME > x.numel()):
        raise _lib.TT2Error(f"{who}: x holds {x.numel()} samples, fewer than the last frame needs")
    for name, t, dtype in (("f0", f0, torch.float32), ("lag", lag, torch.int32), ("aper", aper, torch.float32),
                           ("energy", energy, torch.float32)):
        _vec(who, name, t, B * T, dtype)
    _vec(who, "frames", frames, B, torch.int32)
    ld = 0
    if cmnd is not None:
        if cmnd.dim() != 3 or cmnd.shape[0] != B or cmnd.shape[1] != T:
            raise _lib.TT2Error(f"{who}: cmnd must be [B, T, ld]")
        ld = cmnd.shape[2]
        _vec(who, "cmnd", cmnd, B * T * ld, torch.float32)
    _same_gpu(who, (f0, x, lag, aper, energy, frames, cmnd))
    g = _lib.YinArgs()
    g.x, g.frames, g.cmnd = x.data_ptr(), ptr(frames), ptr(cmnd)
    g.f0, g.lag, g.aper, g.energy = f0.data_ptr(), lag.data_ptr(), aper.data_ptr(), energy.data_ptr()
    g.utt_stride, g.cmnd_ld = utt_stride, ld
    g.batch, g.t, g.hop, g.tau_min, g.tau_max = B, T, hop, int(tau_min), int(tau_max)
    g.sr, g.threshold = float(sr), float(threshold)
    check(lib().tt2_yin(C.byref(g), stream_ptr()), "tt2_yin")
    return f0, lag, aper, energy


def pitch_track(cmnd, frames, f0, lag, cost, tau_min, tau_max, sr, pos, jump, switch, unvoiced, ws=None):
    """Viterbi pitch tracking (tt2_pitch_track_args) over cmnd [B, T, ld] f32, the d' that yin
    writes (a row view with a contiguous last dim is fine): f0 [B, T] f32, lag [B, T] int32 (0
    unvoiced, -1 past the utterance) and cost [B] f32 are written.  frames [B] int32 (or None: T)
    bounds the valid frames of each utterance; pos [>= tau_max + 1] f32 places each lag on the axis
    that `jump` prices; `switch` is paid on a change of voicing and `unvoiced` per unvoiced frame.
    On the current stream, no host synchronisation.  Deterministic."""
    who = "pitch_track"
    if cmnd.dtype != torch.float32 or cmnd.dim() != 3 or (cmnd.shape[2] > 1 and cmnd.stride(2) != 1):
        raise _lib.TT2Error(f"{who}: cmnd must be f32 [B, T, ld] with a contiguous last dim")
    B, T, width = cmnd.shape
    tau_min, tau_max = int(tau_min), int(tau_max)
    if not (1 <= tau_min <= tau_max <= _lib.YIN_MAX_LAG):
        raise _lib.TT2Error(f"{who}: lags must satisfy 1 <= tau_min <= tau_max <= {_lib.YIN_MAX_LAG}")
    if T > _lib.PITCH_TRACK_MAX_FRAMES:
        raise _lib.TT2Error(f"{who}: {T} frames exceed {_lib.PITCH_TRACK_MAX_FRAMES}")
    if width < tau_max + 1:
        raise _lib.TT2Error(f"{who}: cmnd rows hold {width} values, fewer than tau_max + 1")
    ld = _ld(cmnd)
    if ld < width or (B > 1 and T > 0 and cmnd.stride(0) != T * ld):
        raise _lib.TT2Error(f"{who}: cmnd's rows must follow one another (stride(0) = T * stride(1) >= ld)")
    _vec(who, "f0", f0, B * T, torch.float32)
    _vec(who, "lag", lag, B * T, torch.int32)
    _vec(who, "cost", cost, B, torch.float32)
    _vec(who, "pos", pos, tau_max + 1, torch.float32)
    _vec(who, "frames", frames, B, torch.int32)
    _same_gpu(who, (cmnd, f0, lag, cost, pos, frames))
    g = _lib.PitchTrackArgs()
    g.cmnd, g.frames, g.pos = cmnd.data_ptr(), ptr(frames), pos.data_ptr()
    g.f0, g.lag, g.cost = f0.data_ptr(), lag.data_ptr(), cost.data_ptr()
    g.cmnd_ld = ld
    g.batch, g.t, g.tau_min, g.tau_max = B, T, tau_min, tau_max
    g.sr, g.jump, g.switch_cost, g.unvoiced = float(sr), float(jump), float(switch), float(unvoiced)
    L = lib()
    _bind_workspace(g, L.tt2_pitch_track_workspace_size(B, T, tau_min, tau_max), ws)
    check(L.tt2_pitch_track(C.byref(g), stream_ptr()), "tt2_pitch_track")
    return f0, lag, cost


def resample(x, y, bank, up, down, half, lens=None, out_lens=None):
    """Polyphase sample-rate conversion (tt2_resample_args): x [B, n_in] f32 -> y [B, n_out] f32 by
    the factor up / down with bank [up, >= 2 * half + 1] f32 (row r: the taps of the outputs
    n = r mod up).  x, y and bank are 2-D with a contiguous last dim (row views are fine).  lens [B]
    int32 bounds the valid samples of each utterance (None: n_in); out_lens [B] int32, when given,
    receives min(ceil(len * up / down), n_out).  Outputs past that are 0.  On the current stream, no
    host synchronisation.  Deterministic."""
    who = "resample"
    up, down, half = int(up), int(down), int(half)
    if not (1 <= up <= _lib.RESAMPLE_MAX_PHASES) or down < 1:
        raise _lib.TT2Error(f"{who}: 1 <= up <= {_lib.RESAMPLE_MAX_PHASES} and down >= 1, got {up} / {down}")
    K = 2 * half + 1
    if half < 0 or K > _lib.RESAMPLE_MAX_TAPS:
        raise _lib.TT2Error(f"{who}: 2 * half + 1 = {K} taps outside 1 .. {_lib.RESAMPLE_MAX_TAPS}")
    y_ld = _rows(who, "y", y, torch.float32)
    B, n_out = y.shape
    x_ld = _rows(who, "x", x, torch.float32, rows=B)
    n_in = x.shape[1]
    bank_ld = _rows(who, "bank", bank, torch.float32, rows=up, min_cols=K)
    _vec(who, "lens", lens, B, torch.int32)
    _vec(who, "out_lens", out_lens, B, torch.int32)
    _same_gpu(who, (y, x, bank, lens, out_lens))
    g = _lib.ResampleArgs()
    g.x, g.lens, g.bank, g.y, g.out_lens = x.data_ptr(), ptr(lens), bank.data_ptr(), y.data_ptr(), ptr(out_lens)
    g.x_ld, g.y_ld, g.bank_ld = x_ld, y_ld, bank_ld
    g.batch, g.n_in, g.n_out, g.up, g.down, g.half = B, n_in, n_out, up, down, half
    check(lib().tt2_resample(C.byref(g), stream_ptr()), "tt2_resample")
    return y, out_lens


def trim(x, y, hop, r, keep, ratio, lens=None, out_lens=None, start=None, energy=None, workspace=None):
    """Leading / trailing silence trimming (tt2_trim_args): x [B, n_in] f32 -> y [B, n_out] f32, with
    y[b, i] = x[b, start_b + i] for i < out_b and 0 after, where [start_b, end_b) runs from `keep`
    samples before the first to `keep` samples after the last frame (length 2 * r * hop, hop `hop`,
    centred, zero-padded) whose energy exceeds ratio times the utterance's loudest frame's.  x and y
    are 2-D with a contiguous last dim (row views are fine).  lens [B] int32 bounds the valid samples
    (None: n_in); out_lens [B] int32 and start [B] int32, when given, receive min(end_b - start_b,
    n_out) and start_b; energy [B, >= n_in // hop + 1] f32, when given, the frame energies.
    workspace: a Workspace (default: the module's).  On the current stream, no host
    synchronisation.  Deterministic."""
    who = "trim"
    hop, r, keep, ratio = int(hop), int(r), int(keep), float(ratio)
    if hop < 1 or not (1 <= r <= _lib.TRIM_MAX_R) or 2 * r * hop > 2 ** 31 - 1:
        raise _lib.TT2Error(f"{who}: hop >= 1, 1 <= r <= {_lib.TRIM_MAX_R} and 2 * r * hop within int32, got {hop}, {r}")
    if keep < 0 or not (0.0 <= ratio <= 1.0):
        raise _lib.TT2Error(f"{who}: keep >= 0 and 0 <= ratio <= 1, got {keep}, {ratio}")
    y_ld = _rows(who, "y", y, torch.float32)
    B, n_out = y.shape
    x_ld = _rows(who, "x", x, torch.float32, rows=B)
    n_in = x.shape[1]
    energy_ld = 0 if energy is None else _rows(who, "energy", energy, torch.float32, rows=B, min_cols=n_in // hop + 1)
    for name, t in (("lens", lens), ("out_lens", out_lens), ("start", start)):
        _vec(who, name, t, B, torch.int32)
    _same_gpu(who, (y, x, energy, lens, out_lens, start))
    g = _lib.TrimArgs()
    g.x, g.lens, g.y = x.data_ptr(), ptr(lens), y.data_ptr()
    g.out_lens, g.start, g.energy = ptr(out_lens), ptr(start), ptr(energy)
    g.x_ld, g.y_ld, g.energy_ld = x_ld, y_ld, energy_ld
    g.batch, g.n_in, g.n_out, g.hop, g.r, g.keep, g.ratio = B, n_in, n_out, hop, r, keep, ratio
    L = lib()
    _bind_workspace(g, L.tt2_trim_workspace_size(B, n_in, hop), workspace)
    check(L.tt2_trim(C.byref(g), stream_ptr()), "tt2_trim")
    return y, out_lens, start, energy


def loudness(x, step, coef, abs_sum, rel_ratio, target_ms, ceiling, lens=None, y=None, loud=None, gain=None,
             peak=None, limited=None, energy=None, workspace=None):
    """Gated integrated loudness and gain (tt2_loudness_args; include/tt2_capi.h has the definition):
    x [B, n_in] f32 through the two biquads of coef (ten floats: b0 b1 b2 a1 a2 of each section),
    sub-block energies of `step` samples, blocks of four, the absolute gate abs_sum (a block's sum of
    squares) and the relative gate rel_ratio, the gain min(sqrt(target_ms / ms), ceiling / peak).
    Every output is optional, at least one is required: y [B, n_out] f32 = gain * x (zeros past the
    utterance), loud / gain / peak [B] f32, limited [B] int32, energy [B, >= n_in // step + 1] f32.  x, y
    and energy are 2-D with a contiguous last dim (row views are fine).  lens [B] int32 bounds the
    valid samples (None: n_in).  workspace: a Workspace (default: the module's).  On the current
    stream, no host synchronisation.  Deterministic."""
    import math
    who = "loudness"
    step = int(step)
    coef = [float(c) for c in coef]
    abs_sum, rel_ratio, target_ms, ceiling = float(abs_sum), float(rel_ratio), float(target_ms), float(ceiling)
    if step < 1 or 4 * step > 2 ** 31 - 1:
        raise _lib.TT2Error(f"{who}: step >= 1 and 4 * step within int32, got {step}")
    if len(coef) != 10 or not all(math.isfinite(c) for c in coef):
        raise _lib.TT2Error(f"{who}: coef must be ten finite numbers")
    if not (math.isfinite(abs_sum) and abs_sum >= 0.0) or not (0.0 <= rel_ratio <= 1.0):
        raise _lib.TT2Error(f"{who}: abs_sum finite and >= 0 and 0 <= rel_ratio <= 1, got {abs_sum}, {rel_ratio}")
    if not (math.isfinite(target_ms) and target_ms > 0.0 and math.isfinite(ceiling) and ceiling > 0.0):
        raise _lib.TT2Error(f"{who}: target_ms and ceiling finite and > 0, got {target_ms}, {ceiling}")
    outputs = (y, loud, gain, peak, limited, energy)
    if all(t is None for t in outputs):
        raise _lib.TT2Error(f"{who}: at least one output is required")
    x_ld = _rows(who, "x", x, torch.float32)
    B, n_in = x.shape
    y_ld = 0 if y is None else _rows(who, "y", y, torch.float32, rows=B)
    n_out = y.shape[1] if y is not None else 0
    energy_ld = 0 if energy is None else _rows(who, "energy", energy, torch.float32, rows=B, min_cols=n_in // step + 1)
    for name, t in (("loud", loud), ("gain", gain), ("peak", peak)):
        _vec(who, name, t, B, torch.float32)
    _vec(who, "limited", limited, B, torch.int32)
    _vec(who, "lens", lens, B, torch.int32)
    _same_gpu(who, (x, lens) + outputs)
    g = _lib.LoudnessArgs()
    g.x, g.lens, g.y = x.data_ptr(), ptr(lens), ptr(y)
    g.loud, g.gain, g.peak, g.limited, g.energy = ptr(loud), ptr(gain), ptr(peak), ptr(limited), ptr(energy)
    g.x_ld, g.y_ld, g.energy_ld = x_ld, y_ld, energy_ld
    g.batch, g.n_in, g.n_out, g.step = B, n_in, n_out, step
    g.coef = (C.c_double * 10)(*coef)
    g.abs_sum, g.rel_ratio, g.target_ms, g.ceiling = abs_sum, rel_ratio, target_ms, ceiling
    L = lib()
    _bind_workspace(g, L.tt2_loudness_workspace_size(B, n_in, step), workspace)
    check(L.tt2_loudness(C.byref(g), stream_ptr()), "tt2_loudness")
    return y, loud, gain, peak, limited, energy


def regulate_plan(durations, n_out, key_len=None, ends=None, index=None, frames=None, total=None):
    """The plan of a length regulator (tt2_regulate_plan_args; include/tt2_capi.h has the definition):
    durations [B, Tx] int32 (negatives count as 0; entries at and past key_len[b] are not read) ->
    ends [B, Tx] int32 = min(cumsum, n_out), index [B, n_out] int32 (the phoneme of each frame, -1 past
    the utterance's frames), frames [B] = ends[:, -1] and total [B] = the unclamped sum (up to 2^31 - 1).
    ends is required and written for every column; index, frames and total are written where given.
    2-D tensors need a contiguous last dim (row views are fine).  On the current stream, no host
    synchronisation.  Deterministic."""
    who = "regulate_plan"
    n_out = int(n_out)
    dur_ld = _rows(who, "durations", durations, torch.int32, err=ValueError)
    B, tx = durations.shape
    if tx > _lib.REGULATE_MAX_PHONEMES:
        raise ValueError(f"{who}: Tx = {tx} above TT2_REGULATE_MAX_PHONEMES = {_lib.REGULATE_MAX_PHONEMES}")
    if not (0 <= n_out <= 2 ** 31 - 1):
        raise ValueError(f"{who}: n_out must be in [0, 2^31 - 1], got {n_out}")
    if ends is None:
        raise ValueError(f"{who}: ends is required")
    g = _lib.RegulatePlanArgs()
    g.dur_ld = dur_ld
    g.ends_ld = _rows(who, "ends", ends, torch.int32, rows=B, min_cols=tx, err=ValueError)
    if index is not None:
        g.index_ld = _rows(who, "index", index, torch.int32, rows=B, min_cols=n_out, err=ValueError)
    for name, t in (("key_len", key_len), ("frames", frames), ("total", total)):
        _vec(who, name, t, B, torch.int32, exact=True, err=ValueError)
    _same_gpu(who, (durations, ends, index, key_len, frames, total), err=ValueError)
    g.durations, g.key_len, g.ends, g.index = durations.data_ptr(), ptr(key_len), ends.data_ptr(), ptr(index)
    g.frames, g.total = ptr(frames), ptr(total)
    g.batch, g.tx, g.n_out = B, tx, n_out
    check(lib().tt2_regulate_plan(C.byref(g), stream_ptr()), "tt2_regulate_plan")
    return ends, index, frames, total


def _regulate_args(who, src, dst, map_, map_cols):
    for name, t in (("src", src), ("dst", dst)):
        if t.dim() != 3 or t.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"{who}: {name} must be f32 or bf16 [B, rows, D], got {t.dtype} {tuple(t.shape)}")
    if src.dtype != dst.dtype:
        raise ValueError(f"{who}: src is {src.dtype}, dst {dst.dtype}")
    B, D = dst.shape[0], dst.shape[2]
    if src.shape[0] != B or src.shape[2] != D:
        raise ValueError(f"{who}: src is {tuple(src.shape)}, dst {tuple(dst.shape)}")
    g = _lib.RegulateArgs()
    strides = []
    for name, t in (("src", src), ("dst", dst)):
        if D > 1 and t.stride(2) != 1:
            raise ValueError(f"{who}: {name} needs a contiguous last dim")
        ld = _ld(t)
        bs = t.stride(0) if B > 1 else max(t.stride(0), 0)
        if ld < D or (name == "dst" and B > 1 and t.shape[1] > 0 and bs < (t.shape[1] - 1) * ld + D):
            raise ValueError(f"{who}: {name}'s rows overlap (strides {t.stride()} for {tuple(t.shape)})")
        strides += [ld, bs]
    g.src_ld, g.src_bs, g.dst_ld, g.dst_bs = strides
    g.map_ld = _rows(who, "map", map_, torch.int32, rows=B, min_cols=map_cols, err=ValueError)
    _same_gpu(who, (dst, src, map_), err=ValueError)
    g.src, g.dst, g.map = src.data_ptr(), dst.data_ptr(), map_.data_ptr()
    g.batch, g.dim, g.dtype = B, D, dt(dst)
    return g


def regulate_fwd(h, index, y):
    """The expansion of a length regulator (tt2_regulate_fwd): y[b, n, :] = h[b, index[b, n], :], the
    bits copied, and +0 where index[b, n] is outside [0, Tx).  h [B, Tx, D] and y [B, n_out, D], both
    f32 or both bf16, may be slices of wider buffers (any row and batch stride, a contiguous last
    dim); index [B, >= n_out] int32 as regulate_plan writes it.  On the current stream, no host
    synchronisation.  Deterministic."""
    who = "regulate_fwd"
    if h.dim() == 3 and h.shape[1] > _lib.REGULATE_MAX_PHONEMES:
        raise ValueError(f"{who}: Tx = {h.shape[1]} above TT2_REGULATE_MAX_PHONEMES = {_lib.REGULATE_MAX_PHONEMES}")
    g = _regulate_args(who, h, y, index, y.shape[1] if y.dim() == 3 else 0)
    g.tx, g.n_out = h.shape[1], y.shape[1]
    check(lib().tt2_regulate_fwd(C.byref(g), stream_ptr()), "tt2_regulate_fwd")
    return y


def regulate_bwd(dy, ends, dh):
    """The segment sum of a length regulator (tt2_regulate_bwd), the gradient of regulate_fwd in h:
    dh[b, t, :] = the sum of dy[b, n, :] over ends[b, t-1] <= n < ends[b, t] (ends clamped to
    [0, n_out], 0 before t = 0), added in f32 in ascending n and rounded once to dh's dtype; +0 for an
    empty segment.  dy [B, n_out, D] and dh [B, Tx, D], both f32 or both bf16, may be slices of wider
    buffers; ends [B, >= Tx] int32 as regulate_plan writes it.  A phoneme's sum is serial in its
    duration.  On the current stream, no host synchronisation.  Deterministic."""
    who = "regulate_bwd"
    if dh.dim() == 3 and dh.shape[1] > _lib.REGULATE_MAX_PHONEMES:
        raise ValueError(f"{who}: Tx = {dh.shape[1]} above TT2_REGULATE_MAX_PHONEMES = {_lib.REGULATE_MAX_PHONEMES}")
    g = _regulate_args(who, dy, dh, ends, dh.shape[1] if dh.dim() == 3 else 0)
    g.tx, g.n_out = dh.shape[1], dy.shape[1]
    check(lib().tt2_regulate_bwd(C.byref(g), stream_ptr()), "tt2_regulate_bwd")
    return dh


def _fsum_mat(who, name, t, B, tq, tk, out=False):
    """Check that t is f32 [B, tq, tk] with a contiguous last dim (any row and batch stride; an output's
    rows and utterances must not overlap); returns (ld, bs) in elements."""
    if t.dtype != torch.float32 or t.dim() != 3 or (t.shape[2] > 1 and t.stride(2) != 1):
        raise ValueError(f"{who}: {name} must be f32 [B, Ty, Tx] with a contiguous last dim, "
                         f"got {t.dtype} {tuple(t.shape)} of strides {t.stride()}")
    if B is not None and tuple(t.shape) != (B, tq, tk):
        raise ValueError(f"{who}: {name} is {tuple(t.shape)}, the scores are [{B}, {tq}, {tk}]")
    ld = _ld(t)
    bs = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), 0)
    if ld < t.shape[2] or (out and t.shape[0] > 1 and t.shape[1] > 0 and bs < (t.shape[1] - 1) * ld + t.shape[2]):
        raise ValueError(f"{who}: {name}'s rows overlap (strides {t.stride()} for {tuple(t.shape)})")
    return ld, bs


def _fsum_args(who, scores, q_len, key_len):
    g = _lib.ForwardSumArgs()
    g.s_ld, g.s_bs = _fsum_mat(who, "scores", scores, None, 0, 0)
    B, tq, tk = scores.shape
    if tk > _lib.FSUM_MAX_KEYS or tq > _lib.FSUM_MAX_FRAMES:
        raise ValueError(f"{who}: [Ty, Tx] = [{tq}, {tk}] above TT2_FSUM_MAX_FRAMES = {_lib.FSUM_MAX_FRAMES} / "
                         f"TT2_FSUM_MAX_KEYS = {_lib.FSUM_MAX_KEYS}")
    for name, t in (("q_len", q_len), ("key_len", key_len)):
        _vec(who, name, t, B, torch.int32, exact=True, err=ValueError)
    g.scores, g.q_len, g.key_len = scores.data_ptr(), ptr(q_len), ptr(key_len)
    g.batch, g.tq, g.tk = B, tq, tk
    return g


def _fsum_alpha(who, g, alpha):
    B, tq, tk = g.batch, g.tq, g.tk
    if alpha.dtype != torch.float32 or alpha.dim() != 3 or alpha.shape[:2] != (B, tq) or alpha.shape[2] < tk or \
            not alpha.is_contiguous():
        raise ValueError(f"{who}: alpha must be a contiguous f32 [{B}, {tq}, >= {tk}], got {alpha.dtype} {tuple(alpha.shape)}")
    g.alpha, g.a_ld = alpha.data_ptr(), max(alpha.shape[2], tk)


def forward_sum_fwd(scores, loss, lse, alpha=None, q_len=None, key_len=None):
    """The forward-sum alignment loss (tt2_forward_sum_fwd; include/tt2_capi.h has the definition):
    scores [B, Ty, Tx] f32 (any row and batch stride, a contiguous last dim) -> loss [B] f32 = -ln Z
    in nats, lse [B, Ty] f32 (the row log-sum-exps) and, when given, alpha [B, Ty, >= Tx] f32, the
    renormalised forward variable that forward_sum_bwd reads.  q_len / key_len [B] int32 bound the
    frames / phonemes of each utterance (None: Ty / Tx).  On the current stream, no host
    synchronisation.  Deterministic."""
    who = "forward_sum_fwd"
    g = _fsum_args(who, scores, q_len, key_len)
    _vec(who, "loss", loss, g.batch, torch.float32, exact=True, err=ValueError)
    if lse is None or loss is None:
        raise ValueError(f"{who}: loss and lse are required")
    if lse.dtype != torch.float32 or tuple(lse.shape) != (g.batch, g.tq) or not lse.is_contiguous():
        raise ValueError(f"{who}: lse must be a contiguous f32 [{g.batch}, {g.tq}], got {lse.dtype} {tuple(lse.shape)}")
    if alpha is not None:
        _fsum_alpha(who, g, alpha)
    _same_gpu(who, (scores, loss, lse, alpha, q_len, key_len), err=ValueError)
    g.loss, g.lse = loss.data_ptr(), lse.data_ptr()
    check(lib().tt2_forward_sum_fwd(C.byref(g), stream_ptr()), "tt2_forward_sum_fwd")
    return loss, lse, alpha


def forward_sum_bwd(scores, lse, alpha, dscores=None, gamma=None, grad_loss=None, q_len=None, key_len=None,
                    workspace=None):
    """The gradient and posterior of the forward-sum loss (tt2_forward_sum_bwd): with scores, lse and
    alpha as forward_sum_fwd left them, dscores [B, Ty, Tx] f32 = grad_loss[b] * (softmax(scores) -
    gamma) and gamma [B, Ty, Tx] f32 = P(pi(n) = t), both exactly 0 in the padding; either may be
    None, not both, and both may be slices of wider buffers.  grad_loss [B] f32 on the device (None:
    1).  workspace: a Workspace (default: the module's).  On the current stream, no host
    synchronisation.  Deterministic."""
    who = "forward_sum_bwd"
    g = _fsum_args(who, scores, q_len, key_len)
    B, tq, tk = g.batch, g.tq, g.tk
    if dscores is None and gamma is None:
        raise ValueError(f"{who}: dscores or gamma is required")
    if lse is None or alpha is None:
        raise ValueError(f"{who}: lse and alpha are required")
    if lse.dtype != torch.float32 or tuple(lse.shape) != (B, tq) or not lse.is_contiguous():
        raise ValueError(f"{who}: lse must be a contiguous f32 [{B}, {tq}], got {lse.dtype} {tuple(lse.shape)}")
    _fsum_alpha(who, g, alpha)
    if dscores is not None:
        g.d_ld, g.d_bs = _fsum_mat(who, "dscores", dscores, B, tq, tk, out=True)
    if gamma is not None:
        g.g_ld, g.g_bs = _fsum_mat(who, "gamma", gamma, B, tq, tk, out=True)
    _vec(who, "grad_loss", grad_loss, B, torch.float32, exact=True, err=ValueError)
    _same_gpu(who, (scores, lse, alpha, dscores, gamma, grad_loss, q_len, key_len), err=ValueError)
    g.lse, g.grad_loss, g.dscores, g.gamma = lse.data_ptr(), ptr(grad_loss), ptr(dscores), ptr(gamma)
    L = lib()
    _bind_workspace(g, L.tt2_forward_sum_bwd_workspace_size(B, tq, tk), workspace)
    check(L.tt2_forward_sum_bwd(C.byref(g), stream_ptr()), "tt2_forward_sum_bwd")
    return dscores, gamma


def forward_sum_path(scores, path, durations, logp, q_len=None, key_len=None, workspace=None):
    """The best monotone path of a score matrix (tt2_forward_sum_path), the binarisation of the
    forward-sum alignment: scores [B, Ty, Tx] f32 -> path [B, Ty] int32 (-1 past the utterance),
    durations [B, Tx] int32 and logp [B] f32, the mean log-softmax along the path; the conventions are
    align_monotonic's.  workspace: a Workspace (default: the module's).  On the current stream, no
    host synchronisation.  Deterministic."""
    who = "forward_sum_path"
    g = _fsum_args(who, scores, q_len, key_len)
    B, tq, tk = g.batch, g.tq, g.tk
    for name, t, n in (("path", path, tq), ("durations", durations, tk)):
        if t is None or t.dtype != torch.int32 or tuple(t.shape) != (B, n) or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous int32 [{B}, {n}]")
    if logp is None:
        raise ValueError(f"{who}: logp is required")
    _vec(who, "logp", logp, B, torch.float32, exact=True, err=ValueError)
    _same_gpu(who, (scores, path, durations, logp, q_len, key_len), err=ValueError)
    g.path, g.durations, g.logp = path.data_ptr(), durations.data_ptr(), logp.data_ptr()
    L = lib()
    _bind_workspace(g, L.tt2_forward_sum_path_workspace_size(B, tq, tk), workspace)
    check(L.tt2_forward_sum_path(C.byref(g), stream_ptr()), "tt2_forward_sum_path")
    return path, durations, logp


def _gu_mat(who, name, t, B, rows, D, dtype, out=False):
    """Check that t is [B, rows, D] of `dtype` with a contiguous last dim (any row and batch stride; an
    output's rows and utterances must not overlap); returns (ld, bs) in elements."""
    if t.dim() != 3 or t.dtype != dtype or tuple(t.shape) != (B, rows, D):
        raise ValueError(f"{who}: {name} must be {dtype} [{B}, {rows}, {D}], got {t.dtype} {tuple(t.shape)}")
    if D > 1 and t.stride(2) != 1:
        raise ValueError(f"{who}: {name} needs a contiguous last dim")
    ld = _ld(t)
    bs = t.stride(0) if B > 1 else max(t.stride(0), 0)
    if ld < D or (out and B > 1 and rows > 0 and bs < (rows - 1) * ld + D):
        raise ValueError(f"{who}: {name}'s rows overlap (strides {t.stride()} for {tuple(t.shape)})")
    return ld, bs


def _gu_args(who, h, center, prec, bias, y, lse, q_len, key_len, offset, vectors=()):
    """The part of tt2_gauss_upsample_args that forward and backward share.  vectors: further
    (name, tensor | None) per-phoneme f32 [B, >= Tx] tensors (the gradients), which must share the row
    stride of center."""
    if h is None or y is None or h.dim() != 3 or y.dim() != 3 or h.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{who}: h and y must be f32 or bf16 [B, rows, D]")
    B, tx, D = h.shape
    n_out = y.shape[1]
    if tx > _lib.REGULATE_MAX_PHONEMES:
        raise ValueError(f"{who}: Tx = {tx} above TT2_REGULATE_MAX_PHONEMES = {_lib.REGULATE_MAX_PHONEMES}")
    if D > _lib.UPSAMPLE_MAX_DIM:
        raise ValueError(f"{who}: dim = {D} above TT2_UPSAMPLE_MAX_DIM = {_lib.UPSAMPLE_MAX_DIM}")
    offset = float(offset)
    if not (0.0 <= offset < float("inf")):
        raise ValueError(f"{who}: offset must be finite and >= 0, got {offset}")
    g = _lib.GaussUpsampleArgs()
    g.h_ld, g.h_bs = _gu_mat(who, "h", h, B, tx, D, h.dtype)
    g.y_ld, g.y_bs = _gu_mat(who, "y", y, B, n_out, D, h.dtype, out=True)
    if center is None or prec is None or lse is None:
        raise ValueError(f"{who}: center, prec and lse are required")
    g.p_ld = _rows(who, "center", center, torch.float32, rows=B, min_cols=tx, err=ValueError)
    for name, t in (("prec", prec), ("bias", bias)) + tuple(vectors):
        if t is not None and _rows(who, name, t, torch.float32, rows=B, min_cols=tx, err=ValueError) != g.p_ld:
            raise ValueError(f"{who}: {name} must have center's row stride ({g.p_ld})")
    g.lse_ld = _rows(who, "lse", lse, torch.float32, rows=B, min_cols=n_out, err=ValueError)
    for name, t in (("q_len", q_len), ("key_len", key_len)):
        _vec(who, name, t, B, torch.int32, exact=True, err=ValueError)
    g.h, g.center, g.prec, g.bias = h.data_ptr(), center.data_ptr(), prec.data_ptr(), ptr(bias)
    g.y, g.lse, g.q_len, g.key_len = y.data_ptr(), lse.data_ptr(), ptr(q_len), ptr(key_len)
    g.batch, g.tx, g.n_out, g.dim, g.dtype, g.offset = B, tx, n_out, D, dt(h), offset
    return g


def gauss_upsample_fwd(h, center, prec, y, lse, bias=None, q_len=None, key_len=None, offset=0.0):
    """Gaussian upsampling (tt2_gauss_upsample_fwd; include/tt2_capi.h has the definition):
    y[b, n, :] = sum_t W[n, t] h[b, t, :] with W[n, .] = softmax_t(bias[t] - prec[t] (n + offset -
    center[t])^2) over t < key_len[b], and lse[b, n] its log-sum-exp; rows at and past q_len[b] are +0.
    h [B, Tx, D] and y [B, n_out, D], both f32 or both bf16, may be slices of wider buffers; center,
    prec and bias (optional) f32 [B, >= Tx] of one row stride; lse f32 [B, >= n_out]; q_len / key_len
    [B] int32 (None: n_out / Tx).  On the current stream, no host synchronisation.  Deterministic."""
    who = "gauss_upsample_fwd"
    g = _gu_args(who, h, center, prec, bias, y, lse, q_len, key_len, offset)
    _same_gpu(who, (h, center, prec, bias, y, lse, q_len, key_len), err=ValueError)
    check(lib().tt2_gauss_upsample_fwd(C.byref(g), stream_ptr()), "tt2_gauss_upsample_fwd")
    return y, lse


def gauss_upsample_bwd(h, center, prec, y, lse, dy, dh=None, dcenter=None, dprec=None, dbias=None, bias=None,
                       q_len=None, key_len=None, offset=0.0, workspace=None):
    """The gradients of gauss_upsample_fwd (tt2_gauss_upsample_bwd) from dy [B, n_out, D] and the y and
    lse the forward left: dh [B, Tx, D] (h's dtype), dcenter, dprec and dbias f32 [B, >= Tx] of center's
    row stride, each optional (at least one), each +0 at and past key_len[b] and the same bits
    whichever others are asked for.  workspace: a Workspace (default: the module's).  On the current
    stream, no host synchronisation.  Deterministic."""
    who = "gauss_upsample_bwd"
    if dh is None and dcenter is None and dprec is None and dbias is None:
        raise ValueError(f"{who}: one of dh, dcenter, dprec and dbias is required")
    g = _gu_args(who, h, center, prec, bias, y, lse, q_len, key_len, offset,
                 vectors=(("dcenter", dcenter), ("dprec", dprec), ("dbias", dbias)))
    B, tx, n_out, D = g.batch, g.tx, g.n_out, g.dim
    if dy is None:
        raise ValueError(f"{who}: dy is required")
    g.dy_ld, g.dy_bs = _gu_mat(who, "dy", dy, B, n_out, D, h.dtype)
    if dh is not None:
        g.dh_ld, g.dh_bs = _gu_mat(who, "dh", dh, B, tx, D, h.dtype, out=True)
    _same_gpu(who, (h, center, prec, bias, y, lse, dy, dh, dcenter, dprec, dbias, q_len, key_len), err=ValueError)
    g.dy, g.dh, g.dcenter, g.dprec, g.dbias = dy.data_ptr(), ptr(dh), ptr(dcenter), ptr(dprec), ptr(dbias)
    L = lib()
    _bind_workspace(g, L.tt2_gauss_upsample_bwd_workspace_size(B, tx, n_out, D), workspace)
    check(L.tt2_gauss_upsample_bwd(C.byref(g), stream_ptr()), "tt2_gauss_upsample_bwd")
    return dh, dcenter, dprec, dbias


def _drop_into(s, drop: Drop):
    s.drop_seed, s.drop_site, s.drop_thr, s.drop_scale = drop.fields()


def colsum(x, ld, m, n, dst, beta=0.0, ws: Workspace | None = None):
    """dst[n] (f32) = beta*dst + sum over m rows of x[:, :n]  (bias gradient)."""
    L = lib()
    buf = (ws or _WS).get(L.tt2_colsum_workspace_size(m, n))
    check(L.tt2_colsum(x.data_ptr(), dt(x), ld, m, n, dst.data_ptr(), beta, buf.data_ptr(), buf.numel(),
                       stream_ptr()), "tt2_colsum")


def layernorm_fwd(x, branch, gamma, beta, y, mean, rstd, m, eps=1e-5, drop: Drop = NO_DROP):
    L = lib()
    a = _lib.LnArgs()
    a.x, a.branch, a.y = x.data_ptr(), ptr(branch), y.data_ptr()
    a.gamma, a.beta = gamma.data_ptr(), beta.data_ptr()
    a.mean, a.rstd = ptr(mean), ptr(rstd)
    a.m, a.c, a.dtype, a.eps = m, x.shape[-1], dt(x), eps
    _drop_into(a, drop)
    check(L.tt2_layernorm_fwd(C.byref(a), stream_ptr()), "tt2_layernorm_fwd")


def ln_combine(x, part, splits, bias, gamma, beta, y, m, eps=1e-5):
    """y = LN(x + bias + sum_s part[s]) (decode step; part = a skinny split-K GEMM's slabs)."""
    check(lib().tt2_ln_combine(x.data_ptr(), part.data_ptr(), splits, bias.data_ptr(), gamma.data_ptr(),
                               beta.data_ptr(), y.data_ptr(), m, x.shape[-1], eps, dt(x), stream_ptr()),
          "tt2_ln_combine")


def ffn_decode(x, w1, b1, w2, b2, gamma, beta, hidden, slab, sync, y, m, eps=1e-5, stamps=None):
    """The decode step's FFN sublayer in one launch (tt2_ffn_decode): y = LN(x + b2 + relu(x W1^T +
    b1) W2^T), hidden = relu(x W1^T + b1), slab = the 8 raw FFN2 partial slabs; sync: int32 [2048],
    zero before the first call (each call leaves it zero; sync[1088] != 0 flags a timed-out phase).
    stamps (int64 [256, 8], optional): per-work-group wall-clock stamps (tt2_ffn_decode_stamps)."""
    if sync.dtype != torch.int32 or sync.numel() < 2048:
        raise ValueError("ffn_decode: sync must be an int32 tensor of at least TT2_FFN_SYNC_INTS (2048) words")
    for t in (x, w1, w2, hidden, y, slab):
        if not t.is_contiguous():
            raise ValueError("ffn_decode: x, w1, w2, hidden, slab and y must be contiguous (packed rows)")
    a = _lib.FfnDecodeArgs()
    a.x, a.w1, a.b1, a.w2, a.b2 = x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    a.gamma, a.beta, a.hidden, a.slab = gamma.data_ptr(), beta.data_ptr(), hidden.data_ptr(), slab.data_ptr()
    a.sync, a.y = sync.data_ptr(), y.data_ptr()
    a.m, a.d_model, a.d_ffn, a.dtype, a.eps = m, x.shape[-1], w1.shape[0], dt(x), eps
    if stamps is None:
        check(lib().tt2_ffn_decode(C.byref(a), stream_ptr()), "tt2_ffn_decode")
    else:
        check(lib().tt2_ffn_decode_stamps(C.byref(a), stamps.data_ptr(), stream_ptr()), "tt2_ffn_decode")


def layernorm_bwd(dy, x, branch, gamma, mean, rstd, dx, dbranch, dgamma, dbeta, m, drop: Drop = NO_DROP,
                  ws: Workspace | None = None, dbias=None, part=None, defer=False, prev=None):
    """dx = d(LN)/ds, dbranch = drop-masked dx, gamma/beta grads, and optionally
    dbias = column sums of dbranch (the producing linear layer's bias gradient).

    defer=True leaves dgamma/dbeta/dbias as column partials in `part` (a dedicated uint8
    buffer that nothing else may touch until they are finalized); a later call with
    prev=<the returned args> completes them in its own launch, or layernorm_bwd_finalize
    does.  Returns the call's LnArgs."""
    L = lib()
    a = _lib.LnArgs()
    a.dy, a.x, a.branch = dy.data_ptr(), x.data_ptr(), ptr(branch)
    a.dx, a.dbranch = dx.data_ptr(), ptr(dbranch)
    a.dbias = ptr(dbias)
    a.gamma, a.mean, a.rstd = gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    a.dgamma, a.dbeta = dgamma.data_ptr(), dbeta.data_ptr()
    a.m, a.c, a.dtype = m, x.shape[-1], dt(x)
    _drop_into(a, drop)
    need = L.tt2_layernorm_bwd_workspace_size(C.byref(a))
    if defer and part is None:
        raise ValueError("layernorm_bwd: defer needs a dedicated partials buffer")
    buf = part if part is not None else (ws or _WS).get(need)
    if buf.numel() < need:
        raise ValueError(f"layernorm_bwd: partials buffer {buf.numel()} B < {need} B")
    a.workspace, a.ws_bytes = buf.data_ptr(), buf.numel()
    a.defer_finalize = int(defer)
    a.finalize_prev = C.addressof(prev) if prev is not None and prev.defer_finalize else None
    check(L.tt2_layernorm_bwd(C.byref(a), stream_ptr()), "tt2_layernorm_bwd")
    return a


def layernorm_bwd_workspace_size(m: int, c: int) -> int:
    a = _lib.LnArgs()
    a.m, a.c = m, c
    return lib().tt2_layernorm_bwd_workspace_size(C.byref(a))


def layernorm_bwd_finalize(a):
    """Completes a deferred layernorm_bwd (its returned LnArgs)."""
    check(lib().tt2_layernorm_bwd_finalize(C.byref(a), stream_ptr()), "tt2_layernorm_bwd_finalize")


def _bn(y, gamma, beta, mean, rstd, m, c, act, training, drop, eps, momentum, ws):
    a = _lib.BnArgs()
    a.y, a.gamma, a.beta, a.mean, a.rstd = y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), \
        rstd.data_ptr()
    a.m, a.c, a.act, a.dtype, a.training, a.eps, a.momentum = m, c, act, dt(y), int(training), eps, momentum
    _drop_into(a, drop)
    return a


def _bn_sync_into(L, a, sync):
    """SyncBatchNorm exchange buffer of `sync` (tt2/dist.py BnSync: world, rank, buffer(nbytes),
    exchange(tensor)) into the args; returns the slot view that exchange() all-reduces."""
    a.sync_world, a.sync_rank = sync.world, sync.rank
    buf = sync.buffer(L.tt2_batchnorm_sync_size(C.byref(a)))
    a.sync_buf = buf.data_ptr()
    return buf[:sync.world * 4 * a.c]


def batchnorm_fwd(y, gamma, beta, mean, rstd, run_mean, run_var, out, m, c, act, training, drop: Drop = NO_DROP,
                  res=None, res_ld=0, eps=1e-5, momentum=0.1, ws: Workspace | None = None, sync=None, stats=None):
    """sync (training only): SyncBatchNorm over the data-parallel ranks -- the statistics of
    all ranks' rows (tt2_batchnorm_fwd_stats, exchange, tt2_batchnorm_fwd_apply).
    stats = (buf, rows): y's column moments are already in buf, chunks of `rows` rows (the
    producing GEMM's col_stats), so the statistics pass over y is skipped (training only)."""
    L = lib()
    a = _bn(y, gamma, beta, mean, rstd, m, c, act, training, drop, eps, momentum, ws)
    a.run_mean, a.run_var = ptr(run_mean), ptr(run_var)
    a.out, a.out_dtype = out.data_ptr(), dt(out)
    a.res, a.res_dtype, a.res_ld = ptr(res), (dt(res) if res is not None else 0), res_ld
    if stats is not None and training:
        _bn_stats_into(L, a, stats)
    else:
        buf = (ws or _WS).get(L.tt2_batchnorm_workspace_size(C.byref(a)))
        a.workspace, a.ws_bytes = buf.data_ptr(), buf.numel()
    if sync is None or not training:
        check(L.tt2_batchnorm_fwd(C.byref(a), stream_ptr()), "tt2_batchnorm_fwd")
        return
    slots = _bn_sync_into(L, a, sync)
    check(L.tt2_batchnorm_fwd_stats(C.byref(a), stream_ptr()), "tt2_batchnorm_fwd_stats")
    sync.exchange(slots)
    check(L.tt2_batchnorm_fwd_apply(C.byref(a), stream_ptr()), "tt2_batchnorm_fwd_apply")


def _bn_stats_into(L, a, stats):
    sbuf, a.stats_rows = stats
    need = L.tt2_batchnorm_workspace_size(C.byref(a))
    if sbuf.dtype != torch.float32 or sbuf.numel() * 4 < need:
        raise _lib.TT2Error(f"batchnorm: stats buffer needs {need} bytes of f32")
    a.workspace, a.ws_bytes = sbuf.data_ptr(), sbuf.numel() * 4


def bn_bwd_args(y, gamma, beta, mean, rstd, m, c, act, drop: Drop, stats) -> _lib.BnArgs:
    """The BatchNorm backward whose column sums a GEMM producing its dout computes
    (gemm(..., bn_bwd=...)); stats = (buf, rows) as then given to batchnorm_bwd (rows:
    gemm_stats_rows of that GEMM)."""
    L = lib()
    a = _bn(y, gamma, beta, mean, rstd, m, c, act, True, drop, 1e-5, 0.1, None)
    _bn_stats_into(L, a, stats)
    return a


def batchnorm_bwd(y, dout, gamma, beta, mean, rstd, dy, dgamma, dbeta, m, c, act, drop: Drop = NO_DROP,
                  ws: Workspace | None = None, sync=None, stats=None):
    """sync: SyncBatchNorm backward (the column sums over all ranks' rows; dgamma / dbeta
    stay this rank's sums for the gradient all-reduce).
    stats = (buf, rows): the per-chunk column sums are already in buf (the GEMM that produced
    dout, gemm(..., bn_bwd=bn_bwd_args(...))), so the statistics pass is skipped."""
    L = lib()
    a = _bn(y, gamma, beta, mean, rstd, m, c, act, True, drop, 1e-5, 0.1, ws)
    a.dout, a.dout_dtype, a.dy = dout.data_ptr(), dt(dout), dy.data_ptr()
    a.dgamma, a.dbeta = dgamma.data_ptr(), dbeta.data_ptr()
    if stats is not None:
        _bn_stats_into(L, a, stats)
    else:
        buf = (ws or _WS).get(L.tt2_batchnorm_workspace_size(C.byref(a)))
        a.workspace, a.ws_bytes = buf.data_ptr(), buf.numel()
    if sync is None:
        check(L.tt2_batchnorm_bwd(C.byref(a), stream_ptr()), "tt2_batchnorm_bwd")
        return
    slots = _bn_sync_into(L, a, sync)
    check(L.tt2_batchnorm_bwd_stats(C.byref(a), stream_ptr()), "tt2_batchnorm_bwd_stats")
    sync.exchange(slots)
    check(L.tt2_batchnorm_bwd_apply(C.byref(a), stream_ptr()), "tt2_batchnorm_bwd_apply")


def embedding_fwd(ids, table, out, m, vocab):
    check(lib().tt2_embedding_fwd(ids.data_ptr(), table.data_ptr(), out.data_ptr(), m, table.shape[-1], vocab,
                                  dt(table), stream_ptr()), "tt2_embedding_fwd")


def embedding_bwd(ids, dout, dtable, m, vocab, pad_idx=0):
    check(lib().tt2_embedding_bwd(ids.data_ptr(), dout.data_ptr(), dtable.data_ptr(), m, dtable.shape[-1], vocab,
                                  pad_idx, dt(dout), stream_ptr()), "tt2_embedding_bwd")


def posenc_fwd(x, alpha, pe, out, m, t, drop: Drop = NO_DROP, t_offset=0, t_ptr=None):
    a = _lib.PeArgs()
    a.x, a.out, a.alpha, a.pe = x.data_ptr(), out.data_ptr(), alpha.data_ptr(), pe.data_ptr()
    a.t_ptr = ptr(t_ptr)
    a.m, a.c, a.t, a.t_offset, a.dtype = m, x.shape[-1], t, t_offset, dt(x)
    _drop_into(a, drop)
    check(lib().tt2_posenc_fwd(C.byref(a), stream_ptr()), "tt2_posenc_fwd")


def posenc_bwd(dout, pe, dx, dalpha, m, t, drop: Drop = NO_DROP, ws: Workspace | None = None):
    L = lib()
    a = _lib.PeArgs()
    a.dout, a.dx, a.pe, a.dalpha = dout.data_ptr(), dx.data_ptr(), pe.data_ptr(), dalpha.data_ptr()
    a.m, a.c, a.t, a.dtype = m, dout.shape[-1], t, dt(dout)
    _drop_into(a, drop)
    buf = (ws or _WS).get(L.tt2_posenc_bwd_workspace_size())
    a.workspace, a.ws_bytes = buf.data_ptr(), buf.numel()
    check(L.tt2_posenc_bwd(C.byref(a), stream_ptr()), "tt2_posenc_bwd")


def shift_right(mel, out, batch, t, c):
    check(lib().tt2_shift_right(mel.data_ptr(), out.data_ptr(), batch, t, c, dt(out), stream_ptr()),
          "tt2_shift_right")


def cast2d(src, src_ld, dst, dst_ld, m, n):
    check(lib().tt2_cast2d(src.data_ptr(), dt(src), src_ld, dst.data_ptr(), dt(dst), dst_ld, m, n, stream_ptr()),
          "tt2_cast2d")


def tts_loss(heads, heads_ld, mel_after, target, mel_len, loss_out, g_heads, g_after, batch, t, n_mels,
             pos_weight=5.0, grad_scale=1.0, ws: Workspace | None = None, separate_grads=False):
    L = lib()
    a = _lib.LossArgs()
    a.separate_grads = int(separate_grads)
    a.heads, a.mel_after, a.target, a.mel_len = heads.data_ptr(), mel_after.data_ptr(), target.data_ptr(), \
        mel_len.data_ptr()
    a.loss_out, a.g_heads, a.g_after = loss_out.data_ptr(), g_heads.data_ptr(), g_after.data_ptr()
    a.heads_ld, a.batch, a.t, a.n_mels, a.grad_dtype = heads_ld, batch, t, n_mels, dt(g_after)
    a.pos_weight, a.grad_scale = pos_weight, grad_scale
    buf = (ws or _WS).get(L.tt2_loss_workspace_size())
    a.workspace, a.ws_bytes = buf.data_ptr(), buf.numel()
    check(L.tt2_tts_loss(C.byref(a), stream_ptr()), "tt2_tts_loss")


def conv_weight_flip_batch(jobs):
    """One launch flipping every (w, wd, cout, cin, k) of `jobs` (<= 16; same dtype)."""
    if not jobs:
        return
    arr = (_lib.WflipJob * len(jobs))()
    for a, (w, wd, cout, cin, k) in zip(arr, jobs):
        a.w, a.wd, a.cout, a.cin, a.k = w.data_ptr(), wd.data_ptr(), cout, cin, k
    check(lib().tt2_conv_weight_flip_batch(arr, len(jobs), dt(jobs[0][0]), stream_ptr()),
          "tt2_conv_weight_flip_batch")


def conv_weight_flip(w, wd, cout, cin, k):
    check(lib().tt2_conv_weight_flip(w.data_ptr(), wd.data_ptr(), cout, cin, k, dt(w), stream_ptr()),
          "tt2_conv_weight_flip")


def sumsq_parts(g: torch.Tensor, parts: torch.Tensor, nparts: int):
    """parts[:nparts] = partial sums of g**2 (f32, fixed split), for adam_step(norm_parts=)."""
    check(lib().tt2_sumsq_parts(g.data_ptr(), g.numel(), parts.data_ptr(), nparts, stream_ptr()), "tt2_sumsq_parts")


def adam_step(params, grads, m, v, shadow, step, n, lr, beta1=0.9, beta2=0.98, eps=1e-9, weight_decay=0.0,
              clip_norm=1.0, warmup=4000.0, noam=True, d_model=512, ws: Workspace | None = None,
              norm_parts: torch.Tensor | None = None, gate: torch.Tensor | None = None):
    """norm_parts: the squared-norm partial sums of every gradient (sumsq_parts over ranges
    covering grads), so the clip needs no pass of its own over the gradients.
    gate: int32 device flag; the update runs only while it is non-zero (adam_gate)."""
    L = lib()
    a = _lib.AdamArgs()
    if norm_parts is not None:
        a.norm_parts, a.norm_nparts = norm_parts.data_ptr(), norm_parts.numel()
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr()
    a.shadow_bf16, a.step, a.n = ptr(shadow), step.data_ptr(), n
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = lr, beta1, beta2, eps, weight_decay
    a.clip_norm, a.warmup, a.noam, a.d_model = clip_norm, warmup, int(noam), d_model
    a.gate = ptr(gate)
    buf = (ws or _WS).get(L.tt2_adam_workspace_size())
    a.workspace, a.ws_bytes = buf.data_ptr(), buf.numel()
    check(L.tt2_adam_step(C.byref(a), stream_ptr()), "tt2_adam_step")


def step_bump(step, seed=None):
    check(lib().tt2_step_bump(ptr(step), ptr(seed), stream_ptr()), "tt2_step_bump")


def adam_gate(gate, step=None, arm: bool = False):
    """arm: gate = 1.  Otherwise (consume): if gate != 0, step += 1 and gate = 0."""
    check(lib().tt2_adam_gate(gate.data_ptr(), ptr(step), 1 if arm else 0, stream_ptr()), "tt2_adam_gate")


def attn_decode(q, k, v, out, q_ld, k_bstride, k_ld, v_bstride, v_ld, o_ld, batch, heads, tk, key_len=None,
                t_ptr=None, scale=0.125, stop_len=None, step=None, wo=None, wo_ld=0, slab=None, wq=None, wq_ld=0,
                bq=None, ln=None):
    """One query row per batch element over a key cache (see tt2_attn_decode_args).
    wo / slab: the fused output projection, slab[h, b, :] = o[b, h] @ wo[:, h*64:(h+1)*64]^T (f32).
    wq / bq: the fused query projection, q is then the projection input x and the head's
    query is x[b] @ wq[h*64:(h+1)*64]^T + bq[h*64:(h+1)*64].
    ln = (part, bias, gamma, beta, out, eps): with wq, the projection input row is first
    LN(q[b] + bias + sum of the 8 slabs part[s, b]) (as ln_combine), written to out[b]."""
    a = _lib.AttnDecodeArgs()
    a.wq, a.wq_ld, a.bq = ptr(wq), wq_ld, ptr(bq)
    if ln is not None:
        part, lb, lg, lbe, lo, eps = ln
        a.ln_part, a.ln_bias, a.ln_gamma, a.ln_beta, a.ln_out, a.ln_eps = ptr(part), ptr(lb), ptr(lg), ptr(lbe), \
            ptr(lo), eps
    a.stop_len, a.step = ptr(stop_len), ptr(step)
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), ptr(out)
    a.wo, a.wo_ld, a.slab = ptr(wo), wo_ld, ptr(slab)
    a.q_ld, a.k_bstride, a.k_ld, a.v_bstride, a.v_ld, a.o_ld = q_ld, k_bstride, k_ld, v_bstride, v_ld, o_ld
    a.key_len, a.t_ptr = ptr(key_len), ptr(t_ptr)
    a.batch, a.heads, a.head_dim, a.tk, a.dtype, a.scale = batch, heads, 64, tk, dt(q), scale
    check(lib().tt2_attn_decode(C.byref(a), stream_ptr()), "tt2_attn_decode")


def kv_append(src, src_ld, cache, c_bstride, c_ld, n, batch, t_ptr):
    check(lib().tt2_kv_append(src.data_ptr(), src_ld, cache.data_ptr(), c_bstride, c_ld, n, batch, t_ptr.data_ptr(),
                              dt(src), stream_ptr()), "tt2_kv_append")


def decode_emit(heads, heads_ld, batch, n_mels, t_max, mel_seq, stop_seq, prev, t_ptr, seed=None, stop_bias=None,
                stop_len=None, stop_thr=float("inf")):
    check(lib().tt2_decode_emit(heads.data_ptr(), heads_ld, batch, n_mels, t_max, mel_seq.data_ptr(),
                                stop_seq.data_ptr(), prev.data_ptr(), dt(prev), t_ptr.data_ptr(), ptr(seed),
                                ptr(stop_bias), ptr(stop_len), stop_thr, stream_ptr()), "tt2_decode_emit")
