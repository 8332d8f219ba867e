// gemm_common.h -- what the GEMM translation units (gemm*.hip) share.
//
//   C[m, n] = epi( alpha * sum_k A(m, k) * B(n, k) )
//
// One file per kernel family: gemm_v1.hip, gemm_skinny.hip, gemm_ffn_decode.hip, gemm_v8.hip and
// gemm_v10.hip are units of their own; v2, v7 (with the split-K reducers) and v11 are
// gemm_v2_impl.h, gemm_v7_impl.h and gemm_v11_impl.h, compiled as one unit (gemm_v2v7v11.hip says
// why).  Beside them the launch probe's state (gemm_probe.hip) and the host planner / dispatcher
// (gemm.hip).  A family keeps its kernels in an anonymous namespace and exports one host launcher
// (namespace tt2g, below) that owns its trans_a / trans_b ladder, so no unit refers to another
// unit's kernels (no relocatable device code).  Here: the
// operand / epilogue descriptors, the fused epilogue (scalar and 16-B vectorised) and the
// fixed-order split-K reduce body, the LDS-DMA helpers every LDS-DMA kernel uses (zero page,
// per-lane chunk source, swizzles, the 64-deep tile's fragment read), and the device side of the
// launch probe.
#pragma once
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdlib>

#include "tt2_common.h"
#include "tt2_capi.h"
#include "tt2_internal.h"

// Launch probe record width per work group: {start, end}; the in-step phase build (TT2_PHASE) adds
// s_memtime stamps (slot 2: entry; 3 + 2t / 4 + 2t: K step t's start / after its MFMAs,
// t < 12; 27..30: the epilogue's points, G7_STAMP; 31: the last wave's stores drained).
// The probe state and every probed kernel read it: a TT2_PHASE build recompiles all gemm*.hip.
#ifdef TT2_PHASE
#define TT2_SPAN_W 32
#else
#define TT2_SPAN_W 2
#endif

namespace tt2g {

// One operand and the epilogue of a request, as gemm_prep (gemm.hip) builds them.  The kernels
// take them as OpDesc / EpiParams (below).
struct Operand {
  const void* p;
  int64_t ld;
  int outer_max, inner_max;   // bounds of the outer (strided) and inner (contiguous) index
  int conv_t, conv_c, conv_pad;
};

struct Epilogue {
  void* c; int64_t ldc; int c_dt;
  const float* bias;
  const void* res; int64_t ldr; int res_dt;
  const void* gate; int64_t ldg; int gate_dt; float gate_scale;
  float alpha, beta;
  int act;
  DropDesc drop;
  int n_log;  // logical N for dropout index (m * n_log + n)
  int vec;    // every row of C/res/gate/bias is 16-B aligned at 8-column boundaries
  float* ksum; float ksum_beta;   // fused row sums of op(A) over k (v2, M-contiguous A)
  int main_only;                  // split-K: skip the reduce launch (measurement hook)
  float* cstats;                  // v7 LDS-image path: 256-row chunk column moments (tt2_gemm_args col_stats)
  // v7 LDS-image path: C is a BatchNorm backward's dout; its chunk sums of dpre, dpre * xhat go
  // to bnb.part (tt2_gemm_args bn_bwd)
  struct {
    const bf16* y; const float* mean; const float* rstd; const float* gamma; const float* beta;
    float* part;
    DropDesc drop;
    int act;
  } bnb;
};

// ---- gemm_probe.hip: the launch probe's thread-local state, reached only through these ----
// Consume the armed slot (-1: none armed): its event pair, and `groups` span records of the pool.
int probe_take(hipEvent_t& e0, hipEvent_t& e1, unsigned long long*& span, int groups);
// work groups per launch when one probed call goes out as consecutive launches
void probe_chunk(int slot, int wgs);
void probe_disarm();

// ---- per-family launchers (a_kc / b_kc: the operand is K-contiguous, i.e. !trans_a / !trans_b) ----
// gemm_v1.hip
hipError_t launch1(bool bf16_in, bool a_kc, bool b_kc, const Operand& A, const Operand& B, const Epilogue& E, int M,
                   int N, int K, int splits, float* ws, hipStream_t s);
// gemm_v2_impl.h
hipError_t launch2(bool a_kc, bool b_kc, const Operand& A, const Operand& B, const Epilogue& E, int M, int N, int K,
                   int splits, float* ws, hipStream_t s);
// gemm_v7_impl.h: the fixed-order split-K slab reduce + epilogue that follows a split main kernel
// (v1, v2, v7), and v7 itself
void launch_splitk_reduce(const float* ws, int splits, const Epilogue& E, int M, int N, hipStream_t s);
int splitk_blocks(int M, int N, const Epilogue& E);
// gemm_skinny.hip (reads the decode-step fusions from the request itself)
hipError_t launch_skinny(const tt2_gemm_args* a, const Epilogue& E, hipStream_t s);
hipError_t launch7(bool a_kc, bool b_kc, const Operand& A, const Operand& B, const Epilogue& E, int M, int N, int K,
                   int splits, float* ws, hipStream_t s, bool lds_epi);
// gemm_v8.hip
hipError_t launch8(bool b_kc, const Operand& A, const Operand& B, const Epilogue& E, int M, int N, int K,
                   hipStream_t s);
// gemm_v10.hip / gemm_v11_impl.h: the epilogue code of a request (-1: an option set the kernel does
// not fuse; vec: epi_vec_ok) and the launch of that code
int g10_code(const tt2_gemm_args* a, bool vec);
hipError_t launch10(const Operand& A, const Operand& B, const Epilogue& E, int M, int N, int K, int code,
                    hipStream_t s);
int g11_code(const tt2_gemm_args* a, bool vec);
hipError_t launch11(const Operand& A, const Operand& B, const Epilogue& E, int M, int N, int K, bool b_kc, int code,
                    hipStream_t s);

// ---- gemm.hip ----
// Validate one request and build its descriptors; the planner's choice (tt2_gemm_plan).
int gemm_prep(const tt2_gemm_args* a, Operand& A, Operand& B, Epilogue& ep);
int gemm_plan(const tt2_gemm_args* a);

}  // namespace tt2g

namespace {

// The kernels' parameter types.  Unit-local names (as the kernels themselves), so a kernel's
// symbol does not depend on which unit holds it.
struct OpDesc : tt2g::Operand {};
struct EpiParams : tt2g::Epilogue {};

constexpr int NT = 256;   // threads of the 4-wave kernels (v1, v2, skinny, ffn_decode)
constexpr int BM = 128, BN = 128;   // tile of v1 and v2

// Beside the probe's events, every probe-capable kernel records its own span on the device's
// constant-rate wall clock: each workgroup writes {its start, the end of its last wave after
// that wave's stores completed} to its own pair of a slot's record (plain stores, no shared
// address), and tt2_probe_span_ms takes the earliest start and the latest end.
TT2_DEV void span_begin(unsigned long long* span, int* done) {
  if (span && threadIdx.x == 0) {
    *done = 0;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // visible before the first barrier
    span[TT2_SPAN_W * blockIdx.x] = wall_clock64();
#ifdef TT2_PHASE
    span[TT2_SPAN_W * blockIdx.x + 2] = __builtin_amdgcn_s_memtime();
#endif
  }
}
// every wave once its own stores have completed (stores count in vmcnt on gfx9); the last
// wave of the workgroup to get here writes the end
TT2_DEV void span_end(unsigned long long* span, int* done, int waves) {
  if (span) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if ((threadIdx.x & 63) == 0 && atomicAdd(done, 1) == waves - 1) {
#ifdef TT2_PHASE
      span[TT2_SPAN_W * blockIdx.x + 31] = __builtin_amdgcn_s_memtime();
#endif
      span[TT2_SPAN_W * blockIdx.x + 1] = wall_clock64();
    }
  }
}

// The probe around one main-kernel launch.  Eager: the events ride in the kernel's own
// dispatch (hipExtLaunchKernelGGL, ext()) and the kernel records its span.  Under stream
// capture (a hipGraph of the step, bench.py's graph leg) only the span: nothing is added to
// the graph, and every replay re-records the launch's in-step duration.
struct ProbeScope {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  unsigned long long* span = nullptr;   // the kernel's own span record (the pool in gemm_probe.hip)
  int slot = -1;
  ProbeScope(hipStream_t s, int groups) {
    if ((slot = tt2g::probe_take(e0, e1, span, groups)) < 0) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive) e0 = e1 = nullptr;
    (void)hipGetLastError();
  }
  bool ext() const { return e0 != nullptr; }
  void chunk(int wgs) const { if (slot >= 0) tt2g::probe_chunk(slot, wgs); }
};

// An armed launch probe belongs to the next main GEMM launch of this call only: whatever
// path the call takes, it is disarmed on return (tt2_probe_ms then reports -1 for a slot
// no probe-capable kernel consumed).
struct ProbeDisarm {
  ~ProbeDisarm() { tt2g::probe_disarm(); }
};

TT2_DEV float ld_any(const void* p, int64_t i, int dt) {
  if (dt == TT2_F16) return (float)reinterpret_cast<const f16*>(p)[i];
  return dt == TT2_BF16 ? (float)reinterpret_cast<const bf16*>(p)[i] : reinterpret_cast<const float*>(p)[i];
}
TT2_DEV void st_any(void* p, int64_t i, int dt, float v) {
  if (dt == TT2_F16) reinterpret_cast<f16*>(p)[i] = (f16)v;
  else if (dt == TT2_BF16) reinterpret_cast<bf16*>(p)[i] = (bf16)v;
  else reinterpret_cast<float*>(p)[i] = v;
}

TT2_DEV float epi_value(const EpiParams& e, uint32_t seed, int m, int n, float v) {
  v *= e.alpha;
  if (e.bias) v += e.bias[n];
  if (e.res) v += ld_any(e.res, (int64_t)m * e.ldr + n, e.res_dt);
  if (e.act == ACT_RELU) v = fmaxf(v, 0.f);
  else if (e.act == ACT_TANH) v = tanhf(v);
  if (e.gate) v = ld_any(e.gate, (int64_t)m * e.ldg + n, e.gate_dt) != 0.f ? v * e.gate_scale : 0.f;
  if (e.drop.thr) v = drop_apply(e.drop, seed, (uint32_t)((int64_t)m * e.n_log + n), v);
  if (e.beta != 0.f) v += e.beta * ld_any(e.c, (int64_t)m * e.ldc + n, e.c_dt);
  return v;
}

// ---- LDS-DMA staging (global_load_lds_dwordx4: each lane's 16-B chunk lands at lds_base +
// 16*lane).  Out-of-range / conv-padding chunks load from a zero page (one per unit: 1 KB,
// zero-initialised, read-only).
__device__ __attribute__((aligned(64))) uint4 g_zero_page[64];

typedef __attribute__((address_space(1))) void gvoid_t;
typedef __attribute__((address_space(3))) void lvoid_t;

// swizzle of the 16-B chunk index for an M/N-contiguous tile row k (256-B rows)
TT2_DEV int mc_swz(int k) { return ((k & 3) << 1) ^ (((k >> 3) & 1) << 3); }

// Per-lane LDS-DMA source: the chunk's address, or the zero page when the chunk is out
// of range (or reads conv padding).  Branch-free per lane (a select), so the DMA issue
// is not wrapped in exec-mask branches; the conv test is behind a uniform branch.
TT2_DEV const void* chunk_src(const OpDesc& d, int outer, int inner) {
  bool ok = (outer < d.outer_max) & (inner < d.inner_max);
  int64_t off = (int64_t)outer * d.ld + inner;
  if (d.conv_t > 0) {
    const int ts = outer % d.conv_t + inner / d.conv_c - d.conv_pad;
    ok = ok & (ts >= 0) & (ts < d.conv_t);
    off -= (int64_t)d.conv_pad * d.conv_c;
  }
  const void* p = reinterpret_cast<const bf16*>(d.p) + off;
  return ok ? p : (const void*)g_zero_page;
}

// fragment (8 consecutive k of row r0 + (lane&15)) for k-step kk (0/1) of the 64-deep tile
template <bool KC>
TT2_DEV void frag2(Frag8<bf16>& f, const char* tile, int r0, int kk, int lane) {
  if (KC) {
    const int row = r0 + (lane & 15);
    const int h = 4 * kk + (lane >> 4);
    f.v = *reinterpret_cast<const bf16x8*>(tile + row * 128 + ((h ^ (row & 7)) << 4));
  } else {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int c = (r0 + 4 * p) >> 3;
    typedef __attribute__((address_space(3))) short4v lds_s4;
    const int k_lo = 32 * kk + 8 * g + q;
    const int k_hi = k_lo + 4;
    const char* a0 = tile + k_lo * 256 + ((c ^ mc_swz(k_lo)) << 4) + ((p & 1) << 3);
    const char* a1 = tile + k_hi * 256 + ((c ^ mc_swz(k_hi)) << 4) + ((p & 1) << 3);
    short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(a0));
    short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(a1));
    union { short s[8]; bf16x8 v; } u;
    u.s[0] = lo[0]; u.s[1] = lo[1]; u.s[2] = lo[2]; u.s[3] = lo[3];
    u.s[4] = hi[0]; u.s[5] = hi[1]; u.s[6] = hi[2]; u.s[7] = hi[3];
    f.v = u.v;
  }
}

// 8 consecutive elements of a row from a bf16 or f32 tensor (16-B aligned)
TT2_DEV void ld8_any(const void* p, int64_t off, int dt, float (&o)[8]) {
  if (dt == TT2_BF16) {
    const bf16x8 x = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16*>(p) + off);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (float)x[j];
  } else {
    const float* q = reinterpret_cast<const float*>(p) + off;
    const f32x4 a = *reinterpret_cast<const f32x4*>(q), b = *reinterpret_cast<const f32x4*>(q + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { o[j] = a[j]; o[4 + j] = b[j]; }
  }
}

// Chunk epilogue: 8 consecutive outputs of row m starting at column n0.  Full,
// aligned chunks (E.vec) take 16-B loads/stores with every option tested once
// per chunk; edge chunks fall back to the per-element path.
// pre_b: alpha and bias were already applied to v (v7's prefetched bias; E.vec, full chunk)
// Vectorised chunk epilogue without the store: o = epi(v) for a full, aligned chunk (E.vec).
// res_l / gate_l: the chunk of a bf16 residual / gate already staged in LDS by v7's loader
// waves.
TT2_DEV void unpack_lds8(const void* p, float (&t)[8]) {
  const bf16x8 x = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) t[j] = (float)x[j];
}
TT2_DEV void epi_calc8(const EpiParams& E, uint32_t seed, int m, int n0, const float (&v)[8], bool pre_b,
                       float (&o)[8], const void* res_l = nullptr, const void* gate_l = nullptr) {
  const int64_t off = (int64_t)m * E.ldc + n0;
  float t[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = pre_b ? v[j] : v[j] * E.alpha;
  if (E.bias && !pre_b) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(E.bias + n0), b = *reinterpret_cast<const f32x4*>(E.bias + n0 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { o[j] += a[j]; o[4 + j] += b[j]; }
  }
  if (E.res) {
    if (res_l) unpack_lds8(res_l, t);
    else ld8_any(E.res, (int64_t)m * E.ldr + n0, E.res_dt, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] += t[j];
  }
  if (E.act == ACT_RELU) {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = fmaxf(o[j], 0.f);
  } else if (E.act == ACT_TANH) {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = tanhf(o[j]);
  }
  if (E.gate) {
    if (gate_l) unpack_lds8(gate_l, t);
    else ld8_any(E.gate, (int64_t)m * E.ldg + n0, E.gate_dt, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = t[j] != 0.f ? o[j] * E.gate_scale : 0.f;
  }
  if (E.drop.thr) {
    drop_apply8(E.drop, seed, (uint32_t)((int64_t)m * E.n_log + n0), o);
  }
  if (E.beta != 0.f) {
    ld8_any(E.c, off, E.c_dt, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] += E.beta * t[j];
  }
}

TT2_DEV void epi_store8(const EpiParams& E, uint32_t seed, int m, int n0, int N, const float (&v)[8],
                        bool pre_b = false) {
  const int64_t off = (int64_t)m * E.ldc + n0;
  if (E.vec && n0 + 8 <= N) {
    float o[8];
    epi_calc8(E, seed, m, n0, v, pre_b, o);
    if (E.c_dt == TT2_BF16) {
      bf16x8 x;
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = (bf16)o[j];
      *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16*>(E.c) + off) = x;
    } else {
      float* c = reinterpret_cast<float*>(E.c) + off;
      *reinterpret_cast<f32x4*>(c) = f32x4{o[0], o[1], o[2], o[3]};
      *reinterpret_cast<f32x4*>(c + 4) = f32x4{o[4], o[5], o[6], o[7]};
    }
    return;
  }
  for (int j = 0; j < 8; ++j)
    if (n0 + j < N) st_any(E.c, off + j, E.c_dt, epi_value(E, seed, m, n0 + j, v[j]));
}

TT2_DEV void splitk_reduce_body(const float* ws, int splits, const EpiParams& E, int M, int N, int bx, int nbx) {
  const int64_t total = (int64_t)M * N;
  const uint32_t seed = E.drop.thr ? *E.drop.seed : 0u;
  if (E.ksum) {   // [splits][M] k-sum partials after the C slabs, fixed split order
    const float* kp = ws + splits * total;
    for (int64_t m = bx * (int64_t)blockDim.x + threadIdx.x; m < M; m += (int64_t)nbx * blockDim.x) {
      float v = 0.f;
      for (int z = 0; z < splits; ++z) v += kp[z * (int64_t)M + m];
      E.ksum[m] = E.ksum_beta != 0.f ? E.ksum_beta * E.ksum[m] + v : v;
    }
  }
  if ((N & 7) == 0 && E.vec) {
    // 8 consecutive columns per thread: 2 x 16-B slab loads per split (fixed split order),
    // then the vectorised chunk epilogue (16-B bias / residual / gate / C loads and stores)
    const int64_t t8 = total / 8;
    for (int64_t i = bx * (int64_t)blockDim.x + threadIdx.x; i < t8; i += (int64_t)nbx * blockDim.x) {
      const f32x4* w0 = reinterpret_cast<const f32x4*>(ws) + 2 * i;
      f32x4 lo = w0[0], hi = w0[1];
      for (int z = 1; z < splits; ++z) {
        const f32x4* wz = reinterpret_cast<const f32x4*>(ws + z * total) + 2 * i;
        lo += wz[0];
        hi += wz[1];
      }
      const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      int m, n;
      if (total < (1ll << 31)) {   // 32-bit division (the usual case) instead of a 64-bit one per chunk
        const uint32_t e = 8u * (uint32_t)i;
        m = (int)(e / (uint32_t)N);
        n = (int)(e - (uint32_t)m * (uint32_t)N);
      } else {
        m = (int)(8 * i / N);
        n = (int)(8 * i % N);
      }
      epi_store8(E, seed, m, n, N, v);
    }
    return;
  }
  if ((N & 3) == 0) {
    // 4 consecutive columns per thread (16-B partial-slab loads), fixed split order
    const int64_t t4 = total / 4;
    for (int64_t i = bx * (int64_t)blockDim.x + threadIdx.x; i < t4; i += (int64_t)nbx * blockDim.x) {
      // two accumulators, 4 slab loads in flight per step (fixed order per element)
      f32x4 v = reinterpret_cast<const f32x4*>(ws)[i], w = f32x4{0.f, 0.f, 0.f, 0.f};
      int z = 1;
      for (; z + 3 < splits; z += 4) {
        const f32x4 a0 = reinterpret_cast<const f32x4*>(ws + z * total)[i];
        const f32x4 a1 = reinterpret_cast<const f32x4*>(ws + (z + 1) * total)[i];
        const f32x4 a2 = reinterpret_cast<const f32x4*>(ws + (z + 2) * total)[i];
        const f32x4 a3 = reinterpret_cast<const f32x4*>(ws + (z + 3) * total)[i];
        v += a0 + a2;
        w += a1 + a3;
      }
      for (; z < splits; ++z) v += reinterpret_cast<const f32x4*>(ws + z * total)[i];
      v += w;
      const int m = (int)(4 * i / N), n = (int)(4 * i % N);
#pragma unroll
      for (int j = 0; j < 4; ++j) st_any(E.c, (int64_t)m * E.ldc + n + j, E.c_dt, epi_value(E, seed, m, n + j, v[j]));
    }
    return;
  }
  for (int64_t i = bx * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)nbx * blockDim.x) {
    float v = 0.f;
    for (int z = 0; z < splits; ++z) v += ws[z * total + i];
    const int m = (int)(i / N), n = (int)(i % N);
    st_any(E.c, (int64_t)m * E.ldc + n, E.c_dt, epi_value(E, seed, m, n, v));
  }
}

TT2_DEV void bf16x8_unpack(const u32x4& v, float (&f)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = __uint_as_float(v[j] << 16);
    f[2 * j + 1] = __uint_as_float(v[j] & 0xffff0000u);
  }
}

// flat block index -> XCD-contiguous work item (blocks b and b + 8 share an XCD)
TT2_DEV int xcd_item(int bid, int n) {
  const int q = n / 8, r = n % 8, x = bid % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + bid / 8;
}

}  // namespace
