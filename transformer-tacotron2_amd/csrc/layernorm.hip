// layernorm.hip -- fused residual + dropout + LayerNorm, forward and backward, and the decode
// step's residual combine + LayerNorm (gfx950).
//
// LayerNorm (post-LN sublayer end):
//   s = x + drop(branch);  y = (s - mean(s)) * rstd * gamma + beta
// one wave per 512-wide row (8 values per lane, 16-B vector loads).  The
// backward recomputes s from the saved x and branch (no s buffer) and emits
// ds (the residual-stream gradient) and drop-masked ds (the branch gradient),
// plus per-workgroup gamma/beta partial sums, summed in a fixed order by ln_bwd_finalize or,
// deferred, by a later backward's spare waves (ln_fin_col).
// (BatchNorm: batchnorm.hip; ld8f, st8, st8nt, ln_combine_row: tt2_common.h.)
#include <math.h>

#include <type_traits>

#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {
constexpr int NT = 256;

// A deferred LayerNorm-backward finalize: column sums of part[nb][3][C] into (dg, db, dd).
struct LnFin {
  const float* part;
  float* dg; float* db; float* dd;
  float gb;
  int nb;   // 0 = nothing to finalize
};

struct LnArgs {
  const void* x; const void* branch; const void* dy;
  void* y; void* dx; void* dbranch;
  const float* gamma; const float* beta;
  float* mean; float* rstd;
  float* part;  // bwd: [gridDim.x][3][C] (dgamma, dbeta, dbias) partial sums
  float* dgamma; float* dbeta; float* dbias;
  float grad_beta;
  int M, C;
  float eps;
  DropDesc drop;
  LnFin fin;   // bwd: an earlier deferred call's finalize, done in this launch's spare waves
};

template <typename T> TT2_DEV void unpack8(const uint4 (&u)[sizeof(T) / 2], float (&v)[8]) {
  if constexpr (sizeof(T) == 2) {
    union { uint4 q; bf16x8 b; } c;
    c.q = u[0];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)c.b[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = __uint_as_float((&u[0].x)[j]); v[4 + j] = __uint_as_float((&u[1].x)[j]); }
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void ln_fwd_kernel(LnArgs a) {
  constexpr int NV = sizeof(T) / 2;   // 16-B vectors per 8 elements
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.M) return;
  const int c0 = lane * 8;
  const int64_t off = (int64_t)row * a.C + c0;
  // every load of the row first (x, branch, gamma, beta, the dropout seed): one round trip
  // (a branch-dependent load behind the x unpack used to cost a second one)
  const bool has_br = a.branch != nullptr;
  const uint4* X = reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(a.x) + off);
  const uint4* BR = reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(has_br ? a.branch : a.x) + off);
  uint4 xr[NV], brr[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) { xr[v] = X[v]; brr[v] = BR[v]; }
  const f32x4 g0 = *reinterpret_cast<const f32x4*>(a.gamma + c0), g1 = *reinterpret_cast<const f32x4*>(a.gamma + c0 + 4);
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(a.beta + c0), b1 = *reinterpret_cast<const f32x4*>(a.beta + c0 + 4);
  const uint32_t seed = a.drop.thr ? *a.drop.seed : 0u;
  float s[8], br[8];
  unpack8<T>(xr, s);
  if (has_br) {
    unpack8<T>(brr, br);
    if (a.drop.thr) drop_apply8(a.drop, seed, (uint32_t)off, br);
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += br[j];
  }
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) sum += s[j];
  const float mean = wave_sum(sum) / a.C;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) { const float d = s[j] - mean; sq += d * d; }
  const float rstd = rsqrtf(wave_sum(sq) / a.C + a.eps);
  float y[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    y[j] = (s[j] - mean) * rstd * g0[j] + b0[j];
    y[4 + j] = (s[4 + j] - mean) * rstd * g1[j] + b1[j];
  }
  st8nt(reinterpret_cast<T*>(a.y) + off, y);
  if (lane == 0 && a.mean) { a.mean[row] = mean; a.rstd[row] = rstd; }
}

// Decode-step residual combine + LayerNorm: y = LN(x + bias + sum_s part[s]) over the
// 512 columns of a row, where part holds the raw partial sums of a skinny split-K
// projection ([S][M][512] f32).  One wave per row, every load (x, the S slabs, bias,
// gamma, beta) issued before the first reduction: one memory round trip.
#ifndef LNC_ROWS
#define LNC_ROWS 1   // rows (waves) per work group: one row per CU reads its 8 slabs faster than 4 (r06zp)
#endif
template <int S, typename T>
__global__ __launch_bounds__(64 * LNC_ROWS) void ln_combine_kernel(const T* x, const float* part, const float* bias,
                                                                   const float* gamma, const float* beta, T* y, int M,
                                                                   float eps) {
  constexpr int C = 512;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * LNC_ROWS + (threadIdx.x >> 6);
  if (row >= M) return;
  float o[8];
  ln_combine_row<S, T>(x + (int64_t)row * C, part + (int64_t)row * C, (int64_t)M * C, bias, gamma, beta, eps, lane,
                       o);
  st8(y + (int64_t)row * C + lane * 8, o);
}

// Backward: 8 waves per workgroup, one 512-wide row per wave at a time, software-
// pipelined: the raw x / branch / dy chunks of the wave's next row are loaded before the
// current row is reduced, so every wave always has a row of loads in flight.  The
// dropout keep-mask of an element is hashed once and used for both s = x + drop(br)
// and dbranch = drop(ds).  Per-workgroup (dgamma, dbeta, dbias) column partials go to
// part[block][3][C]; ln_bwd_finalize sums them (fixed order: bitwise reproducible).
// 12 waves: 17.0-17.5 us at 12800 x 512 against 18.0-18.5 with 8 and 18.0 with 16
// (tools/norm_ab.py, gpurun_out/r05ln)
constexpr int LNB_NT = 768;
template <typename T> struct LnRow { uint4 x[sizeof(T) / 2], dy[sizeof(T) / 2], br[sizeof(T) / 2]; float mean, rstd; };

template <typename T>
TT2_DEV void ln_row_load(LnRow<T>& r, const LnArgs& a, int row, int c0) {
  constexpr int NV = sizeof(T) / 2;   // 16-B vectors per 8 elements
  const int64_t off = (int64_t)row * a.C + c0;
  const uint4* X = reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(a.x) + off);
  const uint4* DY = reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(a.dy) + off);
#pragma unroll
  for (int v = 0; v < NV; ++v) { r.x[v] = X[v]; r.dy[v] = DY[v]; }
  if (a.branch) {
    const uint4* BR = reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(a.branch) + off);
#pragma unroll
    for (int v = 0; v < NV; ++v) r.br[v] = BR[v];
  }
  r.mean = a.mean[row];
  r.rstd = a.rstd[row];
}


// One wave sums output o (= which * C + c) of a deferred finalize over the nb partial rows
// (4 loads in flight per lane, then a DPP wave sum): a fixed order, shared by the chained
// and the standalone finalize.
TT2_DEV void ln_fin_col(const LnFin& f, int C, int o, int lane) {
  const int which = o / C, c = o - which * C;
  float* dst = which == 0 ? f.dg : (which == 1 ? f.db : f.dd);
  if (!dst) return;
  const float* src = f.part + (int64_t)which * C + c;
  const int64_t rs = 3 * (int64_t)C;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int r = lane;
  for (; r + 192 < f.nb; r += 256) {
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] += src[(r + 64 * u) * rs];
  }
  for (; r < f.nb; r += 64) acc[0] += src[r * rs];
  const float v = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if (lane == 0) dst[c] = f.gb != 0.f ? f.gb * dst[c] + v : v;
}

__global__ __launch_bounds__(LNB_NT) void ln_fin_kernel(LnFin f, int C) {
  const int o = blockIdx.x * (LNB_NT / 64) + (threadIdx.x >> 6);
  if (o < 3 * C) ln_fin_col(f, C, o, threadIdx.x & 63);
}

template <typename T>
__global__ __launch_bounds__(LNB_NT) void ln_bwd_kernel(LnArgs a) {
  constexpr int HW = LNB_NT / 128;   // half the waves
  __shared__ float red[3][HW][512];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c0 = lane * 8;
  float g[8];
  {
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(a.gamma + c0), g1 = *reinterpret_cast<const f32x4*>(a.gamma + c0 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { g[j] = g0[j]; g[4 + j] = g1[j]; }
  }
  float pg[8], pb[8], pd[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) pg[j] = pb[j] = pd[j] = 0.f;
  const uint32_t seed = a.drop.thr ? *a.drop.seed : 0u;
  const int stride = gridDim.x * (LNB_NT / 64);
  int row = blockIdx.x * (LNB_NT / 64) + w;
  LnRow<T> cur, nxt;
  if (row < a.M) ln_row_load<T>(cur, a, row, c0);
  for (; row < a.M; row += stride) {
    if (row + stride < a.M) ln_row_load<T>(nxt, a, row + stride, c0);
    const int64_t off = (int64_t)row * a.C + c0;
    float s[8], dy[8], keep[8];
    unpack8<T>(cur.x, s);
    unpack8<T>(cur.dy, dy);
    {
      const uint32_t kb = a.drop.thr ? drop_bits8(seed, a.drop.site, (uint32_t)off, a.drop.thr) : 0xFFu;
      const float sc = a.drop.thr ? a.drop.scale : 1.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) keep[j] = (kb >> j) & 1u ? sc : 0.f;
    }
    if (a.branch) {
      float br[8];
      unpack8<T>(cur.br, br);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += br[j] * keep[j];
    }
    float c1 = 0.f, c2 = 0.f, xh[8], gd[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xh[j] = (s[j] - cur.mean) * cur.rstd;
      gd[j] = g[j] * dy[j];
      c1 += gd[j];
      c2 += gd[j] * xh[j];
      pg[j] += dy[j] * xh[j];
      pb[j] += dy[j];
    }
    c1 = wave_sum(c1) / a.C;
    c2 = wave_sum(c2) / a.C;
    float ds[8], db[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ds[j] = cur.rstd * (gd[j] - c1 - xh[j] * c2);
      db[j] = ds[j] * keep[j];
      pd[j] += db[j];
    }
    st8nt(reinterpret_cast<T*>(a.dx) + off, ds);
    if (a.dbranch) st8nt(reinterpret_cast<T*>(a.dbranch) + off, db);
    cur = nxt;
  }
  // the waves' partials: the upper half into LDS rows, the lower half adds its own, then rows summed
  if (w >= HW) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[0][w - HW][c0 + j] = pg[j]; red[1][w - HW][c0 + j] = pb[j]; red[2][w - HW][c0 + j] = pd[j]; }
  }
  __syncthreads();
  if (w < HW) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[0][w][c0 + j] += pg[j]; red[1][w][c0 + j] += pb[j]; red[2][w][c0 + j] += pd[j]; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * a.C; i += LNB_NT) {
    const int which = i / a.C, c = i % a.C;
    float v = red[which][0][c] + red[which][1][c] + red[which][2][c] + red[which][3][c];
#pragma unroll
    for (int h = 4; h < HW; ++h) v += red[which][h][c];
    a.part[((int64_t)blockIdx.x * 3 + which) * a.C + c] = v;
  }
  if (a.fin.nb) {   // the previous LayerNorm's column sums, spread over every workgroup's waves
    const int per = (3 * a.C + gridDim.x - 1) / gridDim.x;
    for (int i = w; i < per; i += LNB_NT / 64) {
      const int o = blockIdx.x * per + i;
      if (o < 3 * a.C) ln_fin_col(a.fin, a.C, o, lane);
    }
  }
}

// grid (C / 16, 3): 16 columns of partial array y per block, 16 row groups of 16
// lanes; each lane sums nb/16 partial rows with independent loads in flight.
__global__ __launch_bounds__(256) void ln_bwd_finalize(LnArgs a, int nb) {
  __shared__ float sm[16][17];
  const int which = blockIdx.y;
  float* dst = which == 0 ? a.dgamma : (which == 1 ? a.dbeta : a.dbias);
  if (!dst) return;
  const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  const float* src = a.part + (int64_t)which * a.C + c;
  const int64_t rs = 3 * (int64_t)a.C;   // stride between partial rows
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int r = rg;
  for (; r + 48 < nb; r += 64) {
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] += src[(r + 16 * u) * rs];
  }
  for (; r < nb; r += 16) acc[0] += src[r * rs];
  sm[rg][cl] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  __syncthreads();
  if (rg == 0) {
    float v = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) v += sm[g][cl];
    dst[c] = a.grad_beta != 0.f ? a.grad_beta * dst[c] + v : v;
  }
}

}  // namespace

extern "C" int tt2_layernorm_fwd(const tt2_ln_args* p, hipStream_t s) {
  if (p->c != 512) return tt2_set_error(TT2_E_INVALID, "tt2_layernorm: C must be 512");
  LnArgs a{};
  a.x = p->x; a.branch = p->branch; a.y = p->y;
  a.gamma = p->gamma; a.beta = p->beta; a.mean = p->mean; a.rstd = p->rstd;
  a.M = p->m; a.C = p->c; a.eps = p->eps;
  a.drop = drop_of(p);
  if (p->m == 0) return TT2_OK;
  dim3 g((p->m + 3) / 4);
  by_dtype(p->dtype, [&](auto t) { hipLaunchKernelGGL(ln_fwd_kernel<decltype(t)>, g, dim3(NT), 0, s, a); });
  return tt2_check_launch(hipGetLastError(), "tt2_layernorm_fwd");
}

extern "C" int tt2_ln_combine(const void* x, const float* part, int32_t splits, const float* bias,
                              const float* gamma, const float* beta, void* y, int32_t m, int32_t c, float eps,
                              int32_t dtype, hipStream_t s) {
  if (c != 512) return tt2_set_error(TT2_E_INVALID, "tt2_ln_combine: c must be 512");
  if (!x || !part || !bias || !gamma || !beta || !y) return tt2_set_error(TT2_E_INVALID, "tt2_ln_combine: null");
  if (dtype != TT2_DT_BF16 && dtype != TT2_DT_F16) return tt2_set_error(TT2_E_INVALID, "tt2_ln_combine: bf16 / f16");
  if (m <= 0) return TT2_OK;
  const dim3 g((m + LNC_ROWS - 1) / LNC_ROWS), b(64 * LNC_ROWS);
  auto launch = [&](auto splits_c) {   // (this entry's pair of types is f16 / bf16, not by_dtype's)
    constexpr int S = decltype(splits_c)::value;
    auto of = [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((ln_combine_kernel<S, T>), g, b, 0, s, (const T*)x, part, bias, gamma, beta, (T*)y, m, eps);
    };
    if (dtype == TT2_DT_F16) of(f16());
    else of(bf16());
  };
  switch (splits) {
    case 1: launch(std::integral_constant<int, 1>()); break;
    case 2: launch(std::integral_constant<int, 2>()); break;
    case 4: launch(std::integral_constant<int, 4>()); break;
    case 8: launch(std::integral_constant<int, 8>()); break;
    case 16: launch(std::integral_constant<int, 16>()); break;
    default: return tt2_set_error(TT2_E_INVALID, "tt2_ln_combine: splits must be 1, 2, 4, 8 or 16");
  }
  return tt2_check_launch(hipGetLastError(), "tt2_ln_combine");
}

static int ln_bwd_blocks(int m) {
  // at most one workgroup per CU, 16+ rows each (512 / 1024 / 128 work groups: 19.0-19.3 / 23.6 /
  // 21.5 us against 17.9-18.2 us at 12800 x 512, tools/norm_ab.py, gpurun_out/r05hp)
  return min(256, (m + 15) / 16);
}

static LnFin ln_fin_of(const tt2_ln_args* q) {
  return LnFin{reinterpret_cast<const float*>(q->workspace), q->dgamma, q->dbeta, q->dbias, q->grad_beta,
               ln_bwd_blocks(q->m)};
}

extern "C" size_t tt2_layernorm_bwd_workspace_size(const tt2_ln_args* p) {
  return (size_t)ln_bwd_blocks(p->m) * 3 * p->c * sizeof(float);
}

extern "C" int tt2_layernorm_bwd(const tt2_ln_args* p, hipStream_t s) {
  if (p->c != 512) return tt2_set_error(TT2_E_INVALID, "tt2_layernorm: C must be 512");
  if (!p->workspace || p->ws_bytes < tt2_layernorm_bwd_workspace_size(p))
    return tt2_set_error(TT2_E_INVALID, "tt2_layernorm_bwd: workspace too small");
  if (p->dbias && !p->branch) return tt2_set_error(TT2_E_INVALID, "tt2_layernorm_bwd: dbias needs a branch");
  LnArgs a{};
  a.x = p->x; a.branch = p->branch; a.dy = p->dy; a.dx = p->dx; a.dbranch = p->dbranch;
  a.gamma = p->gamma; a.beta = p->beta; a.mean = p->mean; a.rstd = p->rstd;
  a.part = reinterpret_cast<float*>(p->workspace);
  a.dgamma = p->dgamma; a.dbeta = p->dbeta; a.dbias = p->dbias; a.grad_beta = p->grad_beta;
  a.M = p->m; a.C = p->c; a.eps = p->eps;
  a.drop = drop_of(p);
  if (const tt2_ln_args* q = p->finalize_prev) {
    if (!q->defer_finalize || q->c != p->c || !q->workspace)
      return tt2_set_error(TT2_E_INVALID, "tt2_layernorm_bwd: finalize_prev must be a deferred call with the same c");
    if (q->workspace == p->workspace && q->m > 0)
      return tt2_set_error(TT2_E_INVALID, "tt2_layernorm_bwd: finalize_prev's workspace is overwritten by this call");
    if (q->m > 0) a.fin = ln_fin_of(q);
  }
  if (p->m == 0) {   // nothing of our own; still complete the chained finalize
    if (a.fin.nb) hipLaunchKernelGGL(ln_fin_kernel, dim3((3 * p->c + LNB_NT / 64 - 1) / (LNB_NT / 64)), dim3(LNB_NT), 0, s, a.fin, p->c);
    return tt2_check_launch(hipGetLastError(), "tt2_layernorm_bwd");
  }
  const int nb = ln_bwd_blocks(p->m);
  by_dtype(p->dtype, [&](auto t) { hipLaunchKernelGGL(ln_bwd_kernel<decltype(t)>, dim3(nb), dim3(LNB_NT), 0, s, a); });
  if (!p->defer_finalize) {
    a.fin = LnFin{};
    hipLaunchKernelGGL(ln_bwd_finalize, dim3(p->c / 16, 3), dim3(256), 0, s, a, nb);
  }
  return tt2_check_launch(hipGetLastError(), "tt2_layernorm_bwd");
}

extern "C" int tt2_layernorm_bwd_finalize(const tt2_ln_args* p, hipStream_t s) {
  if (!p->defer_finalize || !p->workspace) return tt2_set_error(TT2_E_INVALID, "tt2_layernorm_bwd_finalize: not a deferred call");
  if (p->m == 0) return TT2_OK;
  hipLaunchKernelGGL(ln_fin_kernel, dim3((3 * p->c + LNB_NT / 64 - 1) / (LNB_NT / 64)), dim3(LNB_NT), 0, s, ln_fin_of(p), p->c);
  return tt2_check_launch(hipGetLastError(), "tt2_layernorm_bwd_finalize");
}
