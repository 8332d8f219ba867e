// batchnorm.hip -- training/eval BatchNorm with fused activation + dropout (+ residual), forward
// and backward, and the four SyncBatchNorm phases (gfx950).
//
// BatchNorm1d over rows (SURVEY 8(a) a1 encoder convs, a9 post-net):
//   train: per-chunk (mean, M2) partials -> Chan combine -> mean, rstd, running
//   stats update (unbiased var, momentum); eval: running stats.
//   z = act((y - mean) * rstd * gamma + beta); out = drop(z) (+ res)
// The backward recomputes z from y (saved) and the statistics.
// (LayerNorm: layernorm.hip; ld8f, st8nt, act_f, act_grad_from_out: tt2_common.h.)
#include <math.h>

#include <algorithm>

#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {
constexpr int NT = 256;

// floats per rank and column of the SyncBatchNorm exchange: forward (mean, M2, rows, mean -
// (float)mean: the rank mean travels as an f32 pair, a single f32 would put its rounding into
// the combine's n_r (mean_r - mean)^2 to first order), backward (sum dpre, sum dpre * xhat, rows, 0)
constexpr int BN_SLOT = 4;

struct BnArgs {
  const void* y; const void* dout; const void* res;
  void* out; void* dy;
  const float* gamma; const float* beta;
  float* mean; float* rstd;
  float* run_mean; float* run_var;
  float* part;  // train stats: [R][2][C] (chunk mean, chunk M2); bwd: [R][2][C] sums
  float* dgamma; float* dbeta;
  int64_t res_ld;
  int M, C, R, rows_per, act, out_dt, res_dt, training;
  int y_dt;   // y's element type (bn_fin64 re-reads the chunk pivots)
  int rel;    // part's chunk means are relative to the chunk's first row of y (bn_stats_kernel's own partials)
  float eps, momentum;
  DropDesc drop;
  // SyncBatchNorm exchange (tt2_batchnorm_{fwd,bwd}_{stats,apply}): [W][BN_SLOT][C] rank slots
  // (this rank's moments or sums and its row count, zeros in the others; all-reduced by the
  // caller) + [2][C]
  float* sync;
  int W, rank;
  int64_t Mtot;   // rows behind the statistics: M (SyncBN: the exchanged counts, see inv_m)
  const float* inv_m;   // SyncBN backward apply: 1 / (sum of the ranks' rows), written by bn_bwd_sync_kernel
};

// (fast_tanh, act_f, act_grad_from_out: tt2_common.h, shared with the GEMM's fused BatchNorm sums)

// All BatchNorm kernels work on 8-column groups (16-B loads/stores; C % 8 == 0).
// Statistics: one workgroup per chunk of rows_per rows; CG = C/8 column groups x
// (256/CG) row lanes.  Chunk moments use a per-column shift (the chunk's first row)
// so sum / sum-of-squares keep full precision; chunks are combined exactly in double.
// The chunk mean is stored relative to that shift (a.rel); bn_fin64 re-reads the shift from y
// and, for a column whose mean dwarfs its spread, adds the two in double (see there).  Moments
// that a GEMM epilogue produced (stats_rows > 0) hold absolute means.

TT2_DEV void ld8v(const void* p, int64_t off, int dt, float (&v)[8]) {
  if (dt == TT2_BF16) ld8f(reinterpret_cast<const bf16*>(p) + off, v);
  else ld8f(reinterpret_cast<const float*>(p) + off, v);
}

template <typename T>
__global__ __launch_bounds__(NT) void bn_stats_kernel(BnArgs a) {
  __shared__ float red[2][NT][8];
  const int CG = a.C >> 3, nrl = NT / CG;
  const int cg = threadIdx.x % CG, rl = threadIdx.x / CG;
  const int r0 = blockIdx.x * a.rows_per, r1 = min(a.M, r0 + a.rows_per);
  const T* y = reinterpret_cast<const T*>(a.y);
  float k[8], s1[8], s2[8];
  ld8f(y + (int64_t)r0 * a.C + cg * 8, k);
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  if (rl < nrl) {
    for (int r = r0 + rl; r < r1; r += nrl) {
      float v[8];
      ld8f(y + (int64_t)r * a.C + cg * 8, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[j] - k[j];
        s1[j] += d;
        s2[j] += d * d;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { red[0][threadIdx.x][j] = s1[j]; red[1][threadIdx.x][j] = s2[j]; }
  __syncthreads();
  if (threadIdx.x < CG) {
    const float n = (float)(r1 - r0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float S1 = 0.f, S2 = 0.f;
      for (int l = 0; l < nrl; ++l) { S1 += red[0][l * CG + cg][j]; S2 += red[1][l * CG + cg][j]; }
      const int c = cg * 8 + j;
      a.part[((int64_t)blockIdx.x * 2 + 0) * a.C + c] = a.rel ? S1 / n : k[j] + S1 / n;
      a.part[((int64_t)blockIdx.x * 2 + 1) * a.C + c] = fmaxf(S2 - S1 * S1 / n, 0.f);
    }
  }
}

// Chunk combine of 64 columns per workgroup: thread (column cl = t % 64, group g = t / 64)
// walks chunks r = g, g + 4, ... (4 loads in flight), then the 4 group partials are added in
// order.  Exact two-pass combine of the chunk moments (no per-chunk division): mean =
// sum n_c mean_c / n, then M2 = sum M2_c + n_c (mean_c - mean)^2, accumulated in double.  The
// standalone finalize (grid ceil(C / 64)) and the apply kernels that finalize their own column
// block (bn_apply_fin_kernel) run this same code, so both give the same statistics.
constexpr int BNC_COLS = 64, BNC_G = NT / BNC_COLS;
// bn_fin64 / bn_bsum64 combine exactly red[0..3] in a fixed order (the standalone finalize's
// summation order, which the fused apply must reproduce bit for bit)
static_assert(BNC_G == 4, "bn_fin64 / bn_bsum64 sum four chunk groups");
struct BnFinScratch { double red[BNC_G][BNC_COLS]; double mu[BNC_COLS]; float mean[BNC_COLS], rstd[BNC_COLS]; int ill[BNC_COLS]; };

// forward: mean / rstd of column block cb into S.mean / S.rstd; write: also a.mean / a.rstd and
// the running statistics (or, SyncBN, this rank's slots)
TT2_DEV void bn_fin64(const BnArgs& a, int cb, BnFinScratch& S, bool write) {
  const int cl = threadIdx.x % BNC_COLS, g = threadIdx.x / BNC_COLS;
  const int c = cb * BNC_COLS + cl;
  const bool ok = c < a.C;
  const int cc = ok ? c : 0;
  auto nrows = [&](int r) { return (double)min(a.rows_per, a.M - r * a.rows_per); };
  auto pm = [&](int r, int w) { return a.part[((int64_t)r * 2 + w) * a.C + cc]; };
  auto piv = [&](int r) {   // the shift chunk r's mean is relative to (0: an absolute mean)
    if (!a.rel) return 0.f;
    const int64_t i = (int64_t)r * a.rows_per * a.C + cc;
    return a.y_dt == TT2_BF16 ? (float)reinterpret_cast<const bf16*>(a.y)[i] : reinterpret_cast<const float*>(a.y)[i];
  };
  // Round 0 takes each chunk mean as the one f32 value shift + delta rounds to (what an absolute
  // f32 mean holds).  That rounding, up to ulp(mean) / 2, enters n_c (mean_c - mean)^2 to first
  // order: harmless while the mean is of the spread's size, but at |mean| = 1e3 sigma rstd was
  // off by up to 60 x the error of a two-pass f32 evaluation.  A column block holding a column
  // with |mean| > 8 sigma runs round 1, where those columns take shift + delta in double.
  // Cost of re-reading the shifts (R strided loads of y per thread, L2-resident after the
  // statistics pass): none measured, tt2_batchnorm_fwd with its own statistics at 12800 x 512 takes
  // 51.6 us in f32 and 89.9 us in bf16 per call before and after (back-to-back calls, MI355X).
  double mu = 0.0, m2 = 0.0;
  for (int round = 0; round < 2; ++round) {
    const bool exact = round == 1 && S.ill[cl];
    auto mean_of = [&](float k, float v) { return exact ? (double)k + (double)v : (double)(k + v); };
    double acc = 0.0;
    int r = g;
    for (; r + 3 * BNC_G < a.R; r += 4 * BNC_G) {
      float v[4], k[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { v[u] = pm(r + u * BNC_G, 0); k[u] = piv(r + u * BNC_G); }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += nrows(r + u * BNC_G) * mean_of(k[u], v[u]);
    }
    for (; r < a.R; r += BNC_G) acc += nrows(r) * mean_of(piv(r), pm(r, 0));
    S.red[g][cl] = acc;
    __syncthreads();
    if (g == 0) S.mu[cl] = (((S.red[0][cl] + S.red[1][cl]) + S.red[2][cl]) + S.red[3][cl]) / a.M;
    __syncthreads();
    mu = S.mu[cl];
    acc = 0.0;
    r = g;
    for (; r + 3 * BNC_G < a.R; r += 4 * BNC_G) {
      float m1[4], q[4], k[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { m1[u] = pm(r + u * BNC_G, 0); q[u] = pm(r + u * BNC_G, 1); k[u] = piv(r + u * BNC_G); }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double d = mean_of(k[u], m1[u]) - mu;
        acc += q[u] + nrows(r + u * BNC_G) * d * d;
      }
    }
    for (; r < a.R; r += BNC_G) {
      const double d = mean_of(piv(r), pm(r, 0)) - mu;
      acc += pm(r, 1) + nrows(r) * d * d;
    }
    __syncthreads();
    S.red[g][cl] = acc;
    __syncthreads();
    m2 = ((S.red[0][cl] + S.red[1][cl]) + S.red[2][cl]) + S.red[3][cl];
    if (round == 1) break;
    const int ill = a.rel && mu * mu * (double)a.M > 64.0 * m2;
    __syncthreads();   // every thread has read S.red
    if (g == 0) S.ill[cl] = ill;
    if (!__syncthreads_or(ill)) break;
  }
  if (g != 0) return;
  const double n = a.M;
  const double var = m2 / n;
  S.mean[cl] = (float)mu;
  S.rstd[cl] = (float)(1.0 / sqrt(var + a.eps));
  if (!write || !ok) return;
  if (a.sync) {   // this rank's (mean, M2, rows) into its slot; the other ranks' slots zero
    const float hi = (float)mu, lo = (float)(mu - (double)hi);
    for (int r2 = 0; r2 < a.W; ++r2) {
      a.sync[((int64_t)r2 * BN_SLOT + 0) * a.C + c] = r2 == a.rank ? hi : 0.f;
      a.sync[((int64_t)r2 * BN_SLOT + 1) * a.C + c] = r2 == a.rank ? (float)m2 : 0.f;
      a.sync[((int64_t)r2 * BN_SLOT + 2) * a.C + c] = r2 == a.rank ? (float)a.M : 0.f;
      a.sync[((int64_t)r2 * BN_SLOT + 3) * a.C + c] = r2 == a.rank ? lo : 0.f;
    }
    return;
  }
  a.mean[c] = S.mean[cl];
  a.rstd[c] = S.rstd[cl];
  if (a.run_mean) {
    const double unb = n > 1 ? m2 / (n - 1) : var;
    a.run_mean[c] = (float)((1.0 - a.momentum) * a.run_mean[c] + a.momentum * mu);
    a.run_var[c] = (float)((1.0 - a.momentum) * a.run_var[c] + a.momentum * unb);
  }
}

__global__ __launch_bounds__(NT) void bn_finalize_kernel(BnArgs a) {
  __shared__ BnFinScratch S;
  if (!a.training) {   // eval: the running statistics
    const int c = blockIdx.x * BNC_COLS + threadIdx.x;
    if (threadIdx.x < BNC_COLS && c < a.C) {
      a.mean[c] = a.run_mean[c];
      a.rstd[c] = rsqrtf(a.run_var[c] + a.eps);
    }
    return;
  }
  bn_fin64(a, blockIdx.x, S, true);
}

// SyncBatchNorm: combine the W exchanged rank moments in rank order, exactly as
// bn_finalize_kernel combines chunks, weighted by each rank's row count n_r (ranks may hold
// different numbers of rows): N = sum n_r, mean = sum n_r mean_r / N,
// M2 = sum M2_r + n_r (mean_r - mean)^2.  Slots are [W][BN_SLOT][C]: (mean hi, M2, n, mean lo) per rank.
__global__ __launch_bounds__(NT) void bn_sync_finalize_kernel(BnArgs a) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= a.C) return;
  auto slot = [&](int r, int w) { return (double)a.sync[((int64_t)r * BN_SLOT + w) * a.C + c]; };
  double n = 0.0, mu = 0.0;
  for (int r = 0; r < a.W; ++r) {
    n += slot(r, 2);
    mu += slot(r, 2) * (slot(r, 0) + slot(r, 3));
  }
  mu /= n;
  double m2 = 0.0;
  for (int r = 0; r < a.W; ++r) {
    const double d = (slot(r, 0) + slot(r, 3)) - mu;
    m2 += slot(r, 1) + slot(r, 2) * d * d;
  }
  const double var = m2 / n;
  a.mean[c] = (float)mu;
  a.rstd[c] = (float)(1.0 / sqrt(var + a.eps));
  if (a.run_mean) {
    const double unb = n > 1 ? m2 / (n - 1) : var;
    a.run_mean[c] = (float)((1.0 - a.momentum) * a.run_mean[c] + a.momentum * mu);
    a.run_var[c] = (float)((1.0 - a.momentum) * a.run_var[c] + a.momentum * unb);
  }
}

// SyncBatchNorm backward: the global column sums (sum dpre, sum dpre * xhat) from the W
// exchanged rank slots, in rank order, into the [2][C] region after the slots, and
// 1 / N (N = sum of the ranks' row counts, as f32: the value bn_bwd_apply_kernel forms from
// Mtot on one rank, so one SyncBN rank reproduces plain BatchNorm bit for bit) after them
__global__ __launch_bounds__(NT) void bn_bwd_sync_kernel(BnArgs a) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= a.C) return;
  float s1 = 0.f, s2 = 0.f, n = 0.f;
  for (int r = 0; r < a.W; ++r) {
    s1 += a.sync[((int64_t)r * BN_SLOT + 0) * a.C + c];
    s2 += a.sync[((int64_t)r * BN_SLOT + 1) * a.C + c];
    n += a.sync[((int64_t)r * BN_SLOT + 2) * a.C + c];
  }
  a.sync[((int64_t)a.W * BN_SLOT + 0) * a.C + c] = s1;
  a.sync[((int64_t)a.W * BN_SLOT + 1) * a.C + c] = s2;
  if (c == 0) a.sync[((int64_t)a.W * BN_SLOT + 2) * a.C] = 1.f / n;
}

// per-column constants of 8 consecutive columns
TT2_DEV void col8(const float* p, int c0, float (&v)[8]) {
  const f32x4 lo = *reinterpret_cast<const f32x4*>(p + c0), hi = *reinterpret_cast<const f32x4*>(p + c0 + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { v[j] = lo[j]; v[4 + j] = hi[j]; }
}

template <typename T>
__global__ __launch_bounds__(NT) void bn_apply_kernel(BnArgs a) {
  const int CG = a.C >> 3;
  const int nq = a.M * CG;
  const T* y = reinterpret_cast<const T*>(a.y);
  const uint32_t seed = a.drop.thr ? *a.drop.seed : 0u;
  for (int q = blockIdx.x * NT + threadIdx.x; q < nq; q += gridDim.x * NT) {
    const int m = q / CG, c0 = (q - m * CG) * 8;
    const int64_t i0 = (int64_t)m * a.C + c0;
    float v[8], mu[8], rs[8], g[8], b[8];
    ld8f(y + i0, v);
    col8(a.mean, c0, mu); col8(a.rstd, c0, rs); col8(a.gamma, c0, g); col8(a.beta, c0, b);
    float z[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = act_f(a.act, (v[j] - mu[j]) * rs[j] * g[j] + b[j]);
    if (a.drop.thr) drop_apply8(a.drop, seed, (uint32_t)i0, z);
    if (a.res) {
      float r[8];
      ld8v(a.res, (int64_t)m * a.res_ld + c0, a.res_dt, r);
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] += r[j];
    }
    if (a.out_dt == TT2_BF16) st8nt(reinterpret_cast<bf16*>(a.out) + i0, z);
    else st8nt(reinterpret_cast<float*>(a.out) + i0, z);
  }
}

// dpre = d(pre-activation BN output): recompute z from y.
// keep: the element's dropout factor (0 or 1 / (1 - p); 1 without dropout)
TT2_DEV float bn_dpre(const BnArgs& a, float keep, float xh, float g, float b, float doutv) {
  const float z = act_f(a.act, xh * g + b);
  return doutv * keep * act_grad_from_out(a.act, z);
}
// the dropout factors of elements i0 .. i0 + 7 (drop_bits8: 4-5 hashes for 8 elements)
TT2_DEV void bn_keep8(const BnArgs& a, uint32_t seed, int64_t i0, float (&k)[8]) {
  const uint32_t bits = a.drop.thr ? drop_bits8(seed, a.drop.site, (uint32_t)i0, a.drop.thr) : 0xFFu;
  const float sc = a.drop.thr ? a.drop.scale : 1.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) k[j] = (bits >> j) & 1u ? sc : 0.f;
}

template <typename T, typename TD>
__global__ __launch_bounds__(NT) void bn_bwd_stats_kernel(BnArgs a) {
  __shared__ float red[2][NT][8];
  const int CG = a.C >> 3, nrl = NT / CG;
  const int cg = threadIdx.x % CG, rl = threadIdx.x / CG;
  const int c0 = cg * 8;
  const int r0 = blockIdx.x * a.rows_per, r1 = min(a.M, r0 + a.rows_per);
  const T* y = reinterpret_cast<const T*>(a.y);
  const TD* dout = reinterpret_cast<const TD*>(a.dout);
  const uint32_t seed = a.drop.thr ? *a.drop.seed : 0u;
  float s1[8], s2[8], mu[8], rs[8], g[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  col8(a.mean, c0, mu); col8(a.rstd, c0, rs); col8(a.gamma, c0, g); col8(a.beta, c0, b);
  if (rl < nrl) {
    for (int r = r0 + rl; r < r1; r += nrl) {
      const int64_t i0 = (int64_t)r * a.C + c0;
      float v[8], d[8], kp[8];
      ld8f(y + i0, v);
      ld8f(dout + i0, d);
      bn_keep8(a, seed, i0, kp);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = (v[j] - mu[j]) * rs[j];
        const float dp = bn_dpre(a, kp[j], xh, g[j], b[j], d[j]);
        s1[j] += dp;
        s2[j] += dp * xh;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { red[0][threadIdx.x][j] = s1[j]; red[1][threadIdx.x][j] = s2[j]; }
  __syncthreads();
  if (threadIdx.x < CG) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float S1 = 0.f, S2 = 0.f;
      for (int l = 0; l < nrl; ++l) { S1 += red[0][l * CG + cg][j]; S2 += red[1][l * CG + cg][j]; }
      a.part[((int64_t)blockIdx.x * 2 + 0) * a.C + c0 + j] = S1;
      a.part[((int64_t)blockIdx.x * 2 + 1) * a.C + c0 + j] = S2;
    }
  }
}

// backward: the chunk sums (sum dpre, sum dpre * xhat) of column block cb, in bn_fin64's order,
// into db / dg (LDS); write: also a.dbeta / a.dgamma (this rank's parameter gradients) and the
// SyncBN slots
struct BnBsumScratch { float red[2][BNC_G][BNC_COLS]; float db[BNC_COLS], dg[BNC_COLS]; };
TT2_DEV void bn_bsum64(const BnArgs& a, int cb, BnBsumScratch& S, bool write) {
  const int cl = threadIdx.x % BNC_COLS, g = threadIdx.x / BNC_COLS;
  const int c = cb * BNC_COLS + cl;
  const int cc = c < a.C ? c : 0;
  float s1 = 0.f, s2 = 0.f;
  int r = g;
  for (; r + 3 * BNC_G < a.R; r += 4 * BNC_G) {
    float v1[4], v2[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v1[u] = a.part[((int64_t)(r + u * BNC_G) * 2 + 0) * a.C + cc];
      v2[u] = a.part[((int64_t)(r + u * BNC_G) * 2 + 1) * a.C + cc];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) { s1 += v1[u]; s2 += v2[u]; }
  }
  for (; r < a.R; r += BNC_G) {
    s1 += a.part[((int64_t)r * 2 + 0) * a.C + cc];
    s2 += a.part[((int64_t)r * 2 + 1) * a.C + cc];
  }
  S.red[0][g][cl] = s1;
  S.red[1][g][cl] = s2;
  __syncthreads();
  if (g != 0) return;
  const float t1 = ((S.red[0][0][cl] + S.red[0][1][cl]) + S.red[0][2][cl]) + S.red[0][3][cl];
  const float t2 = ((S.red[1][0][cl] + S.red[1][1][cl]) + S.red[1][2][cl]) + S.red[1][3][cl];
  S.db[cl] = t1;
  S.dg[cl] = t2;
  if (!write || c >= a.C) return;
  a.dbeta[c] = t1;    // this rank's parameter gradients (the DP all-reduce sums them)
  a.dgamma[c] = t2;
  if (a.sync) {
    for (int r2 = 0; r2 < a.W; ++r2) {
      a.sync[((int64_t)r2 * BN_SLOT + 0) * a.C + c] = r2 == a.rank ? t1 : 0.f;
      a.sync[((int64_t)r2 * BN_SLOT + 1) * a.C + c] = r2 == a.rank ? t2 : 0.f;
      a.sync[((int64_t)r2 * BN_SLOT + 2) * a.C + c] = r2 == a.rank ? (float)a.M : 0.f;
      a.sync[((int64_t)r2 * BN_SLOT + 3) * a.C + c] = 0.f;
    }
  }
}

__global__ __launch_bounds__(NT) void bn_bwd_finalize_kernel(BnArgs a) {
  __shared__ BnBsumScratch S;
  bn_bsum64(a, blockIdx.x, S, true);
}

// one 8-column group of the backward apply (shared by bn_bwd_apply_kernel and the fused
// bn_bwd_apply_fin_kernel, so both compile the same expression: SyncBN at one rank stays
// bit-identical to plain BatchNorm)
TT2_DEV void bn_dy8(const BnArgs& a, const float (&v)[8], const float (&d)[8], const float (&kp)[8],
                    const float (&mu)[8], const float (&rs)[8], const float (&g)[8], const float (&b)[8],
                    const float (&db)[8], const float (&dg)[8], float invM, float (&o)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float xh = (v[j] - mu[j]) * rs[j];
    const float dp = bn_dpre(a, kp[j], xh, g[j], b[j], d[j]);
    o[j] = a.training ? g[j] * rs[j] * (dp - db[j] * invM - xh * dg[j] * invM) : g[j] * rs[j] * dp;
  }
}

template <typename T, typename TD>
__global__ __launch_bounds__(NT) void bn_bwd_apply_kernel(BnArgs a) {
  const int CG = a.C >> 3;
  const int nq = a.M * CG;
  const T* y = reinterpret_cast<const T*>(a.y);
  const TD* dout = reinterpret_cast<const TD*>(a.dout);
  const uint32_t seed = a.drop.thr ? *a.drop.seed : 0u;
  const float invM = a.inv_m ? *a.inv_m : 1.f / (float)a.Mtot;
  for (int q = blockIdx.x * NT + threadIdx.x; q < nq; q += gridDim.x * NT) {
    const int m = q / CG, c0 = (q - m * CG) * 8;
    const int64_t i0 = (int64_t)m * a.C + c0;
    float v[8], d[8], mu[8], rs[8], g[8], b[8], db[8], dg[8], o[8];
    ld8f(y + i0, v);
    ld8f(dout + i0, d);
    col8(a.mean, c0, mu); col8(a.rstd, c0, rs); col8(a.gamma, c0, g); col8(a.beta, c0, b);
    if (a.training) { col8(a.dbeta, c0, db); col8(a.dgamma, c0, dg); }
    float kp[8];
    bn_keep8(a, seed, i0, kp);
    bn_dy8(a, v, d, kp, mu, rs, g, b, db, dg, invM, o);
    st8nt(reinterpret_cast<T*>(a.dy) + i0, o);
  }
}

// Training apply with the finalize folded in: workgroup (column block x, row block y)
// first combines the chunk statistics of its 64 columns (bn_fin64 / bn_bsum64: the
// standalone finalize's code and order, ≈ 25 KB of chunk partials per workgroup), row block
// 0 writing mean / rstd / running statistics (forward) or dbeta / dgamma (backward), then
// applies them to its rows: one launch fewer per BatchNorm pass on the step's critical path.
// Threads: 8 column groups x 32 row lanes.
#ifndef BN_FUSED_FIN
#define BN_FUSED_FIN 1
#endif
TT2_DEV void bn_rows_of(const BnArgs& a, int& r0, int& r1) {
  const int per = (a.M + gridDim.y - 1) / gridDim.y;
  r0 = blockIdx.y * per;
  r1 = min(a.M, r0 + per);
}

template <typename T>
__global__ __launch_bounds__(NT) void bn_apply_fin_kernel(BnArgs a) {
  __shared__ BnFinScratch S;
  bn_fin64(a, blockIdx.x, S, blockIdx.y == 0);
  __syncthreads();
  const int cg = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int c0 = blockIdx.x * BNC_COLS + cg * 8;
  if (c0 >= a.C) return;
  int r0, r1;
  bn_rows_of(a, r0, r1);
  const T* y = reinterpret_cast<const T*>(a.y);
  const uint32_t seed = a.drop.thr ? *a.drop.seed : 0u;
  float mu[8], rs[8], g[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { mu[j] = S.mean[cg * 8 + j]; rs[j] = S.rstd[cg * 8 + j]; }
  col8(a.gamma, c0, g); col8(a.beta, c0, b);
  for (int m = r0 + rl; m < r1; m += NT / 8) {
    const int64_t i0 = (int64_t)m * a.C + c0;
    float v[8];
    ld8f(y + i0, v);
    float z[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = act_f(a.act, (v[j] - mu[j]) * rs[j] * g[j] + b[j]);
    if (a.drop.thr) drop_apply8(a.drop, seed, (uint32_t)i0, z);
    if (a.res) {
      float r[8];
      ld8v(a.res, (int64_t)m * a.res_ld + c0, a.res_dt, r);
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] += r[j];
    }
    if (a.out_dt == TT2_BF16) st8nt(reinterpret_cast<bf16*>(a.out) + i0, z);
    else st8nt(reinterpret_cast<float*>(a.out) + i0, z);
  }
}

// FIN = false: the sums are already final in a.dbeta / a.dgamma (SyncBatchNorm: the exchanged
// global sums) and are only staged; the rest is the same code, so SyncBN at one rank stays
// bit-identical to plain BatchNorm
template <typename T, typename TD, bool FIN>
__global__ __launch_bounds__(NT) void bn_bwd_apply_fin_kernel(BnArgs a) {
  __shared__ BnBsumScratch S;
  if constexpr (FIN) {
    bn_bsum64(a, blockIdx.x, S, blockIdx.y == 0);
  } else if (threadIdx.x < BNC_COLS) {
    const int c = blockIdx.x * BNC_COLS + threadIdx.x;
    S.db[threadIdx.x] = c < a.C ? a.dbeta[c] : 0.f;
    S.dg[threadIdx.x] = c < a.C ? a.dgamma[c] : 0.f;
  }
  __syncthreads();
  const int cg = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int c0 = blockIdx.x * BNC_COLS + cg * 8;
  if (c0 >= a.C) return;
  int r0, r1;
  bn_rows_of(a, r0, r1);
  const T* y = reinterpret_cast<const T*>(a.y);
  const TD* dout = reinterpret_cast<const TD*>(a.dout);
  const uint32_t seed = a.drop.thr ? *a.drop.seed : 0u;
  const float invM = a.inv_m ? *a.inv_m : 1.f / (float)a.Mtot;   // (bn_bwd_apply_kernel's form)
  float mu[8], rs[8], g[8], b[8], db[8], dg[8];
  col8(a.mean, c0, mu); col8(a.rstd, c0, rs); col8(a.gamma, c0, g); col8(a.beta, c0, b);
#pragma unroll
  for (int j = 0; j < 8; ++j) { db[j] = S.db[cg * 8 + j]; dg[j] = S.dg[cg * 8 + j]; }
  for (int m = r0 + rl; m < r1; m += NT / 8) {
    const int64_t i0 = (int64_t)m * a.C + c0;
    float v[8], d[8], o[8], kp[8];
    ld8f(y + i0, v);
    ld8f(dout + i0, d);
    bn_keep8(a, seed, i0, kp);
    bn_dy8(a, v, d, kp, mu, rs, g, b, db, dg, invM, o);
    st8nt(reinterpret_cast<T*>(a.dy) + i0, o);
  }
}

// (column blocks, row blocks) of the fused applies: about 512 workgroups, >= 32 rows each
dim3 bn_fin_grid(int m, int c) {
  const int ncb = (c + BNC_COLS - 1) / BNC_COLS;
  return dim3(ncb, std::max(1, std::min((m + 31) / 32, 512 / ncb)));
}

// host: the passes that the plain and the SyncBatchNorm entry points both launch, in the
// element type (and gradient type) of the request p
void bn_stats(const BnArgs& a, const tt2_bn_args* p, hipStream_t s) {
  by_dtype(p->dtype, [&](auto t) { hipLaunchKernelGGL(bn_stats_kernel<decltype(t)>, dim3(a.R), dim3(NT), 0, s, a); });
}
void bn_apply(const BnArgs& a, const tt2_bn_args* p, hipStream_t s) {
  const dim3 grid(grid_for((int64_t)p->m * p->c / 8));
  by_dtype(p->dtype, [&](auto t) { hipLaunchKernelGGL(bn_apply_kernel<decltype(t)>, grid, dim3(NT), 0, s, a); });
}
void bn_bwd_stats(const BnArgs& a, const tt2_bn_args* p, hipStream_t s) {
  by_dtype2(p->dtype, p->dout_dtype, [&](auto t, auto td) {
    hipLaunchKernelGGL((bn_bwd_stats_kernel<decltype(t), decltype(td)>), dim3(a.R), dim3(NT), 0, s, a);
  });
}
void bn_bwd_apply(const BnArgs& a, const tt2_bn_args* p, hipStream_t s) {
  const dim3 grid(grid_for((int64_t)p->m * p->c / 8));
  by_dtype2(p->dtype, p->dout_dtype, [&](auto t, auto td) {
    hipLaunchKernelGGL((bn_bwd_apply_kernel<decltype(t), decltype(td)>), grid, dim3(NT), 0, s, a);
  });
}
void bn_bwd_apply_fin(const BnArgs& a, const tt2_bn_args* p, bool fin, hipStream_t s) {
  const dim3 grid = bn_fin_grid(p->m, p->c);
  by_dtype2(p->dtype, p->dout_dtype, [&](auto t, auto td) {
    using T = decltype(t);
    using TD = decltype(td);
    if (fin) hipLaunchKernelGGL((bn_bwd_apply_fin_kernel<T, TD, true>), grid, dim3(NT), 0, s, a);
    else hipLaunchKernelGGL((bn_bwd_apply_fin_kernel<T, TD, false>), grid, dim3(NT), 0, s, a);
  });
}

}  // namespace

// rows per statistics chunk: at most TT2_BN_ROWS_PER_CHUNK, fewer for short inputs
// so there are >= ~256 chunk workgroups (one per CU) when the rows allow it
static int bn_rows_per(int m) {
  int rp = TT2_BN_ROWS_PER_CHUNK;
  while (rp > 8 && (m + rp - 1) / rp < 256) rp >>= 1;
  return rp;
}

static BnArgs bn_args(const tt2_bn_args* p) {
  BnArgs a{};
  a.y = p->y; a.dout = p->dout; a.res = p->res; a.out = p->out; a.dy = p->dy;
  a.gamma = p->gamma; a.beta = p->beta; a.mean = p->mean; a.rstd = p->rstd;
  a.run_mean = p->run_mean; a.run_var = p->run_var;
  a.part = reinterpret_cast<float*>(p->workspace);
  a.dgamma = p->dgamma; a.dbeta = p->dbeta;
  a.M = p->m; a.C = p->c; a.act = p->act; a.out_dt = p->out_dtype; a.res_dt = p->res_dtype;
  a.res_ld = p->res_ld > 0 ? p->res_ld : p->c;
  a.training = p->training;
  a.eps = p->eps; a.momentum = p->momentum;
  // stats_rows > 0: the workspace already holds the chunk moments (tt2_gemm col_stats)
  a.rows_per = p->stats_rows > 0 ? p->stats_rows : bn_rows_per(p->m);
  a.R = (p->m + a.rows_per - 1) / a.rows_per;
  a.y_dt = p->dtype == TT2_DT_BF16 ? TT2_BF16 : TT2_F32;
  // (an in-place forward, out == y, keeps absolute means: its apply overwrites the shifts)
  a.rel = p->stats_rows <= 0 && p->out != p->y;
  a.drop = drop_of(p);
  a.W = 1;
  a.Mtot = p->m;
  return a;
}

extern "C" size_t tt2_batchnorm_workspace_size(const tt2_bn_args* p) {
  const int rp = p->stats_rows > 0 ? p->stats_rows : bn_rows_per(p->m);
  const size_t R = (p->m + rp - 1) / rp;
  return R * 2 * p->c * sizeof(float);
}

static int bn_check(const tt2_bn_args* p, const char* what) {
  auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  if (p->c % 8 || p->c / 8 > NT) return tt2_set_error(TT2_E_INVALID, what);
  if (p->res && p->res_ld % 8) return tt2_set_error(TT2_E_INVALID, what);
  if (!al(p->y) || !al(p->out) || !al(p->res) || !al(p->dout) || !al(p->dy) || !al(p->gamma) || !al(p->beta) ||
      !al(p->mean) || !al(p->rstd) || !al(p->dgamma) || !al(p->dbeta))
    return tt2_set_error(TT2_E_INVALID, what);
  return TT2_OK;
}

extern "C" int tt2_batchnorm_fwd(const tt2_bn_args* p, hipStream_t s) {
  if (p->m <= 0) return TT2_OK;
  if (p->training && (!p->workspace || p->ws_bytes < tt2_batchnorm_workspace_size(p)))
    return tt2_set_error(TT2_E_INVALID, "tt2_batchnorm_fwd: workspace too small");
  if (bn_check(p, "tt2_batchnorm_fwd: C % 8, C <= 2048, res_ld % 8 and 16-B aligned buffers required"))
    return TT2_E_INVALID;
  const BnArgs a = bn_args(p);
  if (p->training && p->stats_rows <= 0) bn_stats(a, p, s);
  if (BN_FUSED_FIN && p->training) {   // the finalize inside the apply
    by_dtype(p->dtype, [&](auto t) {
      hipLaunchKernelGGL(bn_apply_fin_kernel<decltype(t)>, bn_fin_grid(p->m, p->c), dim3(NT), 0, s, a);
    });
    return tt2_check_launch(hipGetLastError(), "tt2_batchnorm_fwd");
  }
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((p->c + BNC_COLS - 1) / BNC_COLS), dim3(NT), 0, s, a);
  bn_apply(a, p, s);
  return tt2_check_launch(hipGetLastError(), "tt2_batchnorm_fwd");
}

extern "C" int tt2_batchnorm_bwd(const tt2_bn_args* p, hipStream_t s) {
  if (p->m <= 0) return TT2_OK;
  if (!p->workspace || p->ws_bytes < tt2_batchnorm_workspace_size(p))
    return tt2_set_error(TT2_E_INVALID, "tt2_batchnorm_bwd: workspace too small");
  if (bn_check(p, "tt2_batchnorm_bwd: C % 8, C <= 2048 and 16-B aligned buffers required")) return TT2_E_INVALID;
  const BnArgs a = bn_args(p);
  if (p->stats_rows <= 0) bn_bwd_stats(a, p, s);   // else: tt2_gemm bn_bwd's sums
  if (BN_FUSED_FIN && p->training) {   // the finalize inside the apply
    bn_bwd_apply_fin(a, p, true, s);
    return tt2_check_launch(hipGetLastError(), "tt2_batchnorm_bwd");
  }
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((p->c + BNC_COLS - 1) / BNC_COLS), dim3(NT), 0, s, a);
  bn_bwd_apply(a, p, s);
  return tt2_check_launch(hipGetLastError(), "tt2_batchnorm_bwd");
}

// ------------------------------------------------------------ SyncBatchNorm phases
// The caller SUM-all-reduces the first W * 4 * C floats of sync_buf between the phases
// (tt2/dist.py BnSync: RCCL in the captured step, or torch.distributed).  Every rank then
// holds the same slots and computes the same global statistics in the same order.
extern "C" size_t tt2_batchnorm_sync_size(const tt2_bn_args* p) {
  const int w = p->sync_world > 0 ? p->sync_world : 1;
  return ((size_t)(BN_SLOT * w + 2) * p->c + 4) * sizeof(float);   // + 1 / N (padded to 16 B)
}

static int bn_sync_check(const tt2_bn_args* p, const char* what) {
  if (bn_check(p, what)) return TT2_E_INVALID;
  if (!p->training || p->sync_world < 1 || p->sync_rank < 0 || p->sync_rank >= p->sync_world || !p->sync_buf ||
      (reinterpret_cast<uintptr_t>(p->sync_buf) & 15) || !p->workspace ||
      p->ws_bytes < tt2_batchnorm_workspace_size(p))
    return tt2_set_error(TT2_E_INVALID, what);
  return TT2_OK;
}

static BnArgs bn_sync_args(const tt2_bn_args* p) {
  BnArgs a = bn_args(p);
  a.sync = p->sync_buf;
  a.W = p->sync_world;
  a.rank = p->sync_rank;
  a.Mtot = 1;   // unused: the exchanged statistics carry each rank's row count (bn_*sync*_kernel, inv_m)
  return a;
}

extern "C" int tt2_batchnorm_fwd_stats(const tt2_bn_args* p, hipStream_t s) {
  if (p->m <= 0) return tt2_set_error(TT2_E_INVALID, "tt2_batchnorm_fwd_stats: m must be > 0");
  if (bn_sync_check(p, "tt2_batchnorm_fwd_stats: training, 1 <= sync_world, 0 <= sync_rank < sync_world, "
                       "16-B aligned sync_buf, workspace and the tt2_batchnorm_fwd layout rules required"))
    return TT2_E_INVALID;
  const BnArgs a = bn_sync_args(p);
  if (p->stats_rows <= 0) bn_stats(a, p, s);
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((p->c + BNC_COLS - 1) / BNC_COLS), dim3(NT), 0, s, a);
  return tt2_check_launch(hipGetLastError(), "tt2_batchnorm_fwd_stats");
}

extern "C" int tt2_batchnorm_fwd_apply(const tt2_bn_args* p, hipStream_t s) {
  if (p->m <= 0) return tt2_set_error(TT2_E_INVALID, "tt2_batchnorm_fwd_apply: m must be > 0");
  if (bn_sync_check(p, "tt2_batchnorm_fwd_apply: the tt2_batchnorm_fwd_stats arguments required"))
    return TT2_E_INVALID;
  const BnArgs a = bn_sync_args(p);
  hipLaunchKernelGGL(bn_sync_finalize_kernel, dim3((p->c + NT - 1) / NT), dim3(NT), 0, s, a);
  bn_apply(a, p, s);
  return tt2_check_launch(hipGetLastError(), "tt2_batchnorm_fwd_apply");
}

extern "C" int tt2_batchnorm_bwd_stats(const tt2_bn_args* p, hipStream_t s) {
  if (p->m <= 0) return tt2_set_error(TT2_E_INVALID, "tt2_batchnorm_bwd_stats: m must be > 0");
  if (bn_sync_check(p, "tt2_batchnorm_bwd_stats: the tt2_batchnorm_fwd_stats arguments required"))
    return TT2_E_INVALID;
  const BnArgs a = bn_sync_args(p);
  if (p->stats_rows <= 0) bn_bwd_stats(a, p, s);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((p->c + BNC_COLS - 1) / BNC_COLS), dim3(NT), 0, s, a);
  return tt2_check_launch(hipGetLastError(), "tt2_batchnorm_bwd_stats");
}

extern "C" int tt2_batchnorm_bwd_apply(const tt2_bn_args* p, hipStream_t s) {
  if (p->m <= 0) return tt2_set_error(TT2_E_INVALID, "tt2_batchnorm_bwd_apply: m must be > 0");
  if (bn_sync_check(p, "tt2_batchnorm_bwd_apply: the tt2_batchnorm_fwd_stats arguments required"))
    return TT2_E_INVALID;
  BnArgs a = bn_sync_args(p);
  hipLaunchKernelGGL(bn_bwd_sync_kernel, dim3((p->c + NT - 1) / NT), dim3(NT), 0, s, a);
  a.dbeta = a.sync + (int64_t)a.W * BN_SLOT * a.C;   // the apply reads the global sums and 1 / N
  a.dgamma = a.dbeta + a.C;
  a.inv_m = a.dgamma + a.C;
  if (BN_FUSED_FIN) {   // plain BatchNorm's apply code with the exchanged sums staged (one rank: bitwise equal)
    bn_bwd_apply_fin(a, p, false, s);
    return tt2_check_launch(hipGetLastError(), "tt2_batchnorm_bwd_apply");
  }
  bn_bwd_apply(a, p, s);
  return tt2_check_launch(hipGetLastError(), "tt2_batchnorm_bwd_apply");
}
