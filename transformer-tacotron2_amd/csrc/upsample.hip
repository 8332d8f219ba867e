// upsample.hip -- Gaussian upsampling (the soft length regulator of Non-Attentive Tacotron, Parallel
// Tacotron, JETS and ESPnet's VITS): phoneme states to frame states through softmax weights that are
// a function of two per-phoneme vectors and the frame index, with all four gradients.  tt2_capi.h
// states the definition.  A translation unit of its own.  The [frames, phonemes] weight matrix never
// reaches memory in either direction; no atomics, every order fixed.
//
//   gu_fwd_kernel     a work group per (utterance, 64 frames, 128 columns), a wave per 16 frames.
//                     Walks the phonemes in tiles of 32: centre / precision / bias and the h tile
//                     through LDS, the 16 x 32 scores computed in registers directly in the MFMA's
//                     A-operand layout (no trip through LDS), online softmax, y += P h on the
//                     16x16 MFMA (bf16: 16x16x32; f32: 8 x 16x16x4, exact f32 products).
//   gu_delta_kernel   delta[n] = sum_c dy[n][c] y[n][c], a wave per frame row, into the workspace.
//   gu_bwd_kernel     the attention dK/dV pass with phonemes as keys: a work group owns 32 phonemes
//                     (its h tile stays in LDS, every column of it) and walks the frames in tiles of
//                     32.  dW = dy h^T by MFMA (a 16 x 16 tile per wave, K = dim), W = exp(e - lse)
//                     and dE = W (dW - delta) in registers, the three scalar sums per lane, W^T to
//                     LDS and dh += W^T dy by MFMA (each wave a quarter of the column tiles).  An
//                     utterance of more than 128 frames is shared among up to 16 work groups per
//                     phoneme tile, which write f32 partials to the workspace.
//   gu_reduce_kernel  adds those partials in ascending order of their frames and rounds once.
// DESIGN.md 5.17 has the tiling, the register and LDS figures and the measurements.
#include <limits.h>

#include <algorithm>
#include <cmath>

#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {

constexpr int GU_THREADS = 256;
constexpr int FW_BN = 64;        // fwd: frames per work group (16 per wave)
constexpr int FW_DC = 128;       // fwd: columns per work group
constexpr int GU_BT = 32;        // phonemes per tile, both directions (the K of one bf16 MFMA)
constexpr int BW_BN = 32;        // bwd: frames per tile
constexpr int BW_LDW = 40;       // bwd: row stride of the W^T tile (elements; 16-byte rows)
constexpr int BW_JD = TT2_UPSAMPLE_MAX_DIM / 16 / 4;   // bwd: 16-column tiles of dh per wave at most
constexpr int BW_WALK = 4;       // bwd: frame tiles a work group walks at least; more work groups share an utterance's frames
constexpr int BW_SPLITS = 16;    // ... up to this many of them per phoneme tile

// How the backward shares the frames of an utterance among work groups, and its workspace: delta
// [batch, n_out], then (splits > 1) the f32 partials dh [splits, batch, tx, dim] and the three sums
// [splits, batch, 3, tx].  A function of the sizes alone, so the order of every sum is too.
struct gu_plan {
  int walk;          // frame tiles per work group
  int splits;        // work groups per (utterance, phoneme tile)
  size_t delta_off, dh_off, sums_off, bytes;
};

template <typename T> struct gu_pad { static constexpr int V = 16 / sizeof(T); };   // one chunk per row

TT2_DEV int gu_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// exp(x) through one v_exp_f32 with the product x log2(e) carried in two floats: the rounding of that
// product, |x| 2^-24 relative in the plain exp2 form, is what the weights' accuracy would otherwise be.
// 0 below the smallest float32 (and for x = -inf), NaN for NaN; x = -k ln 2 as float32 gives 2^-k exactly for the
// k the exact tests use (tests/_upsample_refs.py, assert_uniform_premise).
TT2_DEV float gu_exp(float x) {
  constexpr float L2E_HI = 1.4426950216293335f, L2E_LO = 1.9259629911266175e-8f, LN2F = 0.6931471805599453f;
  const float t = x * L2E_HI;
  const float err = __builtin_fmaf(x, L2E_HI, -t) + x * L2E_LO;
  const float r = __builtin_amdgcn_exp2f(t);
  return x < -104.f ? 0.f : __builtin_fmaf(r, err * LN2F, r);
}

// e = bias - prec (x - center)^2 with the roundings pinned (the difference, its square, one fused
// multiply-add): forward and backward must form the same bits, or W = exp(e - lse) is off by the
// rounding of e, 2^-24 |e| relative, where one phoneme holds all the weight and lse = e.
TT2_DEV float gu_score(float x, float c, float p, float b, float& d, float& q) {
  d = __fsub_rn(x, c);
  q = __fmul_rn(d, d);
  return __fmaf_rn(-p, q, b);
}

template <typename T> TT2_DEV void gu_frag_of(Frag8<T>& f, const float (&p)[8]);
template <> TT2_DEV void gu_frag_of(Frag8<bf16>& f, const float (&p)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) f.v[j] = (bf16)p[j];
}
template <> TT2_DEV void gu_frag_of(Frag8<float>& f, const float (&p)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) f.v[j] = p[j];
}

// ROWS x cols tile of a [.., ld] matrix to LDS (row stride lds): rows row0 .. row0 + ROWS - 1 below
// row_end and columns col0 .. col0 + cols - 1 below dim are read, everything else is zero.  vec: 16-byte
// chunks (the caller has checked base, strides and dim); cols is a multiple of a chunk.
template <typename T, int ROWS>
TT2_DEV void gu_tile_to_lds(T* s, int lds, const T* g, int64_t ld, int row0, int row_end, int col0, int cols, int dim,
                            bool vec, int tid) {
  constexpr int N = Chunk<T>::N;
  if (vec) {
    const int chunks = cols / N;
    for (int i = tid; i < ROWS * chunks; i += GU_THREADS) {
      const int r = i / chunks, c = (i - r * chunks) * N;
      ChunkV<T> v = zero_chunk<T>();
      if (row0 + r < row_end && col0 + c < dim) v = ld_chunk(g + (int64_t)(row0 + r) * ld + col0 + c);
      st_chunk(s + r * lds + c, v);
    }
  } else {
    for (int i = tid; i < ROWS * cols; i += GU_THREADS) {
      const int r = i / cols, c = i - r * cols;
      T v = from_f32<T>(0.f);
      if (row0 + r < row_end && col0 + c < dim) v = g[(int64_t)(row0 + r) * ld + col0 + c];
      s[r * lds + c] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------ forward
template <typename T>
__global__ __launch_bounds__(GU_THREADS) void gu_fwd_kernel(tt2_gauss_upsample_args a, int ftiles, int dchunks, int vec) {
  constexpr int LD = FW_DC + gu_pad<T>::V;
  __shared__ __attribute__((aligned(16))) T sH[GU_BT * LD];
  __shared__ float sC[GU_BT], sP[GU_BT], sB[GU_BT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int row_l = lane & 15, hq = lane >> 4;
  int bid = blockIdx.x;
  const int dc = bid % dchunks;
  bid /= dchunks;
  const int ft = bid % ftiles, b = bid / ftiles;
  const int txb = a.key_len ? gu_clamp(a.key_len[b], 0, a.tx) : a.tx;
  const int tyb = a.q_len ? gu_clamp(a.q_len[b], 0, a.n_out) : a.n_out;
  const int n0 = ft * FW_BN, c0 = dc * FW_DC;
  const T* H = static_cast<const T*>(a.h) + (int64_t)b * a.h_bs;
  T* Y = static_cast<T*>(a.y) + (int64_t)b * a.y_bs;
  const float* cen = a.center + (int64_t)b * a.p_ld;
  const float* pre = a.prec + (int64_t)b * a.p_ld;
  const float* bia = a.bias ? a.bias + (int64_t)b * a.p_ld : nullptr;

  // the lane's frame as the A operand's row, and its statistics (the same in the 4 lanes of a row)
  const float x = (float)(n0 + 16 * w + row_l) + a.offset;
  float m = -INFINITY, l = 0.f;
  f32x4 o[FW_DC / 16];
#pragma unroll
  for (int jd = 0; jd < FW_DC / 16; ++jd) o[jd] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (n0 < tyb) {
    for (int t0 = 0; t0 < txb; t0 += GU_BT) {
      __syncthreads();
      if (tid < GU_BT) {
        const int t = t0 + tid;
        const bool ok = t < txb;
        sC[tid] = ok ? cen[t] : 0.f;
        sP[tid] = ok ? pre[t] : 0.f;
        sB[tid] = ok && bia ? bia[t] : 0.f;
      }
      gu_tile_to_lds<T, GU_BT>(sH, LD, H, a.h_ld, t0, txb, c0, FW_DC, a.dim, vec != 0, tid);
      __syncthreads();
      // e[n][t] for t = t0 + 8 hq + j: the A fragment's own elements
      float e[8], mt = -INFINITY;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int tl = 8 * hq + j;
        float d, q;
        const float sc = gu_score(x, sC[tl], sP[tl], sB[tl], d, q);
        e[j] = t0 + tl < txb ? sc : -INFINITY;
        mt = fmaxf(mt, e[j]);
      }
      mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float mn = fmaxf(m, mt);
      const float base = mn == -INFINITY ? 0.f : mn;
      const float alpha = gu_exp(m - base);        // m = -inf: 0
      float p[8], rs = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        p[j] = gu_exp(e[j] - base);
        rs += p[j];
      }
      rs += __shfl_xor(rs, 16, 64);
      rs += __shfl_xor(rs, 32, 64);
      l = l * alpha + rs;
      m = mn;
      Frag8<T> fp;
      gu_frag_of<T>(fp, p);
      // the accumulator holds rows 4 hq + r: their factors come from the lanes that own those rows
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ar = __shfl(alpha, 4 * hq + r, 64);
#pragma unroll
        for (int jd = 0; jd < FW_DC / 16; ++jd) o[jd][r] *= ar;
      }
#pragma unroll
      for (int jd = 0; jd < FW_DC / 16; ++jd) {
        Frag8<T> fv;
        frag_col(fv, sH, LD, 8 * hq, 16 * jd, lane);
        mma16(fp, fv, o[jd]);
      }
    }
  }
  float lr[4], mr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lr[r] = __shfl(l, 4 * hq + r, 64);
    mr[r] = __shfl(m, 4 * hq + r, 64);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = n0 + 16 * w + 4 * hq + r;
    if (n >= a.n_out) continue;
    const bool live = n < tyb && txb > 0;
    const float inv = live ? 1.f / lr[r] : 0.f;
#pragma unroll
    for (int jd = 0; jd < FW_DC / 16; ++jd) {
      const int c = c0 + 16 * jd + row_l;
      if (c < a.dim) Y[(int64_t)n * a.y_ld + c] = from_f32<T>(live ? o[jd][r] * inv : 0.f);
    }
    if (dc == 0 && row_l == 0) a.lse[(int64_t)b * a.lse_ld + n] = live ? mr[r] + logf(lr[r]) : 0.f;
  }
}

// ----------------------------------------------------------------------------------------- backward
// delta[b][n] = sum_c dy[n][c] y[n][c] for n < Ty_b (0 past it): a wave per row, lanes stride the
// columns, then the wave's fixed tree.
template <typename T>
__global__ __launch_bounds__(GU_THREADS) void gu_delta_kernel(tt2_gauss_upsample_args a, float* delta, int rblocks) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x / (unsigned)rblocks;
  const int n = (blockIdx.x % (unsigned)rblocks) * 4 + (threadIdx.x >> 6);
  if (n >= a.n_out) return;
  const int tyb = a.q_len ? gu_clamp(a.q_len[b], 0, a.n_out) : a.n_out;
  float s = 0.f;
  if (n < tyb) {
    const T* dy = static_cast<const T*>(a.dy) + (int64_t)b * a.dy_bs + (int64_t)n * a.dy_ld;
    const T* y = static_cast<const T*>(a.y) + (int64_t)b * a.y_bs + (int64_t)n * a.y_ld;
    for (int c = lane; c < a.dim; c += 64) s += to_f32(dy[c]) * to_f32(y[c]);
    s = wave_sum(s);
  }
  if (lane == 0) delta[(int64_t)b * a.n_out + n] = s;
}

// the bytes of gu_bwd_kernel's LDS at column extent dp (dim rounded up to 32)
template <typename T> size_t gu_bwd_lds(int dp) {
  const size_t ldd = dp + gu_pad<T>::V;
  return (2 * GU_BT * ldd + GU_BT * BW_LDW) * sizeof(T) + (5 * GU_BT + 3 * 8 * GU_BT) * sizeof(float);
}

template <typename T>
__global__ __launch_bounds__(GU_THREADS) void gu_bwd_kernel(tt2_gauss_upsample_args a, const float* delta, float* part_dh,
                                                            float* part_sums, int ktiles, int splits, int walk, int dp,
                                                            int vec_h, int vec_dy) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gu_lds[];
  const int ldd = dp + gu_pad<T>::V;
  T* sH = reinterpret_cast<T*>(gu_lds);            // [32 phonemes][ldd]
  T* sDY = sH + GU_BT * ldd;                       // [32 frames][ldd]
  T* sW = sDY + BW_BN * ldd;                       // [32 phonemes][BW_LDW]: W^T of the tile
  float* sC = reinterpret_cast<float*>(sW + GU_BT * BW_LDW);
  float* sP = sC + GU_BT;
  float* sB = sP + GU_BT;
  float* sL = sB + GU_BT;                          // lse of the tile's frames
  float* sD = sL + BW_BN;                          // delta of the tile's frames
  float* sR = sD + BW_BN;                          // [3][8][32]: the scalar sums' partials

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int row_l = lane & 15, hq = lane >> 4;
  int bid = blockIdx.x;
  const int sp = bid % splits;
  bid /= splits;
  const int b = bid / ktiles;
  const int t0 = (bid % ktiles) * GU_BT;
  const int txb = a.key_len ? gu_clamp(a.key_len[b], 0, a.tx) : a.tx;
  const int tyb = a.q_len ? gu_clamp(a.q_len[b], 0, a.n_out) : a.n_out;
  // this work group's frames: tiles sp * walk .. (sp + 1) * walk - 1, cut at Ty_b
  const int64_t f_lo = (int64_t)sp * walk * BW_BN;
  const int f_begin = (int)min(f_lo, (int64_t)tyb), f_end = (int)min(f_lo + (int64_t)walk * BW_BN, (int64_t)tyb);
  const bool busy = f_begin < f_end && t0 < txb;
  const bool scalars = a.dcenter || a.dprec || a.dbias;
  const int ntile = dp / 16;                       // 16-column tiles of dh

  if (tid < GU_BT) {
    const int t = t0 + tid;
    const bool ok = t < txb && busy;
    sC[tid] = ok ? a.center[(int64_t)b * a.p_ld + t] : 0.f;
    sP[tid] = ok ? a.prec[(int64_t)b * a.p_ld + t] : 0.f;
    sB[tid] = ok && a.bias ? a.bias[(int64_t)b * a.p_ld + t] : 0.f;
  }
  if (busy)
    gu_tile_to_lds<T, GU_BT>(sH, ldd, static_cast<const T*>(a.h) + (int64_t)b * a.h_bs, a.h_ld, t0, txb, 0, dp, a.dim,
                             vec_h != 0, tid);
  __syncthreads();

  // dW tile of this wave: frames 16 fi + 4 hq + r, phoneme 16 ki + row_l
  const int fi = w >> 1, ki = w & 1;
  const int tl = 16 * ki + row_l;
  const bool t_live = t0 + tl < txb;
  const float ct = sC[tl], pt = sP[tl], bt = sB[tl];
  float s_b = 0.f, s_c = 0.f, s_p = 0.f;
  f32x4 acc[2][BW_JD];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int i = 0; i < BW_JD; ++i) acc[k][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const T* DY = static_cast<const T*>(a.dy) + (int64_t)b * a.dy_bs;
  for (int f0 = f_begin; f0 < f_end && busy; f0 += BW_BN) {
    __syncthreads();
    gu_tile_to_lds<T, BW_BN>(sDY, ldd, DY, a.dy_ld, f0, tyb, 0, dp, a.dim, vec_dy != 0, tid);
    if (tid < BW_BN) {
      const int n = f0 + tid;
      sL[tid] = n < tyb ? a.lse[(int64_t)b * a.lse_ld + n] : 0.f;
      sD[tid] = n < tyb && scalars ? delta[(int64_t)b * a.n_out + n] : 0.f;
    }
    __syncthreads();
    f32x4 dw = f32x4{0.f, 0.f, 0.f, 0.f};
    if (scalars) {
      for (int kk = 0; kk < dp; kk += 32) {
        Frag8<T> fa, fb;
        frag_row(fa, sDY + (16 * fi + row_l) * ldd + kk + 8 * hq);
        frag_row(fb, sH + tl * ldd + kk + 8 * hq);
        mma16(fa, fb, dw);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int nl = 16 * fi + 4 * hq + r, n = f0 + nl;
      float d, q;
      const float sc = gu_score((float)n + a.offset, ct, pt, bt, d, q);
      float wgt = 0.f, de = 0.f;
      if (t_live && n < tyb) {
        wgt = gu_exp(sc - sL[nl]);
        de = wgt * (dw[r] - sD[nl]);
      }
      s_b += de;
      s_c += de * (2.f * pt * d);
      s_p += de * q;
      sW[tl * BW_LDW + nl] = from_f32<T>(wgt);
    }
    if (a.dh) {
      __syncthreads();
      Frag8<T> fw[2];
      frag_row(fw[0], sW + row_l * BW_LDW + 8 * hq);
      frag_row(fw[1], sW + (16 + row_l) * BW_LDW + 8 * hq);
#pragma unroll
      for (int i = 0; i < BW_JD; ++i) {
        const int jd = w + 4 * i;
        if (jd < ntile) {
          Frag8<T> fv;
          frag_col(fv, sDY, ldd, 8 * hq, 16 * jd, lane);
          mma16(fw[0], fv, acc[0][i]);
          mma16(fw[1], fv, acc[1][i]);
        }
      }
    }
  }

  // one work group per phoneme tile: the outputs themselves; several: f32 partials for gu_reduce_kernel
  if (a.dh) {
    T* DH = static_cast<T*>(a.dh) + (int64_t)b * a.dh_bs;
    float* PH = part_dh + ((int64_t)sp * a.batch + b) * a.tx * a.dim;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = t0 + 16 * k + 4 * hq + r;
        if (t >= a.tx) continue;
#pragma unroll
        for (int i = 0; i < BW_JD; ++i) {
          const int c = 16 * (w + 4 * i) + row_l;
          if (c >= a.dim) continue;
          if (splits == 1) DH[(int64_t)t * a.dh_ld + c] = from_f32<T>(acc[k][i][r]);
          else PH[(int64_t)t * a.dim + c] = acc[k][i][r];
        }
      }
  }
  if (scalars) {
    // partial (fi, hq) of phoneme tl; added below in that order
    const int slot = (4 * fi + hq) * GU_BT + tl;
    sR[slot] = s_b;
    sR[8 * GU_BT + slot] = s_c;
    sR[16 * GU_BT + slot] = s_p;
    __syncthreads();
    if (tid < GU_BT && t0 + tid < a.tx) {
      float vb = 0.f, vc = 0.f, vp = 0.f;
      for (int k = 0; k < 8; ++k) {
        vb += sR[k * GU_BT + tid];
        vc += sR[(8 + k) * GU_BT + tid];
        vp += sR[(16 + k) * GU_BT + tid];
      }
      if (splits == 1) {
        const int64_t at = (int64_t)b * a.p_ld + t0 + tid;
        if (a.dbias) a.dbias[at] = vb;
        if (a.dcenter) a.dcenter[at] = vc;
        if (a.dprec) a.dprec[at] = 0.f - vp;
      } else {
        float* PS = part_sums + ((int64_t)sp * a.batch + b) * 3 * a.tx + t0 + tid;
        PS[0] = vb;
        PS[a.tx] = vc;
        PS[2 * (int64_t)a.tx] = vp;
      }
    }
  }
}

// The partials of `splits` work groups added in ascending order of their frames: dh (rounded once to
// the output dtype), then the three per-phoneme sums.
template <typename T>
__global__ __launch_bounds__(GU_THREADS) void gu_reduce_kernel(tt2_gauss_upsample_args a, const float* part_dh,
                                                               const float* part_sums, int splits) {
  const int64_t n_dh = a.dh ? (int64_t)a.batch * a.tx * a.dim : 0, n_s = (int64_t)a.batch * 3 * a.tx;
  const int64_t stride = (int64_t)gridDim.x * GU_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * GU_THREADS + threadIdx.x; i < n_dh + n_s; i += stride) {
    if (i < n_dh) {
      float v = 0.f;
      for (int s = 0; s < splits; ++s) v += part_dh[s * n_dh + i];
      const int c = (int)(i % a.dim);
      const int64_t row = i / a.dim;
      const int b = (int)(row / a.tx), t = (int)(row % a.tx);
      static_cast<T*>(a.dh)[(int64_t)b * a.dh_bs + (int64_t)t * a.dh_ld + c] = from_f32<T>(v);
    } else {
      const int64_t j = i - n_dh;
      const int t = (int)(j % a.tx), which = (int)(j / a.tx % 3), b = (int)(j / a.tx / 3);
      float* out = which == 0 ? a.dbias : which == 1 ? a.dcenter : a.dprec;
      if (!out) continue;
      float v = 0.f;
      for (int s = 0; s < splits; ++s) v += part_sums[s * n_s + j];
      out[(int64_t)b * a.p_ld + t] = which == 2 ? 0.f - v : v;
    }
  }
}

// -------------------------------------------------------------------------------------------- host
bool gu_chunks_ok(const void* base, int64_t ld, int64_t bs, int dim, int n) {
  return (reinterpret_cast<uintptr_t>(base) & 15) == 0 && ((ld | bs | (int64_t)dim) & (n - 1)) == 0;
}

// What fwd and bwd refuse alike
int gu_check(const char* who, const tt2_gauss_upsample_args* p) {
  if (!p) return tt2_invalid(who, "args required");
  if (p->batch < 0 || p->tx < 0 || p->n_out < 0 || p->dim < 0) return tt2_invalid(who, "negative batch / tx / n_out / dim");
  if (p->tx > TT2_REGULATE_MAX_PHONEMES) return tt2_invalid(who, "tx above TT2_REGULATE_MAX_PHONEMES");
  if (p->dim > TT2_UPSAMPLE_MAX_DIM) return tt2_invalid(who, "dim above TT2_UPSAMPLE_MAX_DIM");
  if (p->dtype != TT2_DT_F32 && p->dtype != TT2_DT_BF16) return tt2_invalid(who, "dtype must be TT2_DT_F32 or TT2_DT_BF16");
  if (p->h_ld < p->dim || p->y_ld < p->dim) return tt2_invalid(who, "h_ld or y_ld < dim");
  if (p->p_ld < p->tx) return tt2_invalid(who, "p_ld < tx");
  if (p->lse_ld < p->n_out) return tt2_invalid(who, "lse_ld < n_out");
  if (!(p->offset >= 0.f) || !std::isfinite(p->offset)) return tt2_invalid(who, "offset must be finite and >= 0");
  return TT2_OK;
}

gu_plan gu_plan_of(int batch, int tx, int n_out, int dim) {
  gu_plan g;
  const size_t b = (size_t)std::max(batch, 0), t = (size_t)std::max(tx, 0), n = (size_t)std::max(n_out, 0), d = (size_t)std::max(dim, 0);
  const size_t tiles = (n + BW_BN - 1) / BW_BN;
  g.walk = (int)std::max<size_t>(BW_WALK, (tiles + BW_SPLITS - 1) / BW_SPLITS);
  g.splits = (int)std::max<size_t>(1, (tiles + g.walk - 1) / g.walk);
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  g.delta_off = 0;
  if (b == 0 || t == 0 || n == 0) {      // nothing to do, or zeros to write: no workspace
    g.dh_off = g.sums_off = g.bytes = 0;
    return g;
  }
  g.dh_off = up(b * n * sizeof(float));
  g.sums_off = g.dh_off + (g.splits > 1 ? up((size_t)g.splits * b * t * d * sizeof(float)) : 0);
  g.bytes = g.sums_off + (g.splits > 1 ? up((size_t)g.splits * b * 3 * t * sizeof(float)) : 0);
  return g;
}

}  // namespace

extern "C" size_t tt2_gauss_upsample_bwd_workspace_size(int batch, int tx, int n_out, int dim) {
  return gu_plan_of(batch, tx, n_out, dim).bytes;
}

extern "C" int tt2_gauss_upsample_fwd(const tt2_gauss_upsample_args* p, hipStream_t s) {
  const char* who = "tt2_gauss_upsample_fwd";
  const int rc = gu_check(who, p);
  if (rc != TT2_OK) return rc;
  const int ftiles = (int)(((int64_t)p->n_out + FW_BN - 1) / FW_BN);
  const int dchunks = std::max(1, (p->dim + FW_DC - 1) / FW_DC);
  if ((int64_t)p->batch * ftiles * dchunks > INT_MAX) return tt2_invalid(who, "more than 2^31 - 1 work groups");
  if (p->batch == 0 || p->n_out == 0) return TT2_OK;
  if (!p->lse || (p->dim > 0 && !p->y)) return tt2_invalid(who, "y and lse required");
  if (p->tx > 0 && (!p->center || !p->prec || (p->dim > 0 && !p->h))) return tt2_invalid(who, "h, center and prec required");
  const dim3 grid((unsigned)(p->batch * ftiles * dchunks)), block(GU_THREADS);
  by_dtype(p->dtype, [&](auto t) {
    using T = decltype(t);
    const int vec = gu_chunks_ok(p->h, p->h_ld, p->h_bs, p->dim, Chunk<T>::N);
    hipLaunchKernelGGL(gu_fwd_kernel<T>, grid, block, 0, s, *p, ftiles, dchunks, vec);
  });
  return tt2_check_launch(hipGetLastError(), who);
}

extern "C" int tt2_gauss_upsample_bwd(const tt2_gauss_upsample_args* p, hipStream_t s) {
  const char* who = "tt2_gauss_upsample_bwd";
  const int rc = gu_check(who, p);
  if (rc != TT2_OK) return rc;
  if (p->dy_ld < p->dim || (p->dh && p->dh_ld < p->dim)) return tt2_invalid(who, "dy_ld or dh_ld < dim");
  const int ktiles = (p->tx + GU_BT - 1) / GU_BT;
  const int rblocks = (int)(((int64_t)p->n_out + 3) / 4);
  const gu_plan g = gu_plan_of(p->batch, p->tx, p->n_out, p->dim);
  if ((int64_t)p->batch * ktiles * g.splits > INT_MAX || (int64_t)p->batch * rblocks > INT_MAX)
    return tt2_invalid(who, "more than 2^31 - 1 work groups");
  const bool scalars = p->dcenter || p->dprec || p->dbias;
  const size_t need = g.bytes;
  const int wrc = tt2_need_workspace(who, p->workspace, p->workspace_bytes, need, 16);
  if (wrc != TT2_OK) return wrc;
  if (p->batch == 0 || p->tx == 0) return TT2_OK;
  if (!p->dh && !scalars) return tt2_invalid(who, "one of dh, dcenter, dprec and dbias required");
  if (p->n_out > 0 && (!p->center || !p->prec || !p->lse || (p->dim > 0 && (!p->h || !p->dy || !p->y))))
    return tt2_invalid(who, "h, center, prec, dy, y and lse required");
  char* ws = static_cast<char*>(p->workspace);
  float* delta = reinterpret_cast<float*>(ws + g.delta_off);
  float* part_dh = reinterpret_cast<float*>(ws + g.dh_off);
  float* part_sums = reinterpret_cast<float*>(ws + g.sums_off);
  const int dp = (p->dim + 31) / 32 * 32;
  hipError_t attr = hipSuccess;
  by_dtype(p->dtype, [&](auto t) {
    using T = decltype(t);
    if (scalars && p->n_out > 0)
      hipLaunchKernelGGL(gu_delta_kernel<T>, dim3((unsigned)(p->batch * rblocks)), dim3(GU_THREADS), 0, s, *p, delta, rblocks);
    const size_t lds = gu_bwd_lds<T>(dp);
    // LDS above the default 64 KB a kernel may ask for: raised on the current device at every such call
    // (the attribute is per device, and a host-side setting costs nothing beside the launches)
    if (lds > 64 * 1024 && attr == hipSuccess)
      attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&gu_bwd_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)gu_bwd_lds<T>(TT2_UPSAMPLE_MAX_DIM));
    if (attr != hipSuccess) return;
    const int vec_h = gu_chunks_ok(p->h, p->h_ld, p->h_bs, p->dim, Chunk<T>::N);
    const int vec_dy = gu_chunks_ok(p->dy, p->dy_ld, p->dy_bs, p->dim, Chunk<T>::N);
    hipLaunchKernelGGL(gu_bwd_kernel<T>, dim3((unsigned)(p->batch * ktiles * g.splits)), dim3(GU_THREADS), lds, s, *p, delta,
                       part_dh, part_sums, ktiles, g.splits, g.walk, dp, vec_h, vec_dy);
    if (g.splits > 1) {
      const int64_t items = (int64_t)p->batch * p->tx * ((p->dh ? p->dim : 0) + 3);
      hipLaunchKernelGGL(gu_reduce_kernel<T>, dim3((unsigned)grid_for(items, GU_THREADS, 4096)), dim3(GU_THREADS), 0, s, *p,
                         part_dh, part_sums, g.splits);
    }
  });
  if (attr != hipSuccess) return tt2_check_launch(attr, who);
  return tt2_check_launch(hipGetLastError(), who);
}
