// attention_align.hip -- what reads the attention's by-products after the forward: the
// guided-attention loss reduction over the g rows, the alignment statistics (max_t P and its key
// per query row) and the durations kernel (attention_common.h has the map of the attention units).
#include "attention_v3.h"

// ---------------------------------------------------------- guided-attention loss
// One work group, fixed order (no atomics): sum of the selected layers' g rows over the guided
// heads, N = layers * heads * sum_b Tx_b Ty_b from the device lengths, the loss term, and kappa
// for the backward.  Rows past Ty_b and empty rows hold exactly 0, so whole rows are summed.
namespace {
constexpr int GL_NT = 1024;

template <int VEC>
__global__ __launch_bounds__(GL_NT) void guide_loss_kernel(tt2_guide_loss_args a) {
  __shared__ float red[GL_NT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int per = a.guide_heads * a.tq / VEC;   // guided heads of one batch element: contiguous
  const int64_t bstride = (int64_t)a.heads * a.tq;
  const int npair = a.n_layers * a.batch;
  float acc = 0.f;
  // wave w takes the (layer, batch) pairs w, w + 16, ...; its lanes stride the pair's rows
  for (int pr = w; pr < npair; pr += GL_NT / 64) {
    const int l = pr / a.batch, b = pr - l * a.batch;
    const float* src = a.rows[l] + b * bstride;
#pragma unroll 8
    for (int i = lane; i < per; i += 64) {
      if constexpr (VEC == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * i);
        acc += (v[0] + v[1]) + (v[2] + v[3]);
      } else {
        acc += src[i];
      }
    }
  }
  red[tid] = acc;
  __syncthreads();
  for (int st = GL_NT / 2; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  if (tid == 0) {
    double n = 0.0;
    for (int b = 0; b < a.batch; ++b) {
      n += (double)len_limit(a.tk, a.key_len, b) * (double)len_limit(a.tq, a.q_len, b);
    }
    n *= (double)a.n_layers * (double)a.guide_heads;
    const float term = n > 0.0 ? (float)((double)a.scale * (double)red[0] / n) : 0.f;
    *a.term = term;
    *a.coef = n > 0.0 ? (float)((double)a.scale * (double)a.grad_scale / n) : 0.f;
    if (a.loss_out && n > 0.0) a.loss_out[0] += term;
  }
}
}  // namespace

// ---------------------------------------------------------- alignment statistics
// max_t P[n, t] and its key index for every (layer, batch, head, query row) of forwards already
// run, from the saved log2-LSE: the row is already normalised, so one pass over Q K^T with a
// running (max score, key index) pair per lane is all there is (no online softmax, no V, no P V
// products, one exp2 per row).  tt2_align_durations turns them into focus rates and durations.
namespace {

// (v1, i1) replaces (v0, i0): greater value first, then the lower index (-1 = none loses)
TT2_DEV bool align_better(float v1, int i1, float v0, int i0) {
  return v1 > v0 || (v1 == v0 && (unsigned)i1 < (unsigned)i0);
}
TT2_DEV void align_store(const tt2_align_args& a, int li, int bh, int n, int qlim, float lse, float x, int idx) {
  // x: the row's greatest score in the log2 domain (scale * log2e folded in), rounded on its own as
  // the forward rounded it under the LSE.  contract(off): inlined into the MFMA kernel, x - lse was
  // contracted with the product behind x into one fma, which kept the product's rounding residual
  // (up to half an ulp of x, x about 1500 on sharp rows): max P came out as 1.0000423 where the
  // row's only key holds all the weight
#pragma clang fp contract(off)
  const bool ok = n < qlim && lse != INFINITY && idx >= 0;
  const int64_t o = ((int64_t)li * a.batch * a.heads + bh) * a.tq + n;
  a.pmax[o] = ok ? exp2f(x - lse) : 0.f;
  a.amax[o] = ok ? idx : -1;
}

// bf16: the v3 forward's score products (wave = 32 query rows on the lanes, 64-key K tiles in LDS
// with the chunk swizzle, double-buffered and register-staged), so a row's scores are the ones its
// LSE was built from.  Grid (B*H, row blocks, layers); 16 KB of LDS.
template <int NW>
__global__ __launch_bounds__(NW * 64) void attn_align3_kernel(tt2_align_args a) {
  constexpr int NTH = NW * 64, PER = Stage3<NTH>::PER, QB = 32 * NW;
  __shared__ __attribute__((aligned(16))) bf16 sK[2][64 * D];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ql = lane & 31, hi = lane >> 5;
  const int bh = blockIdx.x, b = bh / a.heads, h = bh % a.heads, li = blockIdx.z;
  const int q0 = blockIdx.y * QB, qw = q0 + 32 * w, qv = qw + ql;
  const RowBuf Q = row_buf(reinterpret_cast<const bf16*>(a.q[li]) + (int64_t)b * a.tq * a.q_ld + h * D, a.q_ld, a.tq);
  const RowBuf K = row_buf(reinterpret_cast<const bf16*>(a.k[li]) + (int64_t)b * a.tk * a.k_ld + h * D, a.k_ld, a.tk);

  bf16x8 fq[4];
  own_frags(fq, Q, qv, hi);
  const float lse = qv < a.tq ? a.lse[li][(int64_t)bh * a.tq + qv] : INFINITY;
  const int klim = len_limit(a.tk, a.key_len, b);
  const int ntile = klim > 0 ? (klim + 63) / 64 : 0;
  float best = -INFINITY;   // unscaled, as the forward takes its row maximum
  int bidx = -1;
  uint4 rk[PER];
  if (ntile > 0) {
    g2r3<NTH>(rk, K, 0, tid);
    r2s3<NTH>(rk, sK[0], tid);
  }
  __syncthreads();
  auto tile = [&](auto BUFC, int t) {
    constexpr int BUF = decltype(BUFC)::value;
    const int k0 = 64 * t;
    const bool more = t + 1 < ntile;
    if (more) g2r3<NTH>(rk, K, k0 + 64, tid);
    const bf16* cK = sK[BUF];
    if (qw < a.tq) {   // wave-uniform: the wave has a query row
      f32x16 s[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        zero16(s[kb]);
#pragma unroll
        for (int st = 0; st < 4; ++st) mma32(rowfrag(cK, 32 * kb + ql, 2 * st + hi), fq[st], s[kb]);
      }
      if (k0 + 64 > klim) {
        const int lim = klim - 1 - k0 - 4 * hi;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) s[kb][r] = 32 * kb + crow(r, 0) > lim ? -INFINITY : s[kb][r];
      }
      // the lane's keys in ascending order: a strict compare keeps the lowest index of a tie
      float tb = -INFINITY;
      int ti = 0;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool gt = s[kb][r] > tb;
          tb = gt ? s[kb][r] : tb;
          ti = gt ? 32 * kb + crow(r, 0) : ti;
        }
      if (tb > best) {
        best = tb;
        bidx = k0 + 4 * hi + ti;
      }
    }
    if (more) r2s3<NTH>(rk, sK[BUF ^ 1], tid);
    __syncthreads();
  };
  for (int t = 0; t < ntile; t += 2) {
    tile(std::integral_constant<int, 0>{}, t);
    if (t + 1 < ntile) tile(std::integral_constant<int, 1>{}, t + 1);
  }
  // the two lane halves hold disjoint keys of the same row
  const auto pv = __builtin_amdgcn_permlane32_swap(__float_as_uint(best), __float_as_uint(best), false, false);
  const auto pi = __builtin_amdgcn_permlane32_swap((unsigned)bidx, (unsigned)bidx, false, false);
  const float v0 = __uint_as_float(pv[0]), v1 = __uint_as_float(pv[1]);
  const int i0 = (int)pi[0], i1 = (int)pi[1];
  const bool second = align_better(v1, i1, v0, i0);
  const float bv = second ? v1 : v0;
  const int bi = second ? i1 : i0;
  if (qv < a.tq && hi == 0)
    align_store(a, li, bh, qv, len_limit(a.tq, a.q_len, b), lse, bv * (a.scale * LOG2E), bi);
}

// f32 and variant 1: one work group per (query row, batch*head, layer), attn_probs_kernel's scalar
// dot and its exp2f(dot * c - lse), then an LDS (max, index) reduction with the same tie rule
template <typename T>
__global__ __launch_bounds__(NT) void attn_align_kernel(tt2_align_args a) {
  __shared__ float sq[D];
  __shared__ float rv[NT];
  __shared__ int ri[NT];
  const int tid = threadIdx.x;
  const int qi = blockIdx.x, bh = blockIdx.y, li = blockIdx.z;
  const int b = bh / a.heads, h = bh % a.heads;
  const T* Q = reinterpret_cast<const T*>(a.q[li]) + ((int64_t)b * a.tq + qi) * a.q_ld + h * D;
  if (tid < D) sq[tid] = to_f32(Q[tid]);
  __syncthreads();
  const int klim = len_limit(a.tk, a.key_len, b);
  const float c = a.scale * LOG2E;
  float best = -INFINITY;
  int bidx = -1;
  for (int j = tid; j < klim; j += NT) {
    const T* Kr = reinterpret_cast<const T*>(a.k[li]) + ((int64_t)b * a.tk + j) * a.k_ld + h * D;
    float dot = 0.f;
#pragma unroll 8
    for (int d = 0; d < D; ++d) dot += sq[d] * to_f32(Kr[d]);
    const float x = dot * c;
    if (x > best) {
      best = x;
      bidx = j;
    }
  }
  rv[tid] = best;
  ri[tid] = bidx;
  __syncthreads();
  for (int st = NT / 2; st > 0; st >>= 1) {
    if (tid < st && align_better(rv[tid + st], ri[tid + st], rv[tid], ri[tid])) {
      rv[tid] = rv[tid + st];
      ri[tid] = ri[tid + st];
    }
    __syncthreads();
  }
  if (tid == 0)
    align_store(a, li, bh, qi, len_limit(a.tq, a.q_len, b), a.lse[li][(int64_t)bh * a.tq + qi], rv[0], ri[0]);
}

// One work group per utterance: the focus rate of every (layer, head) (wave w takes the pairs
// w, w + 16, ...; its lanes stride the valid rows, then a fixed shuffle tree), the head choice,
// and the chosen head's histogram of amax in LDS integer adds, AD_KEYS keys at a time.
constexpr int AD_NT = 1024, AD_KEYS = 2048, AD_PAIRS = tt2a::ALIGN_DUR_MAX_PAIRS;

__global__ __launch_bounds__(AD_NT) void align_dur_kernel(tt2_align_dur_args a) {
  __shared__ float sfocus[AD_PAIRS];
  __shared__ int hist[AD_KEYS];
  __shared__ int ssel;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x, H = a.heads;
  const int qlim = len_limit(a.tq, a.q_len, b);
  // (not len_limit: its clamp at 0 is not needed under t >= c0 below, and adds instructions)
  int klim = a.tk;
  if (a.key_len) klim = min(klim, a.key_len[b]);
  const int npair = a.n_layers * H;
  const float inv = qlim > 0 ? 1.f / (float)qlim : 0.f;
  for (int pr = w; pr < npair; pr += AD_NT / 64) {
    const int i = pr / H, h = pr - i * H;
    const float* src = a.pmax + (((int64_t)i * a.batch + b) * H + h) * a.tq;
    float acc = 0.f;
#pragma unroll 4
    for (int n = lane; n < qlim; n += 64) acc += src[n];
    acc = wave_sum(acc);
    if (lane == 0) {
      const float f = acc * inv;
      sfocus[pr] = f;
      a.focus[((int64_t)i * a.batch + b) * H + h] = f;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    if (a.mode == 0) {
      for (int pr = 1; pr < npair; ++pr)
        if (sfocus[pr] > sfocus[best]) best = pr;   // strict: the lowest flat index of a tie
    } else {
      best = a.sel_layer * H + a.sel_head;
    }
    ssel = best;
    a.sel[2 * b] = best / H;
    a.sel[2 * b + 1] = best % H;
    a.sel_focus[b] = sfocus[best];
  }
  __syncthreads();
  const int pr = ssel, i = pr / H, h = pr - i * H;
  const int32_t* am = a.amax + (((int64_t)i * a.batch + b) * H + h) * a.tq;
  for (int c0 = 0; c0 < a.tk; c0 += AD_KEYS) {
    const int nk = min(AD_KEYS, a.tk - c0);
    for (int t = tid; t < nk; t += AD_NT) hist[t] = 0;
    __syncthreads();
    for (int n = tid; n < qlim; n += AD_NT) {
      const int t = am[n];
      // (t < klim always holds for tt2_attn_align's output: a count never lands past key_len)
      if (t >= c0 && t < c0 + nk && t < klim) atomicAdd(&hist[t - c0], 1);
    }
    __syncthreads();
    for (int t = tid; t < nk; t += AD_NT) a.durations[(int64_t)b * a.tk + c0 + t] = hist[t];
    __syncthreads();
  }
}
}  // namespace

namespace tt2a {

void launch_guide_loss(const tt2_guide_loss_args* p, bool vec, hipStream_t s) {
  if (vec) hipLaunchKernelGGL(guide_loss_kernel<4>, dim3(1), dim3(GL_NT), 0, s, *p);
  else hipLaunchKernelGGL(guide_loss_kernel<1>, dim3(1), dim3(GL_NT), 0, s, *p);
}

void launch_align(const tt2_align_args* p, int nw, hipStream_t s) {
  const int BH = p->batch * p->heads;
  if (nw == 4) {
    hipLaunchKernelGGL(attn_align3_kernel<4>, dim3(BH, (p->tq + 127) / 128, p->n_layers), dim3(256), 0, s, *p);
  } else if (nw == 2) {
    hipLaunchKernelGGL(attn_align3_kernel<2>, dim3(BH, (p->tq + 63) / 64, p->n_layers), dim3(128), 0, s, *p);
  } else {
    const dim3 g(p->tq, BH, p->n_layers);
    if (p->dtype == TT2_DT_BF16) hipLaunchKernelGGL(attn_align_kernel<bf16>, g, dim3(NT), 0, s, *p);
    else hipLaunchKernelGGL(attn_align_kernel<float>, g, dim3(NT), 0, s, *p);
  }
}

void launch_align_dur(const tt2_align_dur_args* p, hipStream_t s) {
  hipLaunchKernelGGL(align_dur_kernel, dim3(p->batch), dim3(AD_NT), 0, s, *p);
}

}  // namespace tt2a
