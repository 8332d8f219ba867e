// attention_v1.hip -- the generic attention kernels (f32, and bf16 variant 1) and the probabilities
// diagnostic (attention_common.h has the map of the attention units).
//
// Forward: workgroup = 4 waves = 64 query rows of one (batch, head); each wave owns 16 rows.
// S = Q K^T and O += P V run on MFMA 16x16 (bf16 16x16x32 or exact-f32 16x16x4), K / V / P tiles
// in LDS.  Row max / row sum are wave shuffles over the 16 lanes that hold one row's columns.
// Backward: attn_bwd_prep (delta), attn_bwd_dq, attn_bwd_dkdv on the same tiles.
#include "attention_common.h"

namespace {

template <typename T> struct LdsLd { static constexpr int V = D + Chunk<T>::N; };

// 8 contiguous elements from global (row pointer already offset), zero if !ok
template <typename T> TT2_DEV void frag_g(Frag8<T>& f, const T* p, bool ok);
template <> TT2_DEV void frag_g(Frag8<bf16>& f, const bf16* p, bool ok) {
  if (ok) f.v = *reinterpret_cast<const bf16x8*>(p);
  else { union { uint4 u; bf16x8 v; } z; z.u = make_uint4(0, 0, 0, 0); f.v = z.v; }
}
template <> TT2_DEV void frag_g(Frag8<float>& f, const float* p, bool ok) {
#pragma unroll
  for (int j = 0; j < 8; ++j) f.v[j] = ok ? p[j] : 0.f;
}

// [64 rows][64] tile of a strided global matrix -> LDS (rows >= nrows zeroed)
template <typename T>
TT2_DEV void tile_to_lds(T* s, const T* g, int64_t ld, int row0, int nrows, int tid) {
  constexpr int E = Chunk<T>::N;
  constexpr int CPR = D / E;
  constexpr int LD = LdsLd<T>::V;
#pragma unroll
  for (int c = tid; c < 64 * CPR; c += NT) {
    const int r = c / CPR, cc = c % CPR;
    ChunkV<T> v = (row0 + r < nrows) ? ld_chunk<T>(g + (int64_t)(row0 + r) * ld + cc * E) : zero_chunk<T>();
    st_chunk<T>(s + r * LD + cc * E, v);
  }
}

// ----------------------------------------------------------------- forward
template <typename T, bool G>
__global__ __launch_bounds__(NT) void attn_fwd_kernel(ArgsT<G> a) {
  constexpr int LD = LdsLd<T>::V;
  __shared__ __attribute__((aligned(16))) T sK[BKV * LD];
  __shared__ __attribute__((aligned(16))) T sV[BKV * LD];
  __shared__ __attribute__((aligned(16))) T sP[4 * 16 * LD];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
  const int q0 = blockIdx.x * BQ;
  const int row_l = lane & 15, hq = lane >> 4;
  const T* Q = reinterpret_cast<const T*>(a.q) + (int64_t)b * a.Tq * a.q_ld + h * D;
  const T* K = reinterpret_cast<const T*>(a.k) + (int64_t)b * a.Tk * a.k_ld + h * D;
  const T* V = reinterpret_cast<const T*>(a.v) + (int64_t)b * a.Tk * a.v_ld + h * D;
  T* O = reinterpret_cast<T*>(a.out) + (int64_t)b * a.Tq * a.o_ld + h * D;

  // Q fragments: row q0 + 16w + (lane&15), d = 32*kk + 8*(lane>>4) + j
  Frag8<T> fq[2];
  {
    const int qr = q0 + 16 * w + row_l;
    const bool ok = qr < a.Tq;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) frag_g(fq[kk], Q + (int64_t)(ok ? qr : 0) * a.q_ld + 32 * kk + 8 * hq, ok);
  }
  const float c = a.scale * LOG2E;
  float m_r[4], l_r[4];
  f32x4 o[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_r[r] = -INFINITY; l_r[r] = 0.f; }
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int klim = key_limit(a, b);
  int kend = klim;
  if (a.causal) kend = min(kend, q0 + BQ);
  T* myP = sP + w * 16 * LD;
  Guide gd = {};
  float gk = 0.f;
  float g_r[4] = {0.f, 0.f, 0.f, 0.f};   // G: sum_t p W beside l_r
  if constexpr (G) {
    gd = guide_of(a, b, h, klim);
    gk = a.gk;
  }

  for (int k0 = 0; k0 < kend; k0 += BKV) {
    __syncthreads();
    tile_to_lds<T>(sK, K, a.k_ld, k0, a.Tk, tid);
    tile_to_lds<T>(sV, V, a.v_ld, k0, a.Tk, tid);
    __syncthreads();

    f32x4 s[4];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      s[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        Frag8<T> fk;
        frag_row(fk, sK + (16 * jb + row_l) * LD + 32 * kk + 8 * hq);
        mma16(fq[kk], fk, s[jb]);
      }
    }
    // scale + mask; lane holds S[row 4*hq + r][key 16*jb + (lane&15)]
    float mt[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) mt[r] = -INFINITY;
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      const int key = k0 + 16 * jb + row_l;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qr = q0 + 16 * w + 4 * hq + r;
        float x = s[jb][r] * c;
        if (key >= klim || (a.causal && key > qr)) x = -INFINITY;
        s[jb][r] = x;
        mt[r] = fmaxf(mt[r], x);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mn = fmaxf(m_r[r], max16(mt[r]));
      const float base = mn == -INFINITY ? 0.f : mn;
      const float alpha = exp2f(m_r[r] - base);  // m_r = -inf -> 0
      float rs = 0.f;
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        const float p = exp2f(s[jb][r] - base);
        s[jb][r] = p;
        rs += p;
      }
      l_r[r] = l_r[r] * alpha + sum16(rs);
      m_r[r] = mn;
      if constexpr (G) {
        if (gd.sel) {   // p W in f32, before p is rounded for the P V product
          const float nq = (float)(q0 + 16 * w + 4 * hq + r) * gd.rq;
          float gs = 0.f;
#pragma unroll
          for (int jb = 0; jb < 4; ++jb)
            gs += s[jb][r] * guide_w<false>((float)(k0 + 16 * jb + row_l) * gd.rk, nq, gk);
          g_r[r] = g_r[r] * alpha + sum16(gs);
        }
      }
#pragma unroll
      for (int jd = 0; jd < 4; ++jd) o[jd][r] *= alpha;
    }
    // P -> LDS (wave private), then O += P V
#pragma unroll
    for (int jb = 0; jb < 4; ++jb)
#pragma unroll
      for (int r = 0; r < 4; ++r) myP[(4 * hq + r) * LD + 16 * jb + row_l] = from_f32<T>(s[jb][r]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      Frag8<T> fp;
      frag_row(fp, myP + row_l * LD + 32 * kk + 8 * hq);
#pragma unroll
      for (int jd = 0; jd < 4; ++jd) {
        Frag8<T> fv;
        frag_col(fv, sV, LD, 32 * kk + 8 * hq, 16 * jd, lane);
        mma16(fp, fv, o[jd]);
      }
    }
  }

  // finalize
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qr = q0 + 16 * w + 4 * hq + r;
    if (qr >= a.Tq) continue;
    const float inv = l_r[r] > 0.f ? 1.f / l_r[r] : 0.f;
#pragma unroll
    for (int jd = 0; jd < 4; ++jd) O[(int64_t)qr * a.o_ld + 16 * jd + row_l] = from_f32<T>(o[jd][r] * inv);
    if (row_l == 0)
      a.lse[(int64_t)bh * a.Tq + qr] = l_r[r] > 0.f ? m_r[r] + log2f(l_r[r]) : INFINITY;
    if constexpr (G) {
      if (row_l == 0)
        a.grow[(int64_t)bh * a.Tq + qr] = gd.sel && qr < gd.qlim && l_r[r] > 0.f ? g_r[r] / l_r[r] : 0.f;
    }
  }
}

// ---------------------------------------------------------------- backward
// a * b rounded once, never contracted into a following add or subtract
TT2_DEV float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// delta[bh, t] = sum_d dO[t, h*64 + d] * O[t, h*64 + d]; one wave per (b, t) row, all heads.
// G: delta + kappa g for the guided rows, so dS = P (dP + kappa W - delta) downstream
template <typename T, bool G>
__global__ __launch_bounds__(NT) void attn_bwd_prep_kernel(ArgsT<G> a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);  // b * Tq + t
  if (row >= a.B * a.Tq) return;
  const int b = row / a.Tq, t = row % a.Tq;
  const T* O = reinterpret_cast<const T*>(a.o) + (int64_t)row * a.o_ld;
  const T* dO = reinterpret_cast<const T*>(a.dout) + (int64_t)row * a.do_ld;
  for (int h0 = 0; h0 < a.H; h0 += 8) {
    // lane covers head h0 + lane/8, elements 8*(lane%8) .. +8
    const int h = h0 + (lane >> 3);
    float s = 0.f;
    if (h < a.H) {
      const int off = h * D + 8 * (lane & 7);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += to_f32(O[off + j]) * to_f32(dO[off + j]);
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if constexpr (G) {
      if ((lane & 7) == 0 && h < a.H) {
        const Guide gd = guide_of(a, b, h, key_limit(a, b));
        if (gd.sel && t < gd.qlim) s += *a.gcoef * a.grow[((int64_t)b * a.H + h) * a.Tq + t];
      }
    }
    if ((lane & 7) == 0 && h < a.H) a.delta[((int64_t)b * a.H + h) * a.Tq + t] = s;
  }
}

template <typename T, bool G>
__global__ __launch_bounds__(NT) void attn_bwd_dq_kernel(ArgsT<G> a) {
  constexpr int LD = LdsLd<T>::V;
  __shared__ __attribute__((aligned(16))) T sK[BKV * LD];
  __shared__ __attribute__((aligned(16))) T sV[BKV * LD];
  __shared__ __attribute__((aligned(16))) T sP[4 * 16 * LD];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
  const int q0 = blockIdx.x * BQ;
  const int row_l = lane & 15, hq = lane >> 4;
  const T* Q = reinterpret_cast<const T*>(a.q) + (int64_t)b * a.Tq * a.q_ld + h * D;
  const T* dO = reinterpret_cast<const T*>(a.dout) + (int64_t)b * a.Tq * a.do_ld + h * D;
  const T* K = reinterpret_cast<const T*>(a.k) + (int64_t)b * a.Tk * a.k_ld + h * D;
  const T* V = reinterpret_cast<const T*>(a.v) + (int64_t)b * a.Tk * a.v_ld + h * D;
  T* dQ = reinterpret_cast<T*>(a.dq) + (int64_t)b * a.Tq * a.dq_ld + h * D;

  Frag8<T> fq[2], fdo[2];
  {
    const int qr = q0 + 16 * w + row_l;
    const bool ok = qr < a.Tq;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      frag_g(fq[kk], Q + (int64_t)(ok ? qr : 0) * a.q_ld + 32 * kk + 8 * hq, ok);
      frag_g(fdo[kk], dO + (int64_t)(ok ? qr : 0) * a.do_ld + 32 * kk + 8 * hq, ok);
    }
  }
  float lse[4], dl[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qr = q0 + 16 * w + 4 * hq + r;
    lse[r] = qr < a.Tq ? a.lse[(int64_t)bh * a.Tq + qr] : INFINITY;
    dl[r] = qr < a.Tq ? a.delta[(int64_t)bh * a.Tq + qr] : 0.f;
  }
  const float c = a.scale * LOG2E;
  f32x4 dq[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dq[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int klim = key_limit(a, b);
  int kend = klim;
  if (a.causal) kend = min(kend, q0 + BQ);
  T* myP = sP + w * 16 * LD;
  Guide gd = {};
  float gk = 0.f;
  float kap[4] = {0.f, 0.f, 0.f, 0.f}, nq[4] = {0.f, 0.f, 0.f, 0.f};   // G: kappa of the valid rows (else 0), n / Ty
  if constexpr (G) {
    gd = guide_of(a, b, h, klim);
    gk = a.gk;
    const float kappa = gd.sel ? *a.gcoef : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qr = q0 + 16 * w + 4 * hq + r;
      kap[r] = qr < gd.qlim ? kappa : 0.f;
      nq[r] = (float)qr * gd.rq;
    }
  }

  for (int k0 = 0; k0 < kend; k0 += BKV) {
    __syncthreads();
    tile_to_lds<T>(sK, K, a.k_ld, k0, a.Tk, tid);
    tile_to_lds<T>(sV, V, a.v_ld, k0, a.Tk, tid);
    __syncthreads();
    f32x4 s[4], dp[4];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      s[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        Frag8<T> fk, fv;
        frag_row(fk, sK + (16 * jb + row_l) * LD + 32 * kk + 8 * hq);
        frag_row(fv, sV + (16 * jb + row_l) * LD + 32 * kk + 8 * hq);
        mma16(fq[kk], fk, s[jb]);
        mma16(fdo[kk], fv, dp[jb]);
      }
    }
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      const int key = k0 + 16 * jb + row_l;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qr = q0 + 16 * w + 4 * hq + r;
        // the product rounded as the forward rounded it (its max and LSE come from RN(s c)): left to
        // contract into fma(s, c, -lse), P comes back off by ulp(s c) / 2, 4e-5 at a score of 2000
        float p = exp2f(mul_rn(s[jb][r], c) - lse[r]);
        if (key >= klim || (a.causal && key > qr)) p = 0.f;
        float ds;
        if (G && gd.sel) ds = p * (fmaf(kap[r], guide_w<false>((float)key * gd.rk, nq[r], gk), dp[jb][r]) - dl[r]);
        else ds = p * (dp[jb][r] - dl[r]);
        myP[(4 * hq + r) * LD + 16 * jb + row_l] = from_f32<T>(ds);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      Frag8<T> fds;
      frag_row(fds, myP + row_l * LD + 32 * kk + 8 * hq);
#pragma unroll
      for (int jd = 0; jd < 4; ++jd) {
        Frag8<T> fk;
        frag_col(fk, sK, LD, 32 * kk + 8 * hq, 16 * jd, lane);
        mma16(fds, fk, dq[jd]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qr = q0 + 16 * w + 4 * hq + r;
    if (qr >= a.Tq) continue;
#pragma unroll
    for (int jd = 0; jd < 4; ++jd) dQ[(int64_t)qr * a.dq_ld + 16 * jd + row_l] = from_f32<T>(dq[jd][r] * a.scale);
  }
}

template <typename T, bool G>
__global__ __launch_bounds__(NT) void attn_bwd_dkdv_kernel(ArgsT<G> a) {
  constexpr int LD = LdsLd<T>::V;
  __shared__ __attribute__((aligned(16))) T sQ[BQ * LD];
  __shared__ __attribute__((aligned(16))) T sdO[BQ * LD];
  __shared__ __attribute__((aligned(16))) T sP[4 * 16 * LD];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
  const int k0 = blockIdx.x * BKV;
  const int row_l = lane & 15, hq = lane >> 4;
  const T* Q = reinterpret_cast<const T*>(a.q) + (int64_t)b * a.Tq * a.q_ld + h * D;
  const T* dO = reinterpret_cast<const T*>(a.dout) + (int64_t)b * a.Tq * a.do_ld + h * D;
  const T* K = reinterpret_cast<const T*>(a.k) + (int64_t)b * a.Tk * a.k_ld + h * D;
  const T* V = reinterpret_cast<const T*>(a.v) + (int64_t)b * a.Tk * a.v_ld + h * D;
  T* dK = reinterpret_cast<T*>(a.dk) + (int64_t)b * a.Tk * a.dk_ld + h * D;
  T* dV = reinterpret_cast<T*>(a.dv) + (int64_t)b * a.Tk * a.dv_ld + h * D;

  const int klim = key_limit(a, b);
  // this wave's keys: k0 + 16w + (lane&15) as MFMA rows
  Frag8<T> fk[2], fv[2];
  {
    const int kr = k0 + 16 * w + row_l;
    const bool ok = kr < a.Tk;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      frag_g(fk[kk], K + (int64_t)(ok ? kr : 0) * a.k_ld + 32 * kk + 8 * hq, ok);
      frag_g(fv[kk], V + (int64_t)(ok ? kr : 0) * a.v_ld + 32 * kk + 8 * hq, ok);
    }
  }
  const float c = a.scale * LOG2E;
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { dk[j] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  T* myP = sP + w * 16 * LD;
  const bool block_live = k0 < klim;
  const int qstart = (a.causal ? (k0 / BQ) * BQ : 0);
  Guide gd = {};
  float gk = 0.f;
  float kappa = 0.f, tk[4] = {0.f, 0.f, 0.f, 0.f};   // G: t / Tx of the lane's keys
  if constexpr (G) {
    gd = guide_of(a, b, h, klim);
    gk = a.gk;
    kappa = gd.sel ? *a.gcoef : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) tk[r] = (float)(k0 + 16 * w + 4 * hq + r) * gd.rk;
  }

  for (int q0 = qstart; block_live && q0 < a.Tq; q0 += BQ) {
    __syncthreads();
    tile_to_lds<T>(sQ, Q, a.q_ld, q0, a.Tq, tid);
    tile_to_lds<T>(sdO, dO, a.do_ld, q0, a.Tq, tid);
    __syncthreads();
    // lane holds S^T[key 4*hq + r][query 16*jb + (lane&15)]
    float lse[4], dl[4];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      const int qc = q0 + 16 * jb + row_l;
      lse[jb] = qc < a.Tq ? a.lse[(int64_t)bh * a.Tq + qc] : INFINITY;
      dl[jb] = qc < a.Tq ? a.delta[(int64_t)bh * a.Tq + qc] : 0.f;
    }
    f32x4 s[4], dp[4];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      s[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        Frag8<T> fqq, fdd;
        frag_row(fqq, sQ + (16 * jb + row_l) * LD + 32 * kk + 8 * hq);
        frag_row(fdd, sdO + (16 * jb + row_l) * LD + 32 * kk + 8 * hq);
        mma16(fk[kk], fqq, s[jb]);
        mma16(fv[kk], fdd, dp[jb]);
      }
    }
    float pv[4][4];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      const int qc = q0 + 16 * jb + row_l;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + 16 * w + 4 * hq + r;
        float p = exp2f(mul_rn(s[jb][r], c) - lse[jb]);   // RN(s c) as in the forward (see attn_bwd_dq_kernel)
        if (key >= klim || (a.causal && key > qc) || qc >= a.Tq) p = 0.f;
        pv[jb][r] = p;
        myP[(4 * hq + r) * LD + 16 * jb + row_l] = from_f32<T>(p);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // dV += P^T dO
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      Frag8<T> fp;
      frag_row(fp, myP + row_l * LD + 32 * kk + 8 * hq);
#pragma unroll
      for (int jd = 0; jd < 4; ++jd) {
        Frag8<T> fd;
        frag_col(fd, sdO, LD, 32 * kk + 8 * hq, 16 * jd, lane);
        mma16(fp, fd, dv[jd]);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // dS^T = P^T (dP^T - delta) -> LDS, dK += dS^T Q
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      const int qc = q0 + 16 * jb + row_l;
      const float kq = G && qc < gd.qlim ? kappa : 0.f, nq = (float)qc * gd.rq;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float ds;
        if (G && gd.sel) ds = pv[jb][r] * (fmaf(kq, guide_w<false>(tk[r], nq, gk), dp[jb][r]) - dl[jb]);
        else ds = pv[jb][r] * (dp[jb][r] - dl[jb]);
        myP[(4 * hq + r) * LD + 16 * jb + row_l] = from_f32<T>(ds);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      Frag8<T> fds;
      frag_row(fds, myP + row_l * LD + 32 * kk + 8 * hq);
#pragma unroll
      for (int jd = 0; jd < 4; ++jd) {
        Frag8<T> fqq;
        frag_col(fqq, sQ, LD, 32 * kk + 8 * hq, 16 * jd, lane);
        mma16(fds, fqq, dk[jd]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kr = k0 + 16 * w + 4 * hq + r;
    if (kr >= a.Tk) continue;
#pragma unroll
    for (int jd = 0; jd < 4; ++jd) {
      dK[(int64_t)kr * a.dk_ld + 16 * jd + row_l] = from_f32<T>(dk[jd][r] * a.scale);
      dV[(int64_t)kr * a.dv_ld + 16 * jd + row_l] = from_f32<T>(dv[jd][r]);
    }
  }
}

}  // namespace

// ------------------------------------------------------------ diagnostics
// Attention probabilities of a forward already run (alignment diagnostics, SURVEY 8(f)
// row 3): P[bh][q][j] = exp2(s * scale * log2e - lse[bh][q]) from the saved log2-LSE,
// 0 where masked.  One workgroup per (batch*head, query row); off the training path.
template <typename T>
__global__ __launch_bounds__(NT) void attn_probs_kernel(AttnArgs a, float* probs) {
  __shared__ float sq[D];
  const int bh = blockIdx.y, qi = blockIdx.x;
  const int b = bh / a.H, h = bh % a.H;
  const T* Q = reinterpret_cast<const T*>(a.q) + ((int64_t)b * a.Tq + qi) * a.q_ld + h * D;
  if (threadIdx.x < D) sq[threadIdx.x] = to_f32(Q[threadIdx.x]);
  __syncthreads();
  const float lse = a.lse[(int64_t)bh * a.Tq + qi];
  const int klim = key_limit(a, b);
  const float c = a.scale * LOG2E;
  float* out = probs + ((int64_t)bh * a.Tq + qi) * a.Tk;
  for (int j = threadIdx.x; j < a.Tk; j += NT) {
    float v = 0.f;
    if (j < klim && (!a.causal || j <= qi)) {
      const T* Kr = reinterpret_cast<const T*>(a.k) + ((int64_t)b * a.Tk + j) * a.k_ld + h * D;
      float dot = 0.f;
#pragma unroll 8
      for (int d = 0; d < D; ++d) dot += sq[d] * to_f32(Kr[d]);
      v = exp2f(dot * c - lse);
    }
    out[j] = v;
  }
}

namespace tt2a {

void launch_fwd1(const tt2_attn_args* p, const tt2_attn_guide* g, hipStream_t s) {
  const dim3 grid((p->tq + BQ - 1) / BQ, p->batch * p->heads);
  with_args(p, g, [&](auto GC, const auto& a) {
    constexpr bool G = decltype(GC)::value;
    if (p->dtype == TT2_DT_BF16) hipLaunchKernelGGL((attn_fwd_kernel<bf16, G>), grid, dim3(NT), 0, s, a);
    else hipLaunchKernelGGL((attn_fwd_kernel<float, G>), grid, dim3(NT), 0, s, a);
  });
}

void launch_bwd_prep1(const tt2_attn_args* p, const tt2_attn_guide* g, hipStream_t s) {
  const dim3 grid((p->batch * p->tq + 3) / 4);
  with_args(p, g, [&](auto GC, const auto& a) {
    constexpr bool G = decltype(GC)::value;
    if (p->dtype == TT2_DT_BF16) hipLaunchKernelGGL((attn_bwd_prep_kernel<bf16, G>), grid, dim3(NT), 0, s, a);
    else hipLaunchKernelGGL((attn_bwd_prep_kernel<float, G>), grid, dim3(NT), 0, s, a);
  });
}

void launch_bwd_dq1(const tt2_attn_args* p, const tt2_attn_guide* g, hipStream_t s) {
  const dim3 grid((p->tq + BQ - 1) / BQ, p->batch * p->heads);
  with_args(p, g, [&](auto GC, const auto& a) {
    constexpr bool G = decltype(GC)::value;
    if (p->dtype == TT2_DT_BF16) hipLaunchKernelGGL((attn_bwd_dq_kernel<bf16, G>), grid, dim3(NT), 0, s, a);
    else hipLaunchKernelGGL((attn_bwd_dq_kernel<float, G>), grid, dim3(NT), 0, s, a);
  });
}

void launch_bwd_dkdv1(const tt2_attn_args* p, const tt2_attn_guide* g, hipStream_t s) {
  const dim3 grid((p->tk + BKV - 1) / BKV, p->batch * p->heads);
  with_args(p, g, [&](auto GC, const auto& a) {
    constexpr bool G = decltype(GC)::value;
    if (p->dtype == TT2_DT_BF16) hipLaunchKernelGGL((attn_bwd_dkdv_kernel<bf16, G>), grid, dim3(NT), 0, s, a);
    else hipLaunchKernelGGL((attn_bwd_dkdv_kernel<float, G>), grid, dim3(NT), 0, s, a);
  });
}

void launch_probs(const tt2_attn_args* p, float* probs, hipStream_t s) {
  const AttnArgs a = to_args<false>(p);
  const dim3 grid(p->tq, p->batch * p->heads);
  if (p->dtype == TT2_DT_BF16) hipLaunchKernelGGL(attn_probs_kernel<bf16>, grid, dim3(NT), 0, s, a, probs);
  else hipLaunchKernelGGL(attn_probs_kernel<float>, grid, dim3(NT), 0, s, a, probs);
}

}  // namespace tt2a
