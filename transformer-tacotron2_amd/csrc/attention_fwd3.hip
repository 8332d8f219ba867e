// attention_fwd3.hip -- the bf16 v3 attention forward (attention_v3.h describes the v3 products;
// attention_common.h has the map of the attention units).  Workgroup = NW waves = 32 NW query rows
// of one (batch, head), grid (batch*heads, query blocks): dispatch walks every (batch, head) of
// one row block before the next, so under a causal mask the heaviest blocks go first chip-wide
// (the blocks are reversed in-kernel).
#include "attention_v3.h"

namespace {

// in-kernel timeline hooks of the v3 forward (tools/attn_stamps.hip defines them; empty here)
#ifndef ATTN_STAMP
#define ATTN_STAMP(slot)
#endif

// G (guided, non-causal only): g = sum_t P W of the lane's query row accumulates beside l_r
// (same alpha, same two-half combine, same 1 / l) and is stored to a.grow
template <int NW, bool G>
__global__ __launch_bounds__(NW * 64) void attn_fwd3_kernel(ArgsT<G> a) {
  constexpr int NTH = NW * 64, PER = Stage3<NTH>::PER, QB = 32 * NW;
  __shared__ __attribute__((aligned(16))) bf16 sK[2][64 * D];
  __shared__ __attribute__((aligned(16))) bf16 sV[2][64 * D];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ql = lane & 31, hi = lane >> 5;
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;   // x = (batch, head): block index on y
  const int qblk = a.causal ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)blockIdx.y;   // heavy blocks first
  const int q0 = qblk * QB, qw = q0 + 32 * w, qv = qw + ql;
  ATTN_STAMP(0)
  const RowBuf Q = row_buf(reinterpret_cast<const bf16*>(a.q) + (int64_t)b * a.Tq * a.q_ld + h * D, a.q_ld, a.Tq);
  const RowBuf K = row_buf(reinterpret_cast<const bf16*>(a.k) + (int64_t)b * a.Tk * a.k_ld + h * D, a.k_ld, a.Tk);
  const RowBuf V = row_buf(reinterpret_cast<const bf16*>(a.v) + (int64_t)b * a.Tk * a.v_ld + h * D, a.v_ld, a.Tk);
  bf16* O = reinterpret_cast<bf16*>(a.out) + (int64_t)b * a.Tq * a.o_ld + h * D;

  bf16x8 fq[4];
  own_frags(fq, Q, qv, hi);
  // (no TT2_VMCNT0 here: with the forward's gated MFMAs ungated it measured 0.7-0.9 us slower
  // per launch)
  const float c = a.scale * LOG2E;
  float m_r = -INFINITY, l_r = 0.f;
  f32x16 o[2];
  zero16(o[0]);
  zero16(o[1]);

  const int klim = key_limit(a, b);
  int kend = klim;
  if (a.causal) kend = min(kend, q0 + QB);
  const int ntile = kend > 0 ? (kend + 63) / 64 : 0;
  Guide gd = {};
  float gk = 0.f;
  float g_r = 0.f, nq = 0.f;
  if constexpr (G) {
    gd = guide_of(a, b, h, klim);
    gk = a.gk;
    nq = (float)qv * gd.rq;
  }
  uint4 rk[PER], rv[PER];
  if (ntile > 0) {
    g2r3<NTH>(rk, K, 0, tid);
    g2r3<NTH>(rv, V, 0, tid);
    r2s3<NTH>(rk, sK[0], tid);
    r2s3<NTH>(rv, sV[0], tid);
  }
  __syncthreads();
  ATTN_STAMP(1)
  // one 64-key tile; BUF is compile-time so every LDS address is lane base + immediate
  auto tile = [&](auto BUFC, int t) {
    constexpr int BUF = decltype(BUFC)::value;
    const int k0 = 64 * t;
    const bool more = t + 1 < ntile;
    if (more) {
      g2r3<NTH>(rk, K, k0 + 64, tid);
      g2r3<NTH>(rv, V, k0 + 64, tid);
    }
    const bf16* cK = sK[BUF];
    const bf16* cV = sV[BUF];
    // wave-uniform: the wave has a query row (the last block of a head is partly past Tq:
    // 800 queries give 6.25 blocks of 128) and some key of the tile is visible
    if (qw < a.Tq && !(a.causal && k0 > qw + 31)) {
      f32x16 s[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        zero16(s[kb]);
#pragma unroll
        for (int st = 0; st < 4; ++st) mma32(rowfrag(cK, 32 * kb + ql, 2 * st + hi), fq[st], s[kb]);
      }
      if (k0 + 64 > klim || (a.causal && k0 + 63 > qw)) {
        // visible keys: key <= lim (one compare + select per score, no branches)
        const int lim = (a.causal ? min(klim - 1, qv) : klim - 1) - k0 - 4 * hi;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) s[kb][r] = 32 * kb + crow(r, 0) > lim ? -INFINITY : s[kb][r];
      }
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
      mx = xor32_max(mx);
      ATTN_STAMP(2 + 4 * t)
      const float mn = fmaxf(m_r, mx * c);
      const float base = mn == -INFINITY ? 0.f : mn;
      if (__any(mn != m_r)) {   // exact: skipped lanes would multiply by 1
        const float alpha = fast_exp2(m_r - base);
        l_r *= alpha;
        if constexpr (G) g_r *= alpha;
#pragma unroll
        for (int db = 0; db < 2; ++db) o[db] *= alpha;
      }
      m_r = mn;
      bf16x8 pf[2][2];
      float rs = 0.f;
      if (G && gd.sel) {   // block-uniform: the same p, and p W in f32 before p is rounded
        float gs = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          const float t0 = (float)(k0 + 32 * kb + 4 * hi);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float p = fast_exp2(fmaf(s[kb][r], c, -base));
            rs += p;
            gs = fmaf(p, guide_w<true>((t0 + (float)crow(r, 0)) * gd.rk, nq, gk), gs);
            pf[kb][r >> 3][r & 7] = (bf16)p;
          }
        }
        g_r += gs;
      } else {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float p = fast_exp2(fmaf(s[kb][r], c, -base));
            rs += p;
            pf[kb][r >> 3][r & 7] = (bf16)p;
          }
      }
      l_r += rs;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int db = 0; db < 2; ++db) mma32(trfrag(cV, 32 * kb + 16 * hh, db, lane), pf[kb][hh], o[db]);
    }
    ATTN_STAMP(3 + 4 * t)
    if (more) {
      r2s3<NTH>(rk, sK[BUF ^ 1], tid);
      r2s3<NTH>(rv, sV[BUF ^ 1], tid);
    }
    ATTN_STAMP(4 + 4 * t)
    __syncthreads();
    ATTN_STAMP(5 + 4 * t)
  };
  for (int t = 0; t < ntile; t += 2) {
    tile(std::integral_constant<int, 0>{}, t);
    if (t + 1 < ntile) tile(std::integral_constant<int, 1>{}, t + 1);
  }
  const float l = xor32_sum(l_r);
  if (qv < a.Tq) {
    store_rowT(O + (int64_t)qv * a.o_ld, o, l > 0.f ? 1.f / l : 0.f, hi);
    if (hi == 0) a.lse[(int64_t)bh * a.Tq + qv] = l > 0.f ? m_r + log2f(l) : INFINITY;
  }
  if constexpr (G) {
    const float gsum = xor32_sum(g_r);
    if (qv < a.Tq && hi == 0) a.grow[(int64_t)bh * a.Tq + qv] = gd.sel && qv < gd.qlim && l > 0.f ? gsum / l : 0.f;
  }
}

}  // namespace

namespace tt2a {

void launch_fwd3(const tt2_attn_args* p, const tt2_attn_guide* g, int nw, hipStream_t s) {
  const dim3 grid(p->batch * p->heads, (p->tq + 32 * nw - 1) / (32 * nw));
  with_args(p, g, [&](auto GC, const auto& a) {
    constexpr bool G = decltype(GC)::value;
    if (nw == 4) hipLaunchKernelGGL((attn_fwd3_kernel<4, G>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((attn_fwd3_kernel<2, G>), grid, dim3(128), 0, s, a);
  });
}

}  // namespace tt2a
