// attention_bwd3.hip -- the bf16 v3 attention backward: the dQ and dK/dV bodies, their kernels and
// the fused launch of both (attention_v3.h describes the v3 products; attention_common.h has the
// map of the attention units).  Grids are (batch*heads, row blocks) as the forward's; under a
// causal mask the dQ blocks are reversed in-kernel and dK/dV block 0 is the heaviest.
#include "attention_v3.h"

namespace {

// s_waitcnt vmcnt(0) as the builtin (gfx9 encoding: vmcnt 0, expcnt 7, lgkmcnt 15), which the
// compiler's wait-count pass sees: registers loaded before a tile loop are then known complete.
// Without it the pass carried those loads' pending state around the loop and made each MFMA that
// reads them wait for the NEXT tile's prefetch loads issued just before (vmcnt(3)..vmcnt(0)),
// which put the prefetch's whole memory latency in front of every tile's first MFMAs.
#define TT2_VMCNT0() __builtin_amdgcn_s_waitcnt(0x0F70)

// dQ: wave = 32 queries (query on the lane), workgroup walks 64-key tiles in two
// 32-key halves.
template <int NW, bool G>
// dQ body (also the fused dQ + dK/dV launch): workgroup (bx, by) of a (B*H, ny) grid; smem
// holds sK[2][64 D] and sV[2][64 D]; publish: store delta = rowsum(dO * O) for a later dK/dV
TT2_DEV void attn_bwd_dq3_body(const ArgsT<G>& a, int bx, int by, int ny, char* smem, bool publish) {
  constexpr int NTH = NW * 64, PER = Stage3<NTH>::PER, QB = 32 * NW;
  bf16 (*sK)[64 * D] = reinterpret_cast<bf16 (*)[64 * D]>(smem);
  bf16 (*sV)[64 * D] = reinterpret_cast<bf16 (*)[64 * D]>(smem + 2 * 64 * D * sizeof(bf16));
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ql = lane & 31, hi = lane >> 5;
  const int bh = bx, b = bh / a.H, h = bh % a.H;   // x = (batch, head): block index on y
  const int qblk = a.causal ? ny - 1 - by : by;
  const int q0 = qblk * QB, qw = q0 + 32 * w, qv = qw + ql;
  const RowBuf Q = row_buf(reinterpret_cast<const bf16*>(a.q) + (int64_t)b * a.Tq * a.q_ld + h * D, a.q_ld, a.Tq);
  const RowBuf dO =
      row_buf(reinterpret_cast<const bf16*>(a.dout) + (int64_t)b * a.Tq * a.do_ld + h * D, a.do_ld, a.Tq);
  const RowBuf K = row_buf(reinterpret_cast<const bf16*>(a.k) + (int64_t)b * a.Tk * a.k_ld + h * D, a.k_ld, a.Tk);
  const RowBuf V = row_buf(reinterpret_cast<const bf16*>(a.v) + (int64_t)b * a.Tk * a.v_ld + h * D, a.v_ld, a.Tk);
  bf16* dQ = reinterpret_cast<bf16*>(a.dq) + (int64_t)b * a.Tq * a.dq_ld + h * D;

  const bool qok = qv < a.Tq;
  bf16x8 fq[4], fdo[4], fo[4];
  own_frags(fq, Q, qv, hi);
  own_frags(fdo, dO, qv, hi);
  // delta = rowsum(dO * O) of this lane's query row, computed here (the two lane halves hold
  // 32 dims each) and published for the dK / dV kernel that runs next on the stream
  const RowBuf Ob = row_buf(reinterpret_cast<const bf16*>(a.o) + (int64_t)b * a.Tq * a.o_ld + h * D, a.o_ld, a.Tq);
  own_frags(fo, Ob, qv, hi);
  const float lse = qok ? a.lse[(int64_t)bh * a.Tq + qv] : INFINITY;
  // G: dS = P (dP + kappa W - (delta + kappa g)) on the guided heads' valid rows; kap is 0 on
  // every other row, and the published delta carries the kappa g term for the dK / dV kernel
  Guide gd = {};
  float gk = 0.f;
  float kap = 0.f, nq = 0.f, kg = 0.f;
  if constexpr (G) {
    gd = guide_of(a, b, h, key_limit(a, b));
    gk = a.gk;
    if (gd.sel) {
      kap = qv < gd.qlim ? *a.gcoef : 0.f;
      nq = (float)qv * gd.rq;
      kg = qok ? kap * a.grow[(int64_t)bh * a.Tq + qv] : 0.f;
    }
  }
  TT2_VMCNT0();   // Q / dO / O fragments and the LSE are final before the tile loop
  float dsum = 0.f;
#pragma unroll
  for (int st = 0; st < 4; ++st)
#pragma unroll
    for (int j = 0; j < 8; ++j) dsum += (float)fdo[st][j] * (float)fo[st][j];
  dsum += __shfl_xor(dsum, 32, 64);
  if constexpr (G) dsum += kg;
  const float dl = qok ? dsum : 0.f;
  if (publish && qok && hi == 0) a.delta[(int64_t)bh * a.Tq + qv] = dsum;
  const float c = a.scale * LOG2E;
  f32x16 dq[2];
  zero16(dq[0]);
  zero16(dq[1]);

  const int klim = key_limit(a, b);
  int kend = klim;
  if (a.causal) kend = min(kend, q0 + QB);
  const int ntile = kend > 0 ? (kend + 63) / 64 : 0;
  uint4 rk[PER], rv[PER];
  if (ntile > 0) {
    g2r3<NTH>(rk, K, 0, tid);
    g2r3<NTH>(rv, V, 0, tid);
    r2s3<NTH>(rk, sK[0], tid);
    r2s3<NTH>(rv, sV[0], tid);
  }
  __syncthreads();
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
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int kb0 = k0 + 32 * kb;
      if (qw >= a.Tq || (a.causal && kb0 > qw + 31)) continue;   // wave-uniform (no query row, or masked)
      f32x16 s, dp;
      zero16(s);
      zero16(dp);
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        mma32(rowfrag(cK, 32 * kb + ql, 2 * st + hi), fq[st], s);
        mma32(rowfrag(cV, 32 * kb + ql, 2 * st + hi), fdo[st], dp);
      }
      float p[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) p[r] = fast_exp2(fmaf(s[r], c, -lse));
      if (kb0 + 32 > klim || (a.causal && kb0 + 31 > qw)) {   // wave-uniform: mask edge tiles only
        const int lim = (a.causal ? min(klim - 1, qv) : klim - 1) - kb0 - 4 * hi;
#pragma unroll
        for (int r = 0; r < 16; ++r) p[r] = crow(r, 0) > lim ? 0.f : p[r];
      }
      bf16x8 dsf[2];
      if (G && gd.sel) {   // block-uniform
        const float t0 = (float)(kb0 + 4 * hi);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float wgt = guide_w<true>((t0 + (float)crow(r, 0)) * gd.rk, nq, gk);
          dsf[r >> 3][r & 7] = (bf16)(p[r] * (fmaf(kap, wgt, dp[r]) - dl));
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) dsf[r >> 3][r & 7] = (bf16)(p[r] * (dp[r] - dl));
      }
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int db = 0; db < 2; ++db) mma32(trfrag(cK, 32 * kb + 16 * hh, db, lane), dsf[hh], dq[db]);
    }
    if (more) {
      r2s3<NTH>(rk, sK[BUF ^ 1], tid);
      r2s3<NTH>(rv, sV[BUF ^ 1], tid);
    }
    __syncthreads();
  };
  for (int t = 0; t < ntile; t += 2) {
    tile(std::integral_constant<int, 0>{}, t);
    if (t + 1 < ntile) tile(std::integral_constant<int, 1>{}, t + 1);
  }
  if (qok) store_rowT(dQ + (int64_t)qv * a.dq_ld, dq, a.scale, hi);
}

// dK, dV: wave = 32 keys (key on the lane), workgroup walks 64-query tiles in two
// 32-query halves.
template <int NW, bool G>
// dK / dV body: workgroup (bx, by) of a (B*H, key blocks) grid; smem holds sQ[2][64 D],
// sdO[2][64 D], sL[2][64], sDl[2][64]; reads delta (published by the dQ pass or attn_bwd_prep)
// self_delta: compute delta = rowsum(dO * O) of each staged query tile here (from the dO
// chunks already in registers and the matching O chunks) instead of reading a.delta
// G: dS gains kappa W on the guided heads' valid query rows.  The published delta already
// carries kappa g; with self_delta, kappa g of each staged row is loaded with its LSE and
// staged through sG[2][64] (after sDl)
TT2_DEV void attn_bwd_dkdv3_body(const ArgsT<G>& a, int bx, int by, char* smem, bool self_delta) {
  constexpr int NTH = NW * 64, PER = Stage3<NTH>::PER, KB = 32 * NW;
  bf16 (*sQ)[64 * D] = reinterpret_cast<bf16 (*)[64 * D]>(smem);
  bf16 (*sdO)[64 * D] = reinterpret_cast<bf16 (*)[64 * D]>(smem + 2 * 64 * D * sizeof(bf16));
  float (*sL)[64] = reinterpret_cast<float (*)[64]>(smem + 4 * 64 * D * sizeof(bf16));
  float (*sDl)[64] = reinterpret_cast<float (*)[64]>(smem + 4 * 64 * D * sizeof(bf16) + 2 * 64 * sizeof(float));
  float (*sG)[64] = reinterpret_cast<float (*)[64]>(smem + 4 * 64 * D * sizeof(bf16) + 4 * 64 * sizeof(float));
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kl = lane & 31, hi = lane >> 5;
  const int bh = bx, b = bh / a.H, h = bh % a.H;   // x = (batch, head): block index on y
  const int k0 = by * KB, kw = k0 + 32 * w, kv = kw + kl;   // causal: low blocks (heaviest) first
  const RowBuf Q = row_buf(reinterpret_cast<const bf16*>(a.q) + (int64_t)b * a.Tq * a.q_ld + h * D, a.q_ld, a.Tq);
  const RowBuf dO =
      row_buf(reinterpret_cast<const bf16*>(a.dout) + (int64_t)b * a.Tq * a.do_ld + h * D, a.do_ld, a.Tq);
  const RowBuf K = row_buf(reinterpret_cast<const bf16*>(a.k) + (int64_t)b * a.Tk * a.k_ld + h * D, a.k_ld, a.Tk);
  const RowBuf V = row_buf(reinterpret_cast<const bf16*>(a.v) + (int64_t)b * a.Tk * a.v_ld + h * D, a.v_ld, a.Tk);
  bf16* dK = reinterpret_cast<bf16*>(a.dk) + (int64_t)b * a.Tk * a.dk_ld + h * D;
  bf16* dV = reinterpret_cast<bf16*>(a.dv) + (int64_t)b * a.Tk * a.dv_ld + h * D;
  const float* LSE = a.lse + (int64_t)bh * a.Tq;
  const float* DL = a.delta + (int64_t)bh * a.Tq;
  const RowBuf Ob = row_buf(reinterpret_cast<const bf16*>(a.o) + (int64_t)b * a.Tq * a.o_ld + h * D, a.o_ld, a.Tq);

  bf16x8 fk[4], fv[4];
  own_frags(fk, K, kv, hi);
  own_frags(fv, V, kv, hi);
  TT2_VMCNT0();   // the K / V fragments are final before the tile loop (see TT2_VMCNT0)
  const float c = a.scale * LOG2E;
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    zero16(dk[db]);
    zero16(dv[db]);
  }
  const int klim = key_limit(a, b);
  const int qstart = a.causal ? (k0 / 64) * 64 : 0;
  const int ntile = k0 < klim && a.Tq > qstart ? (a.Tq - qstart + 63) / 64 : 0;
  Guide gd = {};
  float gk = 0.f;
  float kappa = 0.f, tkv = 0.f, g_n = 0.f;
  const float* GR = nullptr;
  if constexpr (G) {
    gd = guide_of(a, b, h, klim);
    gk = a.gk;
    kappa = gd.sel ? *a.gcoef : 0.f;
    tkv = (float)kv * gd.rk;
    GR = a.grow + (int64_t)bh * a.Tq;
  }
  uint4 rq[PER], rd[PER], ro[PER];
  // the next tile's LSE / delta are loaded with its Q / dO rows (stats_load) and stored to LDS
  // with them (stats): loaded at the store, they cost a memory round trip at every tile's end
  float lse_n = INFINITY, dl_n = 0.f;
  auto stats_load = [&](int qb) {
    if (tid < 64) {
      const int q = qb + tid;
      lse_n = q < a.Tq ? LSE[q] : INFINITY;
      if (!self_delta) dl_n = q < a.Tq ? DL[q] : 0.f;
      if constexpr (G) {
        if (self_delta && gd.sel) g_n = q < a.Tq ? kappa * GR[q] : 0.f;   // g is 0 on the rows past Ty
      }
    }
  };
  auto stats = [&](int buf, int qb) {
    (void)qb;
    if (tid < 64) {
      sL[buf][tid] = lse_n;
      if (!self_delta) sDl[buf][tid] = dl_n;
      if constexpr (G) {
        if (self_delta && gd.sel) sG[buf][tid] = g_n;
      }
    }
    if (self_delta) {   // chunk c = tid + NTH i is row c >> 3, 8 columns; the row's 8 chunks sit in 8 lanes
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        union { uint4 u; bf16x8 v; } x, y;
        x.u = rd[i];
        y.u = ro[i];
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d += (float)x.v[j] * (float)y.v[j];
        d += __shfl_xor(d, 1, 64);
        d += __shfl_xor(d, 2, 64);
        d += __shfl_xor(d, 4, 64);
        if ((tid & 7) == 0) sDl[buf][(tid + NTH * i) >> 3] = d;
      }
    }
  };
  if (ntile > 0) {
    g2r3<NTH>(rq, Q, qstart, tid);
    g2r3<NTH>(rd, dO, qstart, tid);
    if (self_delta) g2r3<NTH>(ro, Ob, qstart, tid);
    stats_load(qstart);
    r2s3<NTH>(rq, sQ[0], tid);
    r2s3<NTH>(rd, sdO[0], tid);
    stats(0, qstart);
  }
  __syncthreads();
  auto tile = [&](auto BUFC, int t) {
    constexpr int BUF = decltype(BUFC)::value;
    const int q0 = qstart + 64 * t;
    const bool more = t + 1 < ntile;
    if (more) {
      g2r3<NTH>(rq, Q, q0 + 64, tid);
      g2r3<NTH>(rd, dO, q0 + 64, tid);
      if (self_delta) g2r3<NTH>(ro, Ob, q0 + 64, tid);
      stats_load(q0 + 64);
    }
    const bf16* cQ = sQ[BUF];
    const bf16* cD = sdO[BUF];
    const float* cL = sL[BUF];
    const float* cDl = sDl[BUF];
    const float* cG = sG[BUF];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int qb0 = q0 + 32 * qb;
      if (kw >= klim || (a.causal && qb0 + 31 < kw)) continue;   // wave-uniform
      f32x16 s, dp;
      zero16(s);
      zero16(dp);
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        mma32(rowfrag(cQ, 32 * qb + kl, 2 * st + hi), fk[st], s);
        mma32(rowfrag(cD, 32 * qb + kl, 2 * st + hi), fv[st], dp);
      }
      float p[16], dl[16];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int qi = 32 * qb + 8 * rr + 4 * hi;
        const f32x4 L = *reinterpret_cast<const f32x4*>(cL + qi);
        const f32x4 Dl = *reinterpret_cast<const f32x4*>(cDl + qi);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          p[4 * rr + i] = fast_exp2(fmaf(s[4 * rr + i], c, -L[i]));
          dl[4 * rr + i] = Dl[i];
        }
        if constexpr (G) {
          if (self_delta && gd.sel) {
            const f32x4 Gv = *reinterpret_cast<const f32x4*>(cG + qi);
#pragma unroll
            for (int i = 0; i < 4; ++i) dl[4 * rr + i] += Gv[i];
          }
        }
      }
      if (kw + 32 > klim || (a.causal && qb0 < kw + 31)) {   // wave-uniform: mask edge tiles only
        // masked: query q < kv (causal) or every query when kv >= klim
        const int qlo = (kv >= klim ? 1 << 20 : (a.causal ? kv - qb0 : -1)) - 4 * hi;   // visible iff crow >= qlo
#pragma unroll
        for (int r = 0; r < 16; ++r) p[r] = crow(r, 0) < qlo ? 0.f : p[r];
      }
      bf16x8 pf[2], dsf[2];
      if (G && gd.sel) {   // block-uniform
        const float n0 = (float)(qb0 + 4 * hi);
        const int nval = gd.qlim - qb0 - 4 * hi;   // query row crow is valid iff crow < nval
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float wgt = guide_w<true>(tkv, (n0 + (float)crow(r, 0)) * gd.rq, gk);
          const float kq = crow(r, 0) < nval ? kappa : 0.f;
          pf[r >> 3][r & 7] = (bf16)p[r];
          dsf[r >> 3][r & 7] = (bf16)(p[r] * (fmaf(kq, wgt, dp[r]) - dl[r]));
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          pf[r >> 3][r & 7] = (bf16)p[r];
          dsf[r >> 3][r & 7] = (bf16)(p[r] * (dp[r] - dl[r]));
        }
      }
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          mma32(trfrag(cD, 32 * qb + 16 * hh, db, lane), pf[hh], dv[db]);
          mma32(trfrag(cQ, 32 * qb + 16 * hh, db, lane), dsf[hh], dk[db]);
        }
    }
    if (more) {
      r2s3<NTH>(rq, sQ[BUF ^ 1], tid);
      r2s3<NTH>(rd, sdO[BUF ^ 1], tid);
      stats(BUF ^ 1, q0 + 64);
    }
    __syncthreads();
  };
  for (int t = 0; t < ntile; t += 2) {
    tile(std::integral_constant<int, 0>{}, t);
    if (t + 1 < ntile) tile(std::integral_constant<int, 1>{}, t + 1);
  }
  if (kv < a.Tk) {
    store_rowT(dK + (int64_t)kv * a.dk_ld, dk, a.scale, hi);
    store_rowT(dV + (int64_t)kv * a.dv_ld, dv, 1.f, hi);
  }
}

constexpr int ATTN_BWD3_SMEM = 4 * 64 * D * sizeof(bf16) + 4 * 64 * sizeof(float);   // the larger (dK / dV) body
constexpr int ATTN_BWD3_SMEM_G = ATTN_BWD3_SMEM + 2 * 64 * sizeof(float);              // + sG (guided, self_delta)

template <int NW, bool G>
__global__ __launch_bounds__(NW * 64) void attn_bwd_dq3_kernel(ArgsT<G> a) {
  __shared__ __attribute__((aligned(16))) char smem[4 * 64 * D * sizeof(bf16)];
  attn_bwd_dq3_body<NW, G>(a, blockIdx.x, blockIdx.y, gridDim.y, smem, true);
}

template <int NW, bool G>
__global__ __launch_bounds__(NW * 64) void attn_bwd_dkdv3_kernel(ArgsT<G> a) {
  __shared__ __attribute__((aligned(16))) char smem[ATTN_BWD3_SMEM];   // (no sG: the published delta has kappa g)
  attn_bwd_dkdv3_body<NW, G>(a, blockIdx.x, blockIdx.y, smem, false);
}

// dQ and dK / dV in one launch (each computes delta itself): y < nkb are the key blocks, the
// rest the query blocks, so the (few, long) dK / dV workgroups of a short key range run
// beside the dQ workgroups instead of after them on a mostly idle chip
// (G: held to two waves per SIMD, the plain kernel's occupancy, without scratch; its natural
// allocation is 260 registers.  Measured 47.3 us held against 48.7 not held)
// G: the dQ blocks publish delta + kappa g although no block of this launch reads it, because
// tt2_capi.h promises it in the delta scratch after every guided backward (one store per row,
// before the tile loop); the plain launch leaves the scratch alone, as before.
template <int NW, bool G>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(G ? 2 : 1)))
void attn_bwd_fused3_kernel(ArgsT<G> a, int nkb) {
  __shared__ __attribute__((aligned(16))) char smem[G ? ATTN_BWD3_SMEM_G : ATTN_BWD3_SMEM];
  if ((int)blockIdx.y < nkb) attn_bwd_dkdv3_body<NW, G>(a, blockIdx.x, blockIdx.y, smem, true);
  else attn_bwd_dq3_body<NW, G>(a, blockIdx.x, (int)blockIdx.y - nkb, (int)gridDim.y - nkb, smem, G);
}

}  // namespace

namespace tt2a {

void launch_bwd_dq3(const tt2_attn_args* p, const tt2_attn_guide* g, int nw, hipStream_t s) {
  const dim3 grid(p->batch * p->heads, (p->tq + 32 * nw - 1) / (32 * nw));
  with_args(p, g, [&](auto GC, const auto& a) {
    constexpr bool G = decltype(GC)::value;
    if (nw == 4) hipLaunchKernelGGL((attn_bwd_dq3_kernel<4, G>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((attn_bwd_dq3_kernel<2, G>), grid, dim3(128), 0, s, a);
  });
}

void launch_bwd_dkdv3(const tt2_attn_args* p, const tt2_attn_guide* g, int nw, hipStream_t s) {
  const dim3 grid(p->batch * p->heads, (p->tk + 32 * nw - 1) / (32 * nw));
  with_args(p, g, [&](auto GC, const auto& a) {
    constexpr bool G = decltype(GC)::value;
    if (nw == 4) hipLaunchKernelGGL((attn_bwd_dkdv3_kernel<4, G>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((attn_bwd_dkdv3_kernel<2, G>), grid, dim3(128), 0, s, a);
  });
}

void launch_bwd_fused3(const tt2_attn_args* p, const tt2_attn_guide* g, int nkb, int nqb, hipStream_t s) {
  const dim3 grid(p->batch * p->heads, nkb + nqb);
  with_args(p, g, [&](auto GC, const auto& a) {
    hipLaunchKernelGGL((attn_bwd_fused3_kernel<4, decltype(GC)::value>), grid, dim3(256), 0, s, a, nkb);
  });
}

}  // namespace tt2a
