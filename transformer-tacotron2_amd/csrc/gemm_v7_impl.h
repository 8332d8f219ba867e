// gemm_v7_impl.h -- v7, the warp-specialised 256 x 128 kernel (the auto plan's default), its grouped
// form, the two split-K reducers (the plain one also follows a split v1 / v2 launch) and
// tt2_gemm_grouped / _fin / _ex.  Compiled in gemm_v2v7v11.hip.
// A source, not a header: it defines kernels, non-inline functions and (v7) extern "C" entry
// points, so exactly one translation unit may include it (gemm_v2v7v11.hip).  It carries the .h
// suffix only so that the build's header scan rebuilds that unit when it changes.
#pragma once
#include "gemm_v7.h"

namespace {

// =====================================================================================
// v7 (bf16, plain operands): warp-specialised 256 x 128 tile.  In v6 every wave both
// issues LDS-DMA copies and multiplies; an LDS-DMA issue stalls its wave while the
// CU's address path (~64 B/clk) drains, so the MFMA stream of all 8 waves stops for
// ~700 cycles per K step (in-kernel s_memtime timeline).  Here 4 loader waves (one per
// SIMD) do nothing but copy, three K steps deep into a 3-stage ring, and 8 MFMA waves
// (4 M x 2 N, 64 x 64 each) only read fragments and multiply; one s_barrier per step
// hands stages over (loaders wait their copies of step t+1 with a counted vmcnt first).
// The MFMA operands are swapped (D = B A^T: each lane holds 4 consecutive C columns of
// one row) and v_permlane16_swap pairs adjacent column blocks, so every lane stores 8
// consecutive columns of a row straight from registers -- no LDS round trip for C.
// ksum (row sums of an M-contiguous A): the wn == 0 waves multiply their A fragments by an
// all-ones fragment (one extra MFMA each).
// =====================================================================================
#ifndef G7_REG   // the loader waves stage plain operand steps through VGPRs (1) or by LDS-DMA (0):
#define G7_REG 0   // bit-identical, 3-17 % slower per GEMM, step 6.58 -> 6.88 ms
#endif

// Register-staged copies into their ring slots (the LDS image LDS-DMA would have written).
template <int NI>
TT2_DEV void g7_put(const u32x4 (&r)[NI], char* lds, int lane, int lw) {
#pragma unroll
  for (int i = 0; i < NI; ++i) *reinterpret_cast<u32x4*>(lds + (lw * NI + i) * 1024 + lane * 16) = r[i];
}

constexpr int G7_MAXP = 8;
// A deferred LayerNorm backward's column-sum finalize (tt2_ln_args with defer_finalize) that
// rides in the group's split-K reduce launch: part[nb][3][C] -> dg / db / dd (each
// = gb * old + sum when gb != 0), one wave per output column, fixed order.
struct G7Fin {
  const float* part;
  float* dst[3];
  float gb;
  int nb, C;
};
struct G7Group {
  G7Prob p[G7_MAXP];
  int np, items;
  int ibase;   // first item of this launch (a capped grid: several launches)
  G7Fin fin;   // nb == 0: none
  int fin_only;   // the reduce launch holds only the finalize plane (no split problem to reduce)
};
constexpr int G7_FIN_WAVES = 4;   // columns per 256-thread reduce block

// whole-row store of the LDS C image (all 768 threads; 4 rows x 256 B per wave instruction).
// Nontemporal: C streams out during the epilogue instead of sitting dirty in L2 until the
// end-of-kernel write-back (the consumer kernel reads it from the Infinity Cache either way).
// With E.cstats (a BatchNorm's statistics fused into the producing GEMM), the stored values'
// column moments over the tile's rows ride along: every thread keeps one 8-column chunk
// (768 % 16 == 0) and sums (v - k), (v - k)^2 over its rows with k = the tile's row 0 (the
// statistics kernel's shift), the 4 lanes of a chunk in a wave combine by shuffles, the 12 waves
// through the free ring stage, and 128 threads write the chunk's mean and M2 per column.
// With E.bnb.part (the BatchNorm backward's statistics pass fused into the GEMM that produces its
// dout), each thread sums, over the same rows and chunk, dpre = dout * keep * act'(z) and
// dpre * xhat exactly as bn_bwd_stats_kernel forms them per element (its y rows are loaded
// before the store loop, all in flight), then the same reduction writes plain chunk sums.
// SM (compile time, so the plain kernels carry none of it): 0 store only, 1 col_stats, 2 bn_bwd sums.
template <int SM>
TT2_DEV void g7_store_c(const G7Prob& P, char* smem, int m0, int n0, int nkt) {
  bf16* C = reinterpret_cast<bf16*>(P.E.c);
  constexpr bool st = SM == 1, sb = SM == 2;
  const int c = threadIdx.x & 15;
  float k[8], s1[8], s2[8];
  if (st) bf16x8_unpack(*reinterpret_cast<const u32x4*>(smem + g7_img_row(nkt, 0) + (c << 4)), k);
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  constexpr int NR = (256 * 16 + G7_NT - 1) / G7_NT;   // rows per thread (6; the last only for some)
  constexpr int YB = NR / 2;   // y rows in flight per batch (two batches: register pressure)
  u32x4 yv[YB];
  float mu[8], rs[8], ga[8], be[8];
  uint32_t seed = 0;
  auto load_y = [&](int i0) {
#pragma unroll
    for (int i = 0; i < YB; ++i) {
      const int r = (threadIdx.x >> 4) + (G7_NT / 16) * (i0 + i), m = min(m0 + r, P.M - 1);
      yv[i] = r < 256 ? *reinterpret_cast<const u32x4*>(P.E.bnb.y + (int64_t)m * P.N + n0 + 8 * c)
                      : u32x4{0, 0, 0, 0};
    }
  };
  if constexpr (sb) {
    const int n = n0 + 8 * c;
    load_y(0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mu[j] = P.E.bnb.mean[n + j]; rs[j] = P.E.bnb.rstd[n + j];
      ga[j] = P.E.bnb.gamma[n + j]; be[j] = P.E.bnb.beta[n + j];
    }
    seed = P.E.bnb.drop.thr ? *P.E.bnb.drop.seed : 0u;
  }
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    if constexpr (sb) {
      if (i == YB) load_y(YB);
    }
    const int id = threadIdx.x + G7_NT * i;
    if (id >= 256 * 16) break;
    const int r = id >> 4, m = m0 + r, n = n0 + 8 * c;
    if (m < P.M && n < P.N) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(smem + g7_img_row(nkt, r) + ((c ^ (r & 15)) << 4));
      u32x4* dst = reinterpret_cast<u32x4*>(C + (int64_t)m * P.E.ldc + n);
      __builtin_nontemporal_store(v, dst);
      if constexpr (st) {
        float f[8];
        bf16x8_unpack(v, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = f[j] - k[j];
          s1[j] += d;
          s2[j] += d * d;
        }
      }
      if constexpr (sb) {
        float d[8], yf[8];
        bf16x8_unpack(v, d);
        bf16x8_unpack(yv[i % YB], yf);
        const DropDesc& dd = P.E.bnb.drop;
        const uint32_t bits = dd.thr ? drop_bits8(seed, dd.site, (uint32_t)((int64_t)m * P.N + n), dd.thr) : 0xFFu;
        const float sc = dd.thr ? dd.scale : 1.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float keep = (bits >> j) & 1u ? sc : 0.f;
          const float xh = (yf[j] - mu[j]) * rs[j];
          const float z = act_f(P.E.bnb.act, xh * ga[j] + be[j]);
          const float dp = d[j] * keep * act_grad_from_out(P.E.bnb.act, z);
          s1[j] += dp;
          s2[j] += dp * xh;
        }
      }
    }
  }
  if constexpr (!st && !sb) return;
  else {
#pragma unroll
  for (int j = 0; j < 8; ++j) {   // lanes c, c + 16, c + 32, c + 48 of the wave hold the same chunk
    s1[j] += __shfl_xor(s1[j], 16);
    s2[j] += __shfl_xor(s2[j], 16);
    s1[j] += __shfl_xor(s1[j], 32);
    s2[j] += __shfl_xor(s2[j], 32);
  }
  // the ring stage neither image part occupies (every K step's copies have landed)
  float* red = reinterpret_cast<float*>(smem + ((nkt + 2) % 3) * G7_STAGE);   // [12 waves][128 cols][2]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < 16) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[(wave * 128 + 8 * c + j) * 2 + 0] = s1[j];
      red[(wave * 128 + 8 * c + j) * 2 + 1] = s2[j];
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 128 && n0 + t < P.N) {
    float S1 = 0.f, S2 = 0.f;
    for (int w = 0; w < G7_NT / 64; ++w) {
      S1 += red[(w * 128 + t) * 2 + 0];
      S2 += red[(w * 128 + t) * 2 + 1];
    }
    const float kt = __uint_as_float((uint32_t)*reinterpret_cast<const uint16_t*>(smem + g7_img_row(nkt, 0) +
                                                                                  2 * t) << 16);
    if constexpr (st) {
      const float nr = (float)min(256, P.M - m0);
      float* out = P.E.cstats + (int64_t)(m0 / 256) * 2 * P.N + n0 + t;
      out[0] = kt + S1 / nr;
      out[P.N] = fmaxf(S2 - S1 * S1 / nr, 0.f);
    } else {
      float* out = P.E.bnb.part + (int64_t)(m0 / 256) * 2 * P.N + n0 + t;
      out[0] = S1;
      out[P.N] = S2;
    }
  }
  }
}

// Straight-line LDS-image epilogue of a FULL tile for one option set, fixed at compile time:
// the general path (epi_calc8 over run-time options, with per-lane bounds tests) compiles to
// a long chain of branches that took ~5k cycles of the MFMA waves per tile (tools/gemm_stamps.hip),
// as long as three K steps.  Same operations, same order (alpha, bias, residual, ReLU, gate,
// dropout), so the results are bit-identical to the general path.  The dropout keep bits
// (drop_bits8 of the lane's 8 groups of 8 columns, group 2 i + pr at bits 8 (2 i + pr)) were
// hashed during the K loop, where the MFMA waves' VALU is otherwise idle.
template <bool BIAS, bool RELU, bool DROP, int PX>
TT2_DEV void g7_epi_fast(const EpiParams& E, const f32x4 (&acc)[4][4], const f32x4 (&pbias)[2][2], char* smem,
                         int nkt, int m0, int n0, int wm, int wn, int lane, uint64_t dbits) {
  const int q = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = wm * 64 + 16 * i + (lane & 15), m = m0 + r;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      float v[8];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[i][2 * pr][rr]),
                                                         __float_as_uint(acc[i][2 * pr + 1][rr]), false, false);
        v[rr] = __uint_as_float(sw[0]);
        v[4 + rr] = __uint_as_float(sw[1]);
      }
      const int cl = wn * 64 + 16 * (2 * pr + (q & 1)) + 8 * (q >> 1), n = n0 + cl;
      char* cp = smem + g7_img_row(nkt, r) + (((cl >> 3) ^ (r & 15)) << 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = BIAS ? v[j] * E.alpha + pbias[pr][0][j] : v[j] * E.alpha;
        v[4 + j] = BIAS ? v[4 + j] * E.alpha + pbias[pr][1][j] : v[4 + j] * E.alpha;
      }
      if (PX) {
        float t[8];
        unpack_lds8(cp, t);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (PX == 1) v[j] += t[j];
          else v[j] = t[j] != 0.f ? v[j] * E.gate_scale : 0.f;
        }
      }
      if (RELU) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
      }
      if (DROP) {
        const uint32_t kb = (uint32_t)(dbits >> (8 * (2 * i + pr)));
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (kb >> j) & 1u ? v[j] * E.drop.scale : 0.f;
      }
      bf16x8 x;
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = (bf16)v[j];
      *reinterpret_cast<bf16x8*>(cp) = x;
    }
  }
}

template <bool AK, bool BKC, int SM = 0>
TT2_DEV void g7_item(const G7Prob& P, int tile, int split, char* smem, unsigned long long* span) {
#ifdef TT2_PHASE
  unsigned long long* srec = span ? span + TT2_SPAN_W * blockIdx.x : nullptr;
#else
  (void)span;
#endif
  const OpDesc& A = P.A;
  const OpDesc& B = P.B;
  const EpiParams& E = P.E;
  const int M = P.M, N = P.N, K = P.K, ntn = P.ntn;
  float* ws = P.splits > 1 ? P.ws : nullptr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = (tile / ntn) * 256, n0 = (tile % ntn) * 128;
  const int kb = split * P.k_split, ke = min(K, kb + P.k_split);
  const int nkt = (ke - kb + 63) / 64;
  const bool tail = ((ke - kb) & 63) != 0;
  if (wave >= 8) {   // ------------------------------------------------ loader waves
    const int lw = wave - 8;
    // staged epilogue operand (whole tiles only)
    const bool px = P.pre_x && n0 + 128 <= N;
    const void* xs = P.pre_x == 1 ? E.res : E.gate;
    const int64_t ldx = P.pre_x == 1 ? E.ldr : E.ldg;
#if G7_REG
    // Register-staged operand steps (G7_REG; plain operands, no K tail -- conv operands and
    // tails keep the LDS-DMA ring below): the loader lanes load a step's 16-B pieces into VGPRs
    // (global_load_dwordx4, 48 per lane) and write them into the ring slot with ds_write_b128
    // once the slot is free: step t + 2 is written at the start of step t (into the stage step
    // t - 1 released), then step t + 3 is loaded, so one step is in flight in VGPRs.
    // The same bytes land at the same LDS addresses as the LDS-DMA copies (bit-identical
    // results).  Measured slower than the LDS-DMA ring on every shape (tools/lib_ab.py, DESIGN.md
    // 5.2): off by default, kept for the A/B.
    if (A.conv_t == 0 && B.conv_t == 0 && !tail) {
      // (lane state per path: the conv path's coordinates are not live here)
      G7Lane<G7_AI> la;
      G7Lane<G7_BI> lb;
      g7_lane_init<AK>(la, A, m0, kb, lane, lw);
      g7_lane_init<BKC>(lb, B, n0, kb, lane, lw);
      u32x4 ra[G7_AI], rb[G7_BI];
      auto fetch = [&](int step) {   // plain operands: loop-invariant lane offsets
        const int k0 = kb + 64 * step;
        const char* ba = reinterpret_cast<const char*>(A.p) + (AK ? (int64_t)k0 : (int64_t)k0 * A.ld) * 2;
        const char* bb = reinterpret_cast<const char*>(B.p) + (BKC ? (int64_t)k0 : (int64_t)k0 * B.ld) * 2;
#pragma unroll
        for (int i = 0; i < G7_AI; ++i) ra[i] = *reinterpret_cast<const u32x4*>(ba + la.off[i]);
#pragma unroll
        for (int i = 0; i < G7_BI; ++i) rb[i] = *reinterpret_cast<const u32x4*>(bb + lb.off[i]);
      };
      auto put = [&](int stage) {
        char* sa = smem + stage * G7_STAGE;
        g7_put<G7_AI>(ra, sa, lane, lw);
        g7_put<G7_BI>(rb, sa + G7_A, lane, lw);
      };
      fetch(0);
      put(0);
      if (nkt > 1) { fetch(1); put(1); }
      if (nkt > 2) fetch(2);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      int st = 2;
      for (int t = 0; t < nkt; ++t) {
        if (t + 2 < nkt) {
          put(st);   // step t + 2 into the stage step t - 1 released
          st = st == 2 ? 0 : st + 1;
          if (t + 3 < nkt) fetch(t + 3);
        } else if (px) {
          if (t == nkt - 2 || nkt == 1) g7_issue_x(P, xs, ldx, smem, nkt, m0, n0, 0, 12, lane, lw);
          if (t == nkt - 1) g7_issue_x(P, xs, ldx, smem, nkt, m0, n0, 192, 4, lane, lw);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's slot writes are done
        __builtin_amdgcn_s_barrier();
      }
    } else
#endif
    {
    G7Lane<G7_AI> la;
    G7Lane<G7_BI> lb;
    const bool cfast_a = g7_conv_fast(A) && !tail, cfast_b = g7_conv_fast(B) && !tail;
    g7_lane_init<AK>(la, A, m0, kb, lane, lw);
    g7_lane_init<BKC>(lb, B, n0, kb, lane, lw);
    auto issue = [&](int step, int stage) {   // steps are issued in order 0, 1, 2, ...
      char* sa = smem + stage * G7_STAGE;
      const int k0 = kb + 64 * step;
      const bool tl = tail && step == nkt - 1;
      g7_issue<AK>(A, la, sa, k0, ke, lane, lw, tl, cfast_a);
      g7_issue<BKC>(B, lb, sa + G7_A, k0, ke, lane, lw, tl, cfast_b);
    };
    issue(0, 0);
    if (nkt > 1) { issue(1, 1); asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); }
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    int st = 2;
    for (int t = 0; t < nkt; ++t) {
      if (t + 2 < nkt) {
        issue(t + 2, st);
        st = st == 2 ? 0 : st + 1;
      } else if (px) {
        // rows 0..191 once the stage of step nkt - 3 is free, rows 192..255 a step later
        if (t == nkt - 2 || nkt == 1) g7_issue_x(P, xs, ldx, smem, nkt, m0, n0, 0, 12, lane, lw);
        if (t == nkt - 1) g7_issue_x(P, xs, ldx, smem, nkt, m0, n0, 192, 4, lane, lw);
      }
      if (t + 2 < nkt || (px && t == nkt - 2))
        asm volatile("s_waitcnt vmcnt(12)" ::: "memory");   // step t+1 landed; t+2 (or the staged rows) in flight
      else if (!px)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    }
    if (px) {   // the staged tile has landed
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    if (!P.lds_epi) return;
    __syncthreads();   // the MFMA waves' C image is in LDS
    g7_store_c<SM>(P, smem, m0, n0, nkt);
    return;
  }

  // ------------------------------------------------------------------ MFMA waves
  const int wm = wave >> 1, wn = wave & 1;
  const bool do_ks = !AK && E.ksum && (tile % ntn) == 0 && wn == 0;
  // forward layout: this lane's two 8-column bias chunks, loaded before the K loop (the
  // MFMA waves issue no other global loads, so they land meanwhile) instead of one
  // dependent round trip in the epilogue
  const int ql = lane >> 4;
  const bool pre_b = AK && BKC && !ws && E.bias && E.vec;
  f32x4 pbias[2][2];
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    const int n = n0 + wn * 64 + 16 * (2 * pr + (ql & 1)) + 8 * (ql >> 1);
    pbias[pr][0] = pbias[pr][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (pre_b && n + 8 <= N) {
      pbias[pr][0] = *reinterpret_cast<const f32x4*>(E.bias + n);
      pbias[pr][1] = *reinterpret_cast<const f32x4*>(E.bias + n + 4);
    }
  }
  // k-sums on the matrix core: an all-ones B fragment makes D[n][m] = sum_k A[m][k] (one
  // extra MFMA per A fragment; summing the fragments on the VALU stalled the K loop)
  f32x4 ksa[4];
  Frag8<bf16> fones;
#pragma unroll
  for (int e = 0; e < 8; ++e) fones.v[e] = (bf16)1.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) ksa[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint32_t seed = (!ws && E.drop.thr) ? *E.drop.seed : 0u;
  const bool px = P.pre_x && n0 + 128 <= N;
  // the straight-line image epilogue's option set (wave-uniform), -1: the general path
  const int fast = (P.lds_epi && m0 + 256 <= M && n0 + 128 <= N && (P.pre_x == 0 || px)) ? P.epi_fast : -1;
  const bool pre_drop = fast >= 4 && fast <= 7;   // its dropout keep bits are hashed in the K loop
  const int gps = (8 + nkt - 1) / nkt;            // keep-bit groups per K step
  uint64_t dbits = 0;
#if G7_PRIO
  // waves w and w + 4 share a SIMD and run the same K loop in lockstep: the younger half at
  // static priority 1 wins the VALU / issue arbitration it otherwise always loses
  // (MI355X_MICROARCH.md, two waves per SIMD, item 4)
  if (wave >= 4) __builtin_amdgcn_s_setprio(1);
#endif
  __builtin_amdgcn_s_barrier();
  int stage = 0;
  for (int t = 0; t < nkt; ++t) {
    G7_STAMP(t, 0)
    const char* sa = smem + stage * G7_STAGE;
    const char* sb = sa + G7_A;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      Frag8<bf16> fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) g7_frag<AK>(fa[i], sa, wm * 64 + 16 * i, kk, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) g7_frag<BKC>(fb[j], sb, wn * 64 + 16 * j, kk, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) mma16(fb[j], fa[i], acc[i][j]);   // D[n][m]
      if (!AK && do_ks) {
#pragma unroll
        for (int i = 0; i < 4; ++i) mma16(fones, fa[i], ksa[i]);
      }
    }
    if (pre_drop) {   // VALU work beside this step's MFMAs
      const int g1 = min(8, (t + 1) * gps);
      for (int gi = t * gps; gi < g1; ++gi) {
        const int m = m0 + wm * 64 + 16 * (gi >> 1) + (lane & 15);
        const int n = n0 + wn * 64 + 16 * (2 * (gi & 1) + (ql & 1)) + 8 * (ql >> 1);
        const uint32_t kb = drop_bits8(seed, E.drop.site, (uint32_t)((int64_t)m * E.n_log + n), E.drop.thr);
        dbits |= (uint64_t)kb << (8 * gi);
      }
    }
    stage = stage == 2 ? 0 : stage + 1;
    G7_STAMP(t, 1)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this stage's reads retired (WAR vs the next copy)
    __builtin_amdgcn_s_barrier();
  }
  G7_STAMP(nkt, 0)

  if (!AK && do_ks) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float ks = ksa[i][0];   // every lane of the row's column (lane & 15) holds it
      const int m = m0 + wm * 64 + 16 * i + lane;
      if (lane < 16 && m < M) {
        if (ws) ws[(int64_t)P.splits * M * N + (int64_t)split * M + m] = ks;
        else E.ksum[m] = E.ksum_beta != 0.f ? E.ksum_beta * E.ksum[m] + ks : ks;
      }
    }
  }

  // lane (q = lane >> 4) holds C[m][n0 + wn*64 + 16 j + 4 q + r] in acc[i][j][r]; swapping
  // column blocks (2p, 2p+1) between row pairs q, q^1 leaves 8 consecutive columns per lane
  const int q = ql;
  if (px) __builtin_amdgcn_s_barrier();   // the loaders' staged residual / gate tile has landed
  if (P.lds_epi) {
    // epilogue values -> bf16 C image [256 rows][16 chunks of 16 B] (chunk c of row r at
    // c ^ (r & 15): the 16 rows of one store instruction hit 16 different bank groups),
    // then all 12 waves store whole 256-B row segments
    switch (fast) {   // wave-uniform
#define TT2_G7F(code, B_, R_, D_, X_)                                                                       \
  case code:                                                                                                \
    if constexpr (!B_ || (AK && BKC)) g7_epi_fast<B_, R_, D_, X_>(E, acc, pbias, smem, nkt, m0, n0, wm, wn, lane, dbits); \
    break;
      TT2_G7F(0, false, false, false, 0)
      TT2_G7F(1, true, false, false, 0)
      TT2_G7F(2, false, true, false, 0)
      TT2_G7F(3, true, true, false, 0)
      TT2_G7F(4, false, false, true, 0)
      TT2_G7F(5, true, false, true, 0)
      TT2_G7F(6, false, true, true, 0)
      TT2_G7F(7, true, true, true, 0)
      TT2_G7F(8, false, false, false, 1)
      TT2_G7F(9, false, false, false, 2)
#undef TT2_G7F
      default:
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = wm * 64 + 16 * i + (lane & 15), m = m0 + r;
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        float v[8];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[i][2 * pr][rr]),
                                                           __float_as_uint(acc[i][2 * pr + 1][rr]), false, false);
          v[rr] = __uint_as_float(sw[0]);
          v[4 + rr] = __uint_as_float(sw[1]);
        }
        const int cl = wn * 64 + 16 * (2 * pr + (q & 1)) + 8 * (q >> 1), n = n0 + cl;
        if (m >= M || n >= N) continue;
        if (pre_b) {
          const f32x4 b0 = pbias[pr][0], b1 = pbias[pr][1];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[j] = v[j] * E.alpha + b0[j];
            v[4 + j] = v[4 + j] * E.alpha + b1[j];
          }
        }
        float o[8];
        char* cp = smem + g7_img_row(nkt, r) + (((cl >> 3) ^ (r & 15)) << 4);   // C overwrites the staged chunk
        epi_calc8(E, seed, m, n, v, pre_b, o, px && P.pre_x == 1 ? cp : nullptr, px && P.pre_x == 2 ? cp : nullptr);
        bf16x8 x;
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (bf16)o[j];
        *reinterpret_cast<bf16x8*>(cp) = x;
      }
    }
    }
    G7_STAMP(nkt, 1)
    __syncthreads();
    G7_STAMP(nkt, 2)
    g7_store_c<SM>(P, smem, m0, n0, nkt);
    G7_STAMP(nkt, 3)
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + 16 * i + (lane & 15);
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[i][2 * pr][r]),
                                                         __float_as_uint(acc[i][2 * pr + 1][r]), false, false);
        v[r] = __uint_as_float(sw[0]);
        v[4 + r] = __uint_as_float(sw[1]);
      }
      const int n = n0 + wn * 64 + 16 * (2 * pr + (q & 1)) + 8 * (q >> 1);
      if (m >= M || n >= N) continue;
      if (ws) {
        float* w = ws + ((int64_t)split * M + m) * N + n;
        if (n + 8 <= N && (N % 4) == 0) {
          *reinterpret_cast<f32x4*>(w) = f32x4{v[0], v[1], v[2], v[3]};
          *reinterpret_cast<f32x4*>(w + 4) = f32x4{v[4], v[5], v[6], v[7]};
        } else {
          for (int j = 0; j < 8; ++j)
            if (n + j < N) w[j] = v[j];
        }
      } else if (pre_b && n + 8 <= N) {
        const f32x4 b0 = pbias[pr][0], b1 = pbias[pr][1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = v[j] * E.alpha + b0[j];
          v[4 + j] = v[4 + j] * E.alpha + b1[j];
        }
        epi_store8(E, seed, m, n, N, v, true);
      } else {
        epi_store8(E, seed, m, n, N, v);
      }
    }
  }
  G7_STAMP(nkt, 3)
}

template <bool AK, bool BKC, int SM = 0>
__global__ __launch_bounds__(G7_NT, 1) void gemm7_kernel(G7Prob P) {
  __shared__ __attribute__((aligned(1024))) char smem[G7_SMEM];
  __shared__ int span_done;
  G7_RT(0)
  span_begin(P.span, &span_done);
  const int u = xcd_item(blockIdx.x, P.items);
  g7_item<AK, BKC, SM>(P, u % (P.items / P.splits), u / (P.items / P.splits), smem, P.span);
  span_end(P.span, &span_done, G7_NT / 64);
  G7_RT(1)
}

// Grouped launch: up to G7_MAXP independent problems of one layout (e.g. all weight
// gradients of a layer, which share K = tokens), one workgroup per work item; items
// G.ibase + blockIdx.x (tt2_gemm_grouped_ex launches a capped grid as several launches of
// consecutive items, G.ibase a multiple of 8, so block b still runs on XCD b % 8).
template <bool AK, bool BKC>
__global__ __launch_bounds__(G7_NT, 1) void gemm7g_kernel(G7Group G) {
  __shared__ __attribute__((aligned(1024))) char smem[G7_SMEM];
  __shared__ int span_done;
  span_begin(G.p[0].span, &span_done);
  const int u = xcd_item(G.ibase + blockIdx.x, G.items);
  int p = 0;
#pragma unroll
  for (int i = 1; i < G7_MAXP; ++i)
    if (i < G.np && u >= G.p[i].item0) p = i;
  const G7Prob& P = G.p[p];
  const int local = u - P.item0, nt = P.items / P.splits;
  g7_item<AK, BKC>(P, local % nt, local / nt, smem, G.p[0].span);
  span_end(G.p[0].span, &span_done, G7_NT / 64);
}

// fixed-order split-K slab reduce + epilogue
__global__ void gemm_splitk_reduce(const float* ws, int splits, EpiParams E, int M, int N) {
  splitk_reduce_body(ws, splits, E, M, N, blockIdx.x, gridDim.x);
}

// split-K reduce of every split problem of a group (blockIdx.y = problem); plane y = np, when
// present, finalizes the deferred LayerNorm column sums (4 loads in flight per lane)
__global__ void gemm_splitk_reduce_g(G7Group G) {
  if (G.fin_only || (int)blockIdx.y == G.np) {
    const G7Fin& f = G.fin;
    const int o = blockIdx.x * G7_FIN_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= 3 * f.C) return;
    const int which = o / f.C, c = o - which * f.C;
    float* dst = f.dst[which];
    if (!dst) return;
    const float* src = f.part + (int64_t)which * f.C + c;
    const int64_t rs = 3 * (int64_t)f.C;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int r = lane;
    for (; r + 192 < f.nb; r += 256) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] += src[(r + 64 * u) * rs];
    }
    for (; r < f.nb; r += 64) acc[0] += src[r * rs];
    const float v = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if (lane == 0) dst[c] = f.gb != 0.f ? f.gb * dst[c] + v : v;
    return;
  }
  const G7Prob& P = G.p[blockIdx.y];
  if (P.splits > 1) splitk_reduce_body(P.ws, P.splits, P.E, P.M, P.N, blockIdx.x, gridDim.x);
}

G7Prob g7_prob(const OpDesc& A, const OpDesc& B, const EpiParams& E, int M, int N, int K, int splits,
                            float* ws) {
  G7Prob P{A, B, E, M, N, K, K, 1, (N + 127) / 128, 0, 0, ws, 0, 0, -1, nullptr};
  if (splits > 1) {
    P.k_split = ((K + splits - 1) / splits + 63) / 64 * 64;
    P.splits = (K + P.k_split - 1) / P.k_split;
  }
  P.items = ((M + 255) / 256) * P.ntn * P.splits;
  return P;
}

// g7_epi_fast's option code for this launch, or -1 (general path): bias (forward layout, where
// it is prefetched), ReLU, dropout, or one staged bf16 residual / gate alone; no beta.
int g7_fast_code(const G7Prob& P, bool fwd) {
  const EpiParams& E = P.E;
  if (!P.lds_epi || E.beta != 0.f || E.act == ACT_TANH) return -1;
  if (P.pre_x) {
    const bool alone = !E.bias && E.act == ACT_NONE && !E.drop.thr && (P.pre_x == 1 ? !E.gate : !E.res);
    return alone ? 7 + P.pre_x : -1;
  }
  if (E.res || E.gate) return -1;
  if (E.bias && !fwd) return -1;
  return (E.bias ? 1 : 0) | (E.act == ACT_RELU ? 2 : 0) | (E.drop.thr ? 4 : 0);
}

template <bool AK, bool BKC>
hipError_t launch7_t(const OpDesc& A, const OpDesc& B, const EpiParams& E, int M, int N, int K, int splits, float* ws,
                   hipStream_t s, bool lds_epi) {
  G7Prob P = g7_prob(A, B, E, M, N, K, splits, ws);
  P.lds_epi = lds_epi && P.splits == 1 && E.c_dt == TT2_BF16 && E.vec && (N % 8) == 0;
  // the loader waves stage a bf16 residual / gate tile in LDS during the last K steps
  P.pre_x = !P.lds_epi ? 0 : (E.res && E.res_dt == TT2_BF16) ? 1 : (E.gate && E.gate_dt == TT2_BF16) ? 2 : 0;
  P.epi_fast = g7_fast_code(P, AK && BKC);
  ProbeScope ps(s, P.items);
  P.span = ps.span;
  // fused BatchNorm statistics: own instantiations (the forward / dgrad conv layout only)
  const int sm = E.cstats ? 1 : E.bnb.part ? 2 : 0;
  auto go = [&](auto kern) {
    if (ps.ext()) hipExtLaunchKernelGGL(kern, dim3(P.items), dim3(G7_NT), 0, s, ps.e0, ps.e1, 0, P);
    else hipLaunchKernelGGL(kern, dim3(P.items), dim3(G7_NT), 0, s, P);
  };
  if constexpr (AK && BKC) {
    if (sm == 1) go(gemm7_kernel<AK, BKC, 1>);
    else if (sm == 2) go(gemm7_kernel<AK, BKC, 2>);
    else go(gemm7_kernel<AK, BKC, 0>);
  } else {
    go(gemm7_kernel<AK, BKC, 0>);
  }
  if (P.splits > 1 && !E.main_only)
    tt2g::launch_splitk_reduce(ws, P.splits, E, M, N, s);
  return hipGetLastError();
}

}  // namespace

namespace tt2g {

void launch_splitk_reduce(const float* ws, int splits, const Epilogue& E, int M, int N, hipStream_t s) {
  hipLaunchKernelGGL(gemm_splitk_reduce, dim3(splitk_blocks(M, N, E)), dim3(256), 0, s, ws, splits, EpiParams{E}, M, N);
}

// reduce grid: one 256-thread block per 256 work items of splitk_reduce_body's path (8, 4 or 1
// output elements per thread); a grid of one block per 256 ELEMENTS left 7 of 8 blocks of the
// 8-wide path with nothing to do (dispatching them cost more than the reduce)
int splitk_blocks(int M, int N, const Epilogue& E) {
  const int64_t per = ((N & 7) == 0 && E.vec) ? 8 : ((N & 3) == 0 ? 4 : 1);
  const int64_t items = std::max<int64_t>(((int64_t)M * N + per - 1) / per, M);
  const int64_t nb = (items + 255) / 256;
  return (int)(nb < 4096 ? nb : 4096);
}

hipError_t launch7(bool a_kc, bool b_kc, const Operand& A_, const Operand& B_, const Epilogue& E_, int M, int N, int K,
                   int splits, float* ws, hipStream_t s, bool lds_epi) {
  const OpDesc A{A_}, B{B_};
  const EpiParams E{E_};
  if (a_kc && b_kc) return launch7_t<true, true>(A, B, E, M, N, K, splits, ws, s, lds_epi);
  if (a_kc && !b_kc) return launch7_t<true, false>(A, B, E, M, N, K, splits, ws, s, lds_epi);
  if (!a_kc && b_kc) return launch7_t<false, true>(A, B, E, M, N, K, splits, ws, s, lds_epi);
  return launch7_t<false, false>(A, B, E, M, N, K, splits, ws, s, lds_epi);
}

}  // namespace tt2g

extern "C" int tt2_gemm_grouped_fin(const tt2_gemm_args* probs, int n, const tt2_ln_args* fin,
                                    hipStream_t stream) {
  return tt2_gemm_grouped_ex(probs, n, fin, 0, stream);
}

extern "C" int tt2_gemm_grouped_ex(const tt2_gemm_args* probs, int n, const tt2_ln_args* fin, int max_groups,
                                   hipStream_t stream) {
  ProbeDisarm disarm;
  if (n <= 0 && !fin) return TT2_OK;
  if ((n > 0 && !probs) || n > G7_MAXP) return tt2_set_error(TT2_E_INVALID, "tt2_gemm_grouped: 1..8 problems");
  G7Group G{};
  if (fin && fin->m > 0) {
    if (!fin->defer_finalize || !fin->workspace || fin->c <= 0)
      return tt2_set_error(TT2_E_INVALID, "tt2_gemm_grouped_fin: fin must be a deferred LayerNorm backward");
    G.fin.part = reinterpret_cast<const float*>(fin->workspace);
    G.fin.dst[0] = fin->dgamma; G.fin.dst[1] = fin->dbeta; G.fin.dst[2] = fin->dbias;
    G.fin.gb = fin->grad_beta;
    G.fin.C = fin->c;
    G.fin.nb = (int)(tt2_layernorm_bwd_workspace_size(fin) / (3 * sizeof(float) * fin->c));
  }
  int reduce_blocks = 0, ta = -1, tb = -1, main_only = 1;
  for (int i = 0; i < n; ++i) {
    const tt2_gemm_args* a = probs + i;
    if (a->m <= 0 || a->n <= 0) continue;
    OpDesc A, B;
    EpiParams ep;
    if (const int rc = tt2g::gemm_prep(a, A, B, ep); rc != TT2_OK) return rc;
    if (tt2g::gemm_plan(a) != 13)
      return tt2_set_error(TT2_E_INVALID, "tt2_gemm_grouped: every problem must take the v7 kernel (bf16, "
                                          "8-aligned inner dims, conv T, C >= 64, no decode fusions)");
    if (a->col_stats || a->bn_bwd) return tt2_set_error(TT2_E_INVALID, "tt2_gemm_grouped: no col_stats / bn_bwd");
    if (ta < 0) { ta = a->trans_a; tb = a->trans_b; }
    if (a->trans_a != ta || a->trans_b != tb)
      return tt2_set_error(TT2_E_INVALID, "tt2_gemm_grouped: problems must share trans_a / trans_b");
    G7Prob P = g7_prob(A, B, ep, a->m, a->n, a->k, a->splits > 1 ? a->splits : 1,
                       reinterpret_cast<float*>(a->workspace));
    P.item0 = G.items;
    G.items += P.items;
    G.p[G.np++] = P;
    main_only &= a->main_only;
    if (P.splits > 1) {
      reduce_blocks = std::max(reduce_blocks, tt2g::splitk_blocks(a->m, a->n, ep));
    }
  }
  const int fin_blocks = G.fin.nb ? (3 * G.fin.C + G7_FIN_WAVES - 1) / G7_FIN_WAVES : 0;
  if (G.np == 0) {
    G.fin_only = 1;
    if (fin_blocks) hipLaunchKernelGGL(gemm_splitk_reduce_g, dim3(fin_blocks, 1), dim3(256), 0, stream, G);
    return tt2_check_launch(hipGetLastError(), "tt2_gemm_grouped");
  }
  // max_groups > 0: at most that many work groups at a time (rounded down to a multiple of 8,
  // >= 8): the items go out as consecutive launches of that many, so a launch beside other
  // work leaves the rest of the CUs free.  An armed launch probe times the whole sequence: the
  // span slots of launch i start at item ibase, the eager events ride on the first and last.
  const int grid = max_groups > 0 ? std::min(G.items, std::max(8, max_groups / 8 * 8)) : G.items;
  ProbeScope ps(stream, G.items);
  ps.chunk(grid);
  for (G.ibase = 0; G.ibase < G.items; G.ibase += grid) {
    const dim3 g(std::min(grid, G.items - G.ibase));
    G.p[0].span = ps.span ? ps.span + (size_t)TT2_SPAN_W * G.ibase : nullptr;
    hipEvent_t ev0 = G.ibase == 0 ? ps.e0 : nullptr, ev1 = G.ibase + grid >= G.items ? ps.e1 : nullptr;
#define TT2_G7G(A_, B_)                                                                                    \
  if (ps.ext())                                                                                          \
    hipExtLaunchKernelGGL((gemm7g_kernel<A_, B_>), g, dim3(G7_NT), 0, stream, ev0, ev1, 0, G);            \
  else                                                                                                   \
    hipLaunchKernelGGL((gemm7g_kernel<A_, B_>), g, dim3(G7_NT), 0, stream, G);
    if (!ta && !tb) { TT2_G7G(true, true) }
    else if (!ta && tb) { TT2_G7G(true, false) }
    else if (ta && !tb) { TT2_G7G(false, true) }
    else { TT2_G7G(false, false) }
#undef TT2_G7G
  }
  G.ibase = 0;
  G.p[0].span = nullptr;
  if (main_only) reduce_blocks = 0;
  G.fin_only = reduce_blocks == 0 && fin_blocks > 0;
  if (G.fin_only)
    hipLaunchKernelGGL(gemm_splitk_reduce_g, dim3(fin_blocks, 1), dim3(256), 0, stream, G);
  else if (reduce_blocks > 0)
    hipLaunchKernelGGL(gemm_splitk_reduce_g, dim3(std::max(reduce_blocks, fin_blocks), G.np + (fin_blocks ? 1 : 0)),
                       dim3(256), 0, stream, G);
  return tt2_check_launch(hipGetLastError(), "tt2_gemm_grouped");
}

extern "C" int tt2_gemm_grouped(const tt2_gemm_args* probs, int n, hipStream_t stream) {
  return tt2_gemm_grouped_fin(probs, n, nullptr, stream);
}
