// gemm_v8.hip -- v8, the 64 x 64-tile kernel for products too small to fill the chip with v7's
// tiles, with its G8_RING / G8_LOADERS / G8_SPB knobs.
#include "gemm_common.h"

namespace {

// =====================================================================================
// v8 (bf16, A K-contiguous): 64 x 64 tiles for products whose 256 x 128 tiles cannot
// fill the chip -- the encoder's 2048-row GEMMs give v7 32-96 tiles for 256 CUs, and a
// lone v7 tile costs ~20k cycles however few CUs are busy.  512 threads: 4 MFMA waves,
// each one 32 x 32 block on v_mfma_f32_32x32x16_bf16 (a single f32x16 accumulator), and
// 4 loader waves that only issue LDS-DMA copies (as in v7: a wave that both copies into
// LDS and reads it gets a compiler-inserted vmcnt(0) before its reads, which would drain
// the pipeline every step).  Both operand tiles (64 rows x 64 k, 8 KB each) land in a
// 4-stage ring three K steps ahead, one s_barrier per step; 64 KB of LDS per workgroup,
// so two share a CU.  Images are 128-B rows with
// chunk c of row r at slot c ^ g8_swz(r) (the attention tiles' swizzle): K-contiguous
// operands are read as row fragments (two ds_read_b64), an N-contiguous B (dgrad) by
// ds_read_b64_tr_b16; both deliver the same permuted k order, which the MFMA sums over.
// Operands are swapped (D = B A^T) so each lane ends with one C row; a permlane32 swap
// gives it 8 consecutive columns, the fused epilogue runs in registers, and the tile
// leaves through LDS as whole 128-B rows.
// =====================================================================================
typedef float f32x16 __attribute__((ext_vector_type(16)));
#ifndef G8_RING   // ring stages (a power of two); the loaders run G8_RING - 1 steps ahead
#define G8_RING 4
#endif
#ifndef G8_LOADERS   // loader waves: 4 (2 copies per operand per wave and step) or 8 (1).  8: the
#define G8_LOADERS 8  // LDS-DMA issue rate, not the bytes in flight, bounded the K step
#endif
#ifndef G8_SPB   // K steps per barrier (64 deep each): 2 or 4 make the barrier cadence 128 / 256 deep
#define G8_SPB 1
#endif
static_assert(G8_RING > G8_SPB && G8_RING % G8_SPB == 0, "v8 ring: whole barrier groups, one ahead at least");
constexpr int G8_LW = G8_LOADERS, G8_PC = 8 / G8_LW;   // copies per operand tile per loader wave
constexpr int G8_NT = 64 * (4 + G8_LW), G8_STAGES = G8_RING;   // 4 MFMA waves + the loader waves
constexpr int G8_EPI = 512;   // threads of the C image store / fused statistics (64 rows x 8 chunks)
constexpr int G8_TILE = 64 * 128;          // bytes per operand tile: 64 rows x 64 bf16
constexpr int G8_STAGE = 2 * G8_TILE;

TT2_DEV int g8_swz(int r) {
  const int x = (r >> 1) & 7;
  return ((x & 1) << 2) | (x >> 1);
}

// this wave's G8_PC of the 8 LDS-DMA copies of one operand tile (8 rows x 128 B each);
// KC: tile rows are m / n and chunks run along k; MC: tile rows are k, chunks along n
template <bool KC>
TT2_DEV void g8_issue(const OpDesc& d, char* img, int r0, int k0, int lane, int wave) {
#pragma unroll
  for (int i = 0; i < G8_PC; ++i) {
    const int inst = wave * G8_PC + i;
    const int row = inst * 8 + (lane >> 3);
    const int c = (lane & 7) ^ g8_swz(row);
    const void* src = KC ? chunk_src(d, r0 + row, k0 + c * 8) : chunk_src(d, k0 + row, r0 + c * 8);
    __builtin_amdgcn_global_load_lds((gvoid_t*)src, (lvoid_t*)(img + inst * 1024), 16, 0, 0);
  }
}

// K-contiguous conv operand with C % 64 == 0 and K % 64 == 0 (as g7_conv_fast): each copy's
// row offset and valid-tap mask are set once per tile; a step reads tap k0 / C.
struct G8Conv { int64_t off[G8_PC]; uint32_t vm[G8_PC]; };
TT2_DEV void g8_conv_init(const OpDesc& d, G8Conv& c, int r0, int lane, int wave) {
#pragma unroll
  for (int i = 0; i < G8_PC; ++i) {
    const int row = (wave * G8_PC + i) * 8 + (lane >> 3), outer = r0 + row;
    const int t = outer % d.conv_t;
    const int lo = max(0, d.conv_pad - t), hi = min(31, d.conv_t - 1 - t + d.conv_pad);
    c.off[i] = (int64_t)outer * d.ld + ((lane & 7) ^ g8_swz(row)) * 8 - (int64_t)d.conv_pad * d.conv_c;
    c.vm[i] = outer < d.outer_max && hi >= lo ? (0xFFFFFFFFu >> (31 - hi)) & (0xFFFFFFFFu << lo) : 0u;
  }
}
TT2_DEV void g8_issue_conv(const OpDesc& d, const G8Conv& c, char* img, int k0, int wave) {
  const int tap = k0 / d.conv_c;
  const bf16* p = reinterpret_cast<const bf16*>(d.p) + k0;
#pragma unroll
  for (int i = 0; i < G8_PC; ++i) {
    const void* src = (c.vm[i] >> tap) & 1u ? (const void*)(p + c.off[i]) : (const void*)g_zero_page;
    __builtin_amdgcn_global_load_lds((gvoid_t*)src, (lvoid_t*)(img + (wave * G8_PC + i) * 1024), 16, 0, 0);
  }
}

// K-contiguous fragment of row `row`, k slice s (16 k): element j holds
// k = 16 s + 8 (j >> 2) + 4 hi + (j & 3), the order the transposed read delivers
TT2_DEV bf16x8 g8_frag_kc(const char* img, int row, int s, int hi) {
  const char* r = img + row * 128 + 8 * hi;
  const uint2 lo = *reinterpret_cast<const uint2*>(r + (((2 * s) ^ g8_swz(row)) << 4));
  const uint2 up = *reinterpret_cast<const uint2*>(r + (((2 * s + 1) ^ g8_swz(row)) << 4));
  union { uint4 u; bf16x8 v; } x;
  x.u = make_uint4(lo.x, lo.y, up.x, up.y);
  return x.v;
}

// N-contiguous fragment (image rows = k): column col0 + (lane & 31), same k order
TT2_DEV bf16x8 g8_frag_mc(const char* img, int col0, int s, int lane) {
  typedef __attribute__((address_space(3))) short4v lds_s4;
  const int hi = lane >> 5, q = (lane >> 2) & 3, p = lane & 3, g = (lane >> 4) & 1;
  const int col = col0 + 16 * g + 4 * p;
  const int r0 = 16 * s + 4 * hi + q;
  auto at = [&](int r) { return img + r * 128 + ((((col >> 3) ^ g8_swz(r))) << 4) + (col & 7) * 2; };
  short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)at(r0));
  short4v up = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)at(r0 + 8));
  union { short4v s[2]; bf16x8 v; } u;
  u.s[0] = lo;
  u.s[1] = up;
  return u.v;
}

// v8's fused BatchNorm statistics (SM 1: col_stats moments, 2: bn_bwd sums; see g7_store_c): each
// thread holds one row x 8 columns of the 64 x 64 image; the 8 rows of a wave that share a chunk
// combine by shuffles, the 8 waves through a free ring slot, and 64 threads write the 64-row
// chunk's value per column.
template <int SM>
TT2_DEV void g8_stats(const EpiParams& E, char* smem, int m0, int n0, int M, int N) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int rr = (tid >> 3) & 63, c = tid & 7, m = m0 + rr, n = n0 + 8 * c;
  const bool ok = tid < G8_EPI && m < M && n < N;   // (8 loader waves: threads past 512 add nothing)
  float v[8], s1[8], s2[8];
  bf16x8_unpack(*reinterpret_cast<const u32x4*>(smem + rr * 128 + ((c ^ g8_swz(rr)) << 4)), v);
  if constexpr (SM == 1) {
    float k[8];
    bf16x8_unpack(*reinterpret_cast<const u32x4*>(smem + ((c ^ g8_swz(0)) << 4)), k);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = ok ? v[j] - k[j] : 0.f;
      s1[j] = d;
      s2[j] = d * d;
    }
  } else {
    const int mc = min(m, M - 1), nc = min(n, N - 8);
    float yf[8];
    bf16x8_unpack(*reinterpret_cast<const u32x4*>(E.bnb.y + (int64_t)mc * N + nc), yf);
    const DropDesc& dd = E.bnb.drop;
    const uint32_t seed = dd.thr ? *dd.seed : 0u;
    const uint32_t bits = dd.thr ? drop_bits8(seed, dd.site, (uint32_t)((int64_t)m * N + n), dd.thr) : 0xFFu;
    const float sc = dd.thr ? dd.scale : 1.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float keep = (bits >> j) & 1u ? sc : 0.f;
      const float xh = (yf[j] - E.bnb.mean[nc + j]) * E.bnb.rstd[nc + j];
      const float z = act_f(E.bnb.act, xh * E.bnb.gamma[nc + j] + E.bnb.beta[nc + j]);
      const float dp = ok ? v[j] * keep * act_grad_from_out(E.bnb.act, z) : 0.f;
      s1[j] = dp;
      s2[j] = dp * xh;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {   // lanes c, c + 8, ..., c + 56: the wave's 8 rows of this chunk
    s1[j] += __shfl_xor(s1[j], 8);
    s2[j] += __shfl_xor(s2[j], 8);
    s1[j] += __shfl_xor(s1[j], 16);
    s2[j] += __shfl_xor(s2[j], 16);
    s1[j] += __shfl_xor(s1[j], 32);
    s2[j] += __shfl_xor(s2[j], 32);
  }
  float* red = reinterpret_cast<float*>(smem + 2 * G8_STAGE);   // [8 waves][64 cols][2], past the image
  if (lane < 8 && w < G8_EPI / 64) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[(w * 64 + 8 * c + j) * 2 + 0] = s1[j];
      red[(w * 64 + 8 * c + j) * 2 + 1] = s2[j];
    }
  }
  __syncthreads();
  if (tid < 64 && n0 + tid < N) {
    float S1 = 0.f, S2 = 0.f;
    for (int q = 0; q < G8_EPI / 64; ++q) {
      S1 += red[(q * 64 + tid) * 2 + 0];
      S2 += red[(q * 64 + tid) * 2 + 1];
    }
    float* out = (SM == 1 ? E.cstats : E.bnb.part) + (int64_t)(m0 / 64) * 2 * N + n0 + tid;
    if constexpr (SM == 1) {
      const int cc = tid >> 3;
      const float kt = __uint_as_float((uint32_t)*reinterpret_cast<const uint16_t*>(
                                           smem + ((cc ^ g8_swz(0)) << 4) + 2 * (tid & 7)) << 16);
      const float nr = (float)min(64, M - m0);
      out[0] = kt + S1 / nr;
      out[N] = fmaxf(S2 - S1 * S1 / nr, 0.f);
    } else {
      out[0] = S1;
      out[N] = S2;
    }
  }
}

template <bool BKC, int SM = 0>
__global__ __launch_bounds__(G8_NT, G8_STAGES <= 4 ? 2 : 1) void gemm8_kernel(OpDesc A, OpDesc B, EpiParams E, int M, int N, int K,
                                                         int ntn, int items, unsigned long long* span) {
  __shared__ __attribute__((aligned(1024))) char smem[G8_STAGES * G8_STAGE];
  __shared__ int span_done;
  span_begin(span, &span_done);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5;
  const int tile = xcd_item(blockIdx.x, items);
  const int m0 = (tile / ntn) * 64, n0 = (tile % ntn) * 64;
  const int nkt = (K + 63) / 64;
  if (wave >= 4) {   // ---------------------------------------------- loader waves
    const int lw = wave - 4;
    const bool afast = A.conv_t > 0 && (A.conv_c & 63) == 0 && (K & 63) == 0;
    G8Conv ca;
    if (afast) g8_conv_init(A, ca, m0, lane, lw);
    auto issue = [&](int t) {
      char* st = smem + (t & (G8_STAGES - 1)) * G8_STAGE;
      if (afast) g8_issue_conv(A, ca, st, 64 * t, lw);
      else g8_issue<true>(A, st, m0, 64 * t, lane, lw);
      g8_issue<BKC>(B, st + G8_TILE, n0, 64 * t, lane, lw);
    };
    // G8_STAGES - G8_SPB steps ahead; each step is 2 G8_PC copies per loader wave
    constexpr int AH = G8_STAGES - G8_SPB;
    auto wait_ahead = [](int ahead) {   // step t+1 landed, `ahead` later steps may stay in flight
      switch (ahead * 2 * G8_PC) {        // copies per step and wave: 2 G8_PC
        case 24: asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); break;
        case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
        case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
        case 14: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
        case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
        case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    };
    for (int t = 0; t < AH && t < nkt; ++t) issue(t);
    wait_ahead(min(AH, nkt) - G8_SPB);   // steps 0 .. G8_SPB - 1 landed
    __builtin_amdgcn_s_barrier();
    for (int t = 0; t < nkt; t += G8_SPB) {
#pragma unroll
      for (int j = 0; j < G8_SPB; ++j)   // into the stages steps t - G8_SPB .. t - 1 used: free since the last barrier
        if (t + AH + j < nkt) issue(t + AH + j);
      wait_ahead(min(AH - G8_SPB, nkt - 2 * G8_SPB - t));
      __builtin_amdgcn_s_barrier();    // steps t + G8_SPB .. t + 2 G8_SPB - 1 landed
    }
  } else {   // ------------------------------------------------------- MFMA waves
    const int wm = wave >> 1, wn = wave & 1;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    __builtin_amdgcn_s_barrier();
    for (int t0 = 0; t0 < nkt; t0 += G8_SPB) {
#pragma unroll
      for (int j = 0; j < G8_SPB; ++j) {
        const int t = t0 + j;
        if (G8_SPB > 1 && t >= nkt) break;
        const char* sa = smem + (t & (G8_STAGES - 1)) * G8_STAGE;
        const char* sb = sa + G8_TILE;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const bf16x8 fa = g8_frag_kc(sa, wm * 32 + (lane & 31), s, hi);
          const bf16x8 fb = BKC ? g8_frag_kc(sb, wn * 32 + (lane & 31), s, hi) : g8_frag_mc(sb, wn * 32, s, lane);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb, fa, acc, 0, 0, 0);   // D[n][m]
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // these stages' reads retired before they are re-filled
      __builtin_amdgcn_s_barrier();
    }
    // lane holds C[m0 + 32 wm + (lane & 31)][n0 + 32 wn + (r & 3) + 8 (r >> 2) + 4 hi]; the
    // permlane32 swap of register groups (0,1) and (2,3) leaves 8 consecutive columns per lane.
    // The ring is free (every wave passed the last barrier): it takes the C image [64][128 B].
    const int r = wm * 32 + (lane & 31), m = m0 + r;
    const uint32_t seed = E.drop.thr ? *E.drop.seed : 0u;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[8 * pr + i]),
                                                         __float_as_uint(acc[8 * pr + 4 + i]), false, false);
        v[i] = __uint_as_float(sw[0]);
        v[4 + i] = __uint_as_float(sw[1]);
      }
      const int cl = wn * 32 + 16 * pr + 8 * hi, n = n0 + cl;
      if (m >= M || n >= N) continue;
      float o[8];
      epi_calc8(E, seed, m, n, v, false, o);
      bf16x8 x;
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = (bf16)o[j];
      *reinterpret_cast<bf16x8*>(smem + r * 128 + (((cl >> 3) ^ g8_swz(r)) << 4)) = x;
    }
  }
  __syncthreads();   // the C image is complete: 512 threads store whole 128-B rows
  bf16* C = reinterpret_cast<bf16*>(E.c);
  const int id = tid, rr = id >> 3, c = id & 7, mm = m0 + rr, nn = n0 + 8 * c;
  if (tid < G8_EPI && mm < M && nn < N)   // nontemporal, as v7's C (g7_store_c)
    __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(smem + rr * 128 + ((c ^ g8_swz(rr)) << 4)),
                                reinterpret_cast<u32x4*>(C + (int64_t)mm * E.ldc + nn));
  if constexpr (SM != 0) g8_stats<SM>(E, smem, m0, n0, M, N);
  span_end(span, &span_done, G8_NT / 64);
}

template <bool BKC>
hipError_t launch8_t(const OpDesc& A, const OpDesc& B, const EpiParams& E, int M, int N, int K, hipStream_t s) {
  const int ntn = (N + 63) / 64, items = ((M + 63) / 64) * ntn;
  ProbeScope ps(s, items);
  auto go = [&](auto kern) {
    if (ps.ext())
      hipExtLaunchKernelGGL(kern, dim3(items), dim3(G8_NT), 0, s, ps.e0, ps.e1, 0, A, B, E, M, N, K, ntn, items,
                            ps.span);
    else
      hipLaunchKernelGGL(kern, dim3(items), dim3(G8_NT), 0, s, A, B, E, M, N, K, ntn, items, ps.span);
  };
  if (E.cstats) go(gemm8_kernel<BKC, 1>);   // fused BatchNorm statistics (64-row chunks)
  else if (E.bnb.part) go(gemm8_kernel<BKC, 2>);
  else go(gemm8_kernel<BKC, 0>);
  return hipGetLastError();
}

}  // namespace

namespace tt2g {

hipError_t launch8(bool b_kc, const Operand& A_, const Operand& B_, const Epilogue& E_, int M, int N, int K,
                   hipStream_t s) {
  const OpDesc A{A_}, B{B_};
  const EpiParams E{E_};
  return b_kc ? launch8_t<true>(A, B, E, M, N, K, s) : launch8_t<false>(A, B, E, M, N, K, s);
}

}  // namespace tt2g
