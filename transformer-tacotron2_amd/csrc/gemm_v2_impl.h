// gemm_v2_impl.h -- v2, the LDS-DMA 128 x 128 kernel (bf16).  Compiled in gemm_v2v7v11.hip.
// A source, not a header: it defines kernels, non-inline functions and (v7) extern "C" entry
// points, so exactly one translation unit may include it (gemm_v2v7v11.hip).  It carries the .h
// suffix only so that the build's header scan rebuilds that unit when it changes.
#pragma once
#include "gemm_common.h"

namespace {

// =====================================================================================
// v2 (bf16): BK = 64, LDS-DMA staging (global_load_lds_dwordx4: each lane's 16-B chunk
// lands at lds_base + 16*lane), two LDS stages, one barrier per K-tile, XOR swizzles
// applied on the per-lane GLOBAL source address so the lane-linear LDS image reads
// conflict-free with ds_read_b128 (K-contiguous tiles) and ds_read_b64_tr_b16
// (M/N-contiguous tiles).  Out-of-range / conv-padding chunks load from a zero page.
// Epilogue: accumulators -> LDS (f32) -> 16-B vectorised epilogue + stores.
// =====================================================================================
constexpr int BK2 = 64;
constexpr int TILE_BYTES = 128 * BK2 * 2;               // 16 KB per operand tile
constexpr int STAGE_BYTES = 2 * TILE_BYTES;             // A + B
constexpr int EPI_LD = 132;                             // f32 words per staged C row (pad: conflict-free)
constexpr int SMEM2 = (2 * STAGE_BYTES > 128 * EPI_LD * 4) ? 2 * STAGE_BYTES : 128 * EPI_LD * 4;

// issue this wave's 4 of the 16 LDS-DMA instructions of one 128 x 64 operand tile
template <bool KC>
TT2_DEV void issue_tile(const OpDesc& d, char* lds_tile, int r0, int k0, int lane, int wave) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int inst = wave * 4 + i;
    const void* src;
    if (KC) {
      const int row = inst * 8 + (lane >> 3);
      const int gc = (lane & 7) ^ (row & 7);
      src = chunk_src(d, r0 + row, k0 + gc * 8);
    } else {
      const int kr = inst * 4 + (lane >> 4);
      const int gc = (lane & 15) ^ mc_swz(kr);
      src = chunk_src(d, k0 + kr, r0 + gc * 8);
    }
    __builtin_amdgcn_global_load_lds((gvoid_t*)src, (lvoid_t*)(lds_tile + inst * 1024), 16, 0, 0);
  }
}

template <bool AK, bool BKC>
__global__ __launch_bounds__(NT, 2) void gemm2_kernel(OpDesc A, OpDesc B, EpiParams E, int M, int N, int K,
                                                      int k_split, float* ws, int ntm, int ntn) {
  __shared__ __attribute__((aligned(1024))) char smem[SMEM2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // XCD-aware tile order: blocks b and b+8 share an XCD, so give each XCD a
  // contiguous run of tiles (walking n for a fixed m: the A row panel stays in that L2).
  const int nt = ntm * ntn;
  const int bid = blockIdx.x;
  const int q = nt / 8, rr = nt % 8, x = bid % 8;
  const int tile = (x < rr ? x * (q + 1) : rr * (q + 1) + (x - rr) * q) + bid / 8;
  const int m0 = (tile / ntn) * BM, n0 = (tile % ntn) * BN;
  const int kb = blockIdx.y * k_split;
  const int ke = min(K, kb + k_split);
  if (AK) A.inner_max = ke; else A.outer_max = ke;
  if (BKC) B.inner_max = ke; else B.outer_max = ke;
  const int nkt = (ke - kb + BK2 - 1) / BK2;
  const bool do_ks = !AK && E.ksum && (tile % ntn) == 0;   // one n-tile per m-tile sums A over k
  float ks[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  issue_tile<AK>(A, smem, m0, kb, lane, wave);
  issue_tile<BKC>(B, smem + TILE_BYTES, n0, kb, lane, wave);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    const char* sa = smem + (kt & 1) * STAGE_BYTES;
    const char* sb = sa + TILE_BYTES;
    if (kt + 1 < nkt) {
      char* na = smem + ((kt + 1) & 1) * STAGE_BYTES;
      issue_tile<AK>(A, na, m0, kb + (kt + 1) * BK2, lane, wave);
      issue_tile<BKC>(B, na + TILE_BYTES, n0, kb + (kt + 1) * BK2, lane, wave);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      Frag8<bf16> fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) frag2<AK>(fa[i], sa, wm * 64 + 16 * i, kk, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) frag2<BKC>(fb[j], sb, wn * 64 + 16 * j, kk, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) mma16(fa[i], fb[j], acc[i][j]);
    }
    if (!AK && do_ks) {
      // rows 4*(tid>>4) .. +3 of the [64 k][128 m] A image, m-chunk tid & 15
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kr = 4 * (tid >> 4) + r;
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(sa + kr * 256 + (((tid & 15) ^ mc_swz(kr)) << 4));
#pragma unroll
        for (int j = 0; j < 8; ++j) ks[j] += (float)v[j];
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (!AK && do_ks) {
    // reduce over the 16 k-groups: lanes l, l^16, l^32, l^48, then the 4 waves via LDS
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ks[j] += __shfl_xor(ks[j], 16, 64);
      ks[j] += __shfl_xor(ks[j], 32, 64);
    }
    if (lane < 16) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red[(wave * 16 + lane) * 8 + j] = ks[j];
    }
    __syncthreads();
    if (tid < 128) {
      const int cc = tid >> 3, j = tid & 7, m = m0 + tid;
      const float v = (red[(0 * 16 + cc) * 8 + j] + red[(1 * 16 + cc) * 8 + j]) +
                      (red[(2 * 16 + cc) * 8 + j] + red[(3 * 16 + cc) * 8 + j]);
      if (m < M) {
        if (ws) ws[(int64_t)gridDim.y * M * N + (int64_t)blockIdx.y * M + m] = v;
        else E.ksum[m] = E.ksum_beta != 0.f ? E.ksum_beta * E.ksum[m] + v : v;
      }
    }
    __syncthreads();
  }

  // stage C (f32) through LDS: row-major [128][EPI_LD]
  float* cs = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        cs[(wm * 64 + 16 * i + 4 * (lane >> 4) + r) * EPI_LD + wn * 64 + 16 * j + (lane & 15)] = acc[i][j][r];
  __syncthreads();
  const uint32_t seed = (!ws && E.drop.thr) ? *E.drop.seed : 0u;
#pragma unroll 2
  for (int it = 0; it < 8; ++it) {
    const int id = tid + NT * it;
    const int row = id >> 4, c8 = (id & 15) * 8;
    const int m = m0 + row, n = n0 + c8;
    if (m >= M || n >= N) continue;
    float v[8];
    const f32x4 lo = *reinterpret_cast<const f32x4*>(cs + row * EPI_LD + c8);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(cs + row * EPI_LD + c8 + 4);
    v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
    v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
    if (ws) {
      float* w = ws + ((int64_t)blockIdx.y * M + m) * N + n;
      if (n + 8 <= N && (N % 4) == 0) {
        *reinterpret_cast<f32x4*>(w) = lo;
        *reinterpret_cast<f32x4*>(w + 4) = hi;
      } else {
        for (int j = 0; j < 8; ++j)
          if (n + j < N) w[j] = v[j];
      }
    } else {
      epi_store8(E, seed, m, n, N, v);
    }
  }
}

template <bool AK, bool BKC>
hipError_t launch2_t(const OpDesc& A, const OpDesc& B, const EpiParams& E, int M, int N, int K, int splits, float* ws,
                   hipStream_t s) {
  int k_split = K;
  if (splits > 1) {
    k_split = ((K + splits - 1) / splits + BK2 - 1) / BK2 * BK2;
    splits = (K + k_split - 1) / k_split;
  }
  const int ntm = (M + BM - 1) / BM, ntn = (N + BN - 1) / BN;
  dim3 grid(ntm * ntn, splits);
  ProbeScope ps(s, 0);   // no span record in this kernel
  if (ps.ext())
    hipExtLaunchKernelGGL((gemm2_kernel<AK, BKC>), grid, dim3(NT), 0, s, ps.e0, ps.e1, 0, A, B, E, M, N, K, k_split,
                     splits > 1 ? ws : nullptr, ntm, ntn);
  else
    hipLaunchKernelGGL((gemm2_kernel<AK, BKC>), grid, dim3(NT), 0, s, A, B, E, M, N, K, k_split,
                     splits > 1 ? ws : nullptr, ntm, ntn);
  if (splits > 1 && !E.main_only)
    tt2g::launch_splitk_reduce(ws, splits, E, M, N, s);
  return hipGetLastError();
}


}  // namespace

namespace tt2g {

hipError_t launch2(bool a_kc, bool b_kc, const Operand& A_, const Operand& B_, const Epilogue& E_, int M, int N, int K,
                   int splits, float* ws, hipStream_t s) {
  const OpDesc A{A_}, B{B_};
  const EpiParams E{E_};
  if (a_kc && b_kc) return launch2_t<true, true>(A, B, E, M, N, K, splits, ws, s);
  if (a_kc && !b_kc) return launch2_t<true, false>(A, B, E, M, N, K, splits, ws, s);
  if (!a_kc && b_kc) return launch2_t<false, true>(A, B, E, M, N, K, splits, ws, s);
  return launch2_t<false, false>(A, B, E, M, N, K, splits, ws, s);
}

}  // namespace tt2g
