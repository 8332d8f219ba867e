// gemm_v1.hip -- v1, the register-staged 128 x 128 kernel: every dtype and alignment (the f32
// exact mode, operands whose rows are not whole 16-B chunks).
//
// Tiling: 128x128 output tile, BK = 32, 256 threads = 4 waves (2 x 2), each wave
// 64x64 = 4x4 MFMA 16x16 blocks.  Global -> registers -> LDS double buffer with
// the next tile's loads in flight during the current tile's MFMAs (one barrier
// per K step).  K-contiguous tiles are read with 16-B ds_read, M/N-contiguous
// tiles with ds_read_b64_tr_b16 (gfx950 transposing LDS read).
// Split-K (gridDim.z > 1) writes raw f32 partial slabs to the workspace and a
// second kernel (gemm_splitk_reduce) sums them in a fixed order (bitwise
// reproducible) and applies the epilogue.
#include "gemm_common.h"

namespace {

constexpr int BK = 32;

// Load one 16-B chunk at (outer, inner) with bounds/conv masking.
template <typename T>
TT2_DEV ChunkV<T> load_op_chunk(const OpDesc& d, int outer, int inner) {
  constexpr int E = Chunk<T>::N;
  const T* base = reinterpret_cast<const T*>(d.p);
  if (outer >= d.outer_max || inner >= d.inner_max) return zero_chunk<T>();
  if (d.conv_t > 0) {
    const int t = outer % d.conv_t;
    const int ts = t + inner / d.conv_c - d.conv_pad;
    if (ts < 0 || ts >= d.conv_t) return zero_chunk<T>();
    // chunks never straddle taps (conv_c % E == 0, checked on the host)
    return ld_chunk<T>(base + (int64_t)outer * d.ld + inner - (int64_t)d.conv_pad * d.conv_c);
  }
  const T* p = base + (int64_t)outer * d.ld + inner;
  if (inner + E <= d.inner_max) return ld_chunk<T>(p);
  ChunkV<T> c = zero_chunk<T>();
  for (int e = 0; e < E; ++e)
    if (inner + e < d.inner_max) c.e[e] = p[e];
  return c;
}

// LDS tile geometry for one operand.
//  KC (K-contiguous): tile[128][BK + pad], row = m (or n)
//  MC (M-contiguous): tile[BK][128 + pad], row = k
template <typename T, bool KC> struct TileGeo;
template <typename T> struct TileGeo<T, true> {
  static constexpr int LD = BK + Chunk<T>::N;   // +16 B per row
  static constexpr int ELEMS = 128 * LD;
  static constexpr int CPR = BK / Chunk<T>::N;   // chunks per row
};
template <typename T> struct TileGeo<T, false> {
  static constexpr int LD = 128 + Chunk<T>::N;
  static constexpr int ELEMS = BK * LD;
  static constexpr int CPR = 128 / Chunk<T>::N;
};

template <typename T> struct NCh { static constexpr int V = 128 * BK / Chunk<T>::N / NT; };

// global tile -> registers.  tile_r0: first m/n of the tile; k0: first k.
template <typename T, bool KC>
TT2_DEV void g2r(ChunkV<T> (&r)[NCh<T>::V], const OpDesc& d, int tile_r0, int k0, int tid) {
  using G = TileGeo<T, KC>;
#pragma unroll
  for (int i = 0; i < NCh<T>::V; ++i) {
    const int c = tid + NT * i;
    const int row = c / G::CPR, cc = c % G::CPR;
    if (KC) r[i] = load_op_chunk<T>(d, tile_r0 + row, k0 + cc * Chunk<T>::N);
    else r[i] = load_op_chunk<T>(d, k0 + row, tile_r0 + cc * Chunk<T>::N);
  }
}
template <typename T, bool KC>
TT2_DEV void r2s(const ChunkV<T> (&r)[NCh<T>::V], T* tile, int tid) {
  using G = TileGeo<T, KC>;
#pragma unroll
  for (int i = 0; i < NCh<T>::V; ++i) {
    const int c = tid + NT * i;
    const int row = c / G::CPR, cc = c % G::CPR;
    st_chunk<T>(tile + row * G::LD + cc * Chunk<T>::N, r[i]);
  }
}

// fragment for rows [r0, r0+16) of the tile (r = m or n), k in [0, 32)
template <typename T, bool KC>
TT2_DEV void s2f(Frag8<T>& f, const T* tile, int r0, int lane) {
  using G = TileGeo<T, KC>;
  if (KC) frag_row(f, tile + (r0 + (lane & 15)) * G::LD + 8 * (lane >> 4));
  else frag_col(f, tile, G::LD, 8 * (lane >> 4), r0, lane);
}

template <typename T, bool AK, bool BKC>
__global__ __launch_bounds__(NT) void gemm_kernel(OpDesc A, OpDesc B, EpiParams E, int M, int N, int K,
                                                  int k_split, float* ws) {
  using GA = TileGeo<T, AK>;
  using GB = TileGeo<T, BKC>;
  __shared__ __attribute__((aligned(16))) T smem[2 * (GA::ELEMS + GB::ELEMS)];
  constexpr int STAGE = GA::ELEMS + GB::ELEMS;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int kb = blockIdx.z * k_split;
  const int ke = min(K, kb + k_split);
  // bound the k dimension of both operands to this split
  if (AK) A.inner_max = ke; else A.outer_max = ke;
  if (BKC) B.inner_max = ke; else B.outer_max = ke;
  const int nkt = (ke - kb + BK - 1) / BK;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  ChunkV<T> ra[NCh<T>::V], rb[NCh<T>::V];
  g2r<T, AK>(ra, A, m0, kb, tid);
  g2r<T, BKC>(rb, B, n0, kb, tid);
  r2s<T, AK>(ra, smem, tid);
  r2s<T, BKC>(rb, smem + GA::ELEMS, tid);
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nkt;
    if (more) {
      g2r<T, AK>(ra, A, m0, kb + (kt + 1) * BK, tid);
      g2r<T, BKC>(rb, B, n0, kb + (kt + 1) * BK, tid);
    }
    Frag8<T> fa[4], fb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) s2f<T, AK>(fa[i], smem + cur * STAGE, wm * 64 + 16 * i, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) s2f<T, BKC>(fb[j], smem + cur * STAGE + GA::ELEMS, wn * 64 + 16 * j, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) mma16(fa[i], fb[j], acc[i][j]);
    if (more) {
      r2s<T, AK>(ra, smem + (cur ^ 1) * STAGE, tid);
      r2s<T, BKC>(rb, smem + (cur ^ 1) * STAGE + GA::ELEMS, tid);
    }
    __syncthreads();
  }

  // epilogue: acc[i][j][r] = C[m0 + wm*64 + 16i + 4*(lane>>4) + r][n0 + wn*64 + 16j + (lane&15)]
  const uint32_t seed = E.drop.thr ? *E.drop.seed : 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * 64 + 16 * i + 4 * (lane >> 4) + r;
        const int n = n0 + wn * 64 + 16 * j + (lane & 15);
        if (m < M && n < N) {
          if (ws) ws[((int64_t)blockIdx.z * M + m) * N + n] = acc[i][j][r];
          else st_any(E.c, (int64_t)m * E.ldc + n, E.c_dt, epi_value(E, seed, m, n, acc[i][j][r]));
        }
      }
}


template <typename T, bool AK, bool BKC>
hipError_t launch_t(const OpDesc& A, const OpDesc& B, const EpiParams& E, int M, int N, int K, int splits,
                    float* ws, hipStream_t s) {
  int k_split = K;
  if (splits > 1) {
    k_split = ((K + splits - 1) / splits + BK - 1) / BK * BK;
    splits = (K + k_split - 1) / k_split;
  }
  dim3 grid((N + BN - 1) / BN, (M + BM - 1) / BM, splits);
  hipLaunchKernelGGL((gemm_kernel<T, AK, BKC>), grid, dim3(NT), 0, s, A, B, E, M, N, K, k_split,
                     splits > 1 ? ws : nullptr);
  if (splits > 1 && !E.main_only)
    tt2g::launch_splitk_reduce(ws, splits, E, M, N, s);
  return hipGetLastError();
}
}  // namespace

namespace tt2g {

hipError_t launch1(bool bf16_in, bool a_kc, bool b_kc, const Operand& A_, const Operand& B_, const Epilogue& E_, int M,
                   int N, int K, int splits, float* ws, hipStream_t s) {
  const OpDesc A{A_}, B{B_};
  const EpiParams E{E_};
#define TT2_GEMM_CASE(T)                                                                    \
  if (a_kc && b_kc) return launch_t<T, true, true>(A, B, E, M, N, K, splits, ws, s);        \
  if (a_kc && !b_kc) return launch_t<T, true, false>(A, B, E, M, N, K, splits, ws, s);      \
  if (!a_kc && b_kc) return launch_t<T, false, true>(A, B, E, M, N, K, splits, ws, s);      \
  return launch_t<T, false, false>(A, B, E, M, N, K, splits, ws, s);
  if (bf16_in) { TT2_GEMM_CASE(bf16) }
  TT2_GEMM_CASE(float)
#undef TT2_GEMM_CASE
}

}  // namespace tt2g
