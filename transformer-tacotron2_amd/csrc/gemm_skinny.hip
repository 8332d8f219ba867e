// gemm_skinny.hip -- the skinny-M decode GEMM and its launcher.
#include "gemm_skinny.h"

namespace {

// =====================================================================================
// skinny-M (decode, M <= 64) bf16: out[M, N] = X[M, K] W[N, K]^T.  The problem is a
// latency-bound weight stream: every workgroup owns 16 output columns, its 4 waves split
// K, and each lane issues its WHOLE slice of W (NCH 16-B chunks) before anything else,
// then its X chunks (or the LayerNorm prologue), so the kernel pays about one memory
// round trip instead of one per 32-deep K step.  One MFMA 16x16x32 per 16 rows x 16
// columns x 32 k; cross-wave sums go through LDS.  Decode-step epilogues: KV-cache
// scatter (QKV projection), scaled positional encoding (pre-net projection) and the
// frame emit (mel/stop heads: mel_seq / stop_seq / previous frame, then the last
// workgroup to finish advances the device step counter).
// =====================================================================================

// Decode-step fusions carried by the skinny kernel (tt2_gemm_args a_ln_* / kv_* / pe_* / emit_*).
struct SkinnyFuse {
  const bf16* br; const float* gamma; const float* beta; bf16* h_out; float eps;   // LN prologue (gamma != 0)
  void* kv; const int32_t* kv_t; int kv_col0; int64_t kv_bstride, kv_ld;           // KV scatter (kv != 0)
  const float* pe; const float* pe_alpha; const int32_t* pe_t;                     // + alpha * pe[t][n]
  float* emit_mel; float* emit_stop; void* emit_prev; int32_t* emit_t; uint32_t* emit_seed;
  int32_t* emit_done; int emit_nmels, emit_tmax;                                   // frame emit (heads)
  const float* emit_stop_bias; int32_t* emit_stop_len; float emit_stop_thr;        // stop injection / tracking
};

constexpr int SK_LN_LD = 512 + 8;   // bf16 per LDS row of the normalised A (16-B pad)


template <typename TE, int NCH, bool LN, int MR>
__global__ __launch_bounds__(NT) void gemm_skinny_kernel(const TE* X, int64_t ldx, const TE* W, int64_t ldw,
                                                         EpiParams E, int M, int N, int K, SkinnyFuse F,
                                                         float* slab, int kper) {
  static_assert(!LN || (MR == 2 && __is_same(TE, bf16)), "LN prologue: bf16, m <= 32");
  typedef typename SkT<TE>::V V8;
  __shared__ float red[4][16 * MR][SK_COLS + 1];
  extern __shared__ __attribute__((aligned(16))) bf16 s_h[];   // [32][SK_LN_LD] when F.gamma (K == 512)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * SK_COLS;
  const int r = lane & 15, g = lane >> 4;
  const int n = n0 + r;
  const bool nok = n < N;
  // device scalars of the epilogue, issued up front
  const uint32_t seed = E.drop.thr ? *E.drop.seed : 0u;
  const int kv_t = F.kv ? *F.kv_t : 0;
  const int pe_t = F.pe ? *F.pe_t : 0;
  const float pe_al = F.pe ? *F.pe_alpha : 0.f;
  const int em_t = F.emit_mel ? *F.emit_t : 0;
  const TE* wrow = W + (int64_t)(nok ? n : 0) * ldw;
  // MR blocks of 16 rows: block q covers rows 16 q + r
  const TE* xr[MR];
  bool rok[MR];
#pragma unroll
  for (int q = 0; q < MR; ++q) {
    rok[q] = 16 * q + r < M;
    xr[q] = X + (int64_t)(rok[q] ? 16 * q + r : 0) * ldx;
  }
  union U { uint4 u; V8 v; };
  const uint4 z4 = make_uint4(0, 0, 0, 0);
  f32x4 acc[MR];
#pragma unroll
  for (int q = 0; q < MR; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  // split-K (slab != 0): workgroup row blockIdx.y takes k in [kbeg, kend) and stores its raw
  // partial sums to slab[blockIdx.y][m][n] (f32, no epilogue; tt2_ln_combine sums them)
  const int kbeg = slab ? blockIdx.y * kper : 0;
  const int kend = slab ? min(K, kbeg + kper) : K;
  float e_bias = 0.f, e_res[MR], e_pe = 0.f;
#pragma unroll
  for (int q = 0; q < MR; ++q) e_res[q] = 0.f;
  const int ecol = threadIdx.x & 15, erow = threadIdx.x >> 4, enn = n0 + ecol;
  for (int ks = kbeg; ks < kend; ks += 4 * NCH * 32) {
    const int kb = ks + wave * (NCH * 32);
    U w[NCH], a[MR][NCH];
    // (1) this lane's whole W slice: branch-free (an out-of-range chunk reads the zero page)
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int kk = kb + 32 * c + 8 * g;
      w[c].u = *reinterpret_cast<const uint4*>(nok && kk < kend ? (const void*)(wrow + kk) : (const void*)g_zero_page);
    }
    if constexpr (LN) {
      // (2a) h = LN(x + br) for the (<= 32) rows (K == 512, one pass): rows wave, wave + 4, ...,
      // every load issued before the first reduction; h goes to LDS (the A operand) and,
      // from workgroup 0, to F.h_out (the next residual)
      const int c0 = lane * 8;
      U xa[8], xb[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int row = min(wave + 4 * u, M - 1);
        xa[u].u = *reinterpret_cast<const uint4*>(X + (int64_t)row * ldx + c0);
        xb[u].u = *reinterpret_cast<const uint4*>(F.br + (int64_t)row * ldx + c0);
      }
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(F.gamma + c0), g1 = *reinterpret_cast<const f32x4*>(F.gamma + c0 + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(F.beta + c0), b1 = *reinterpret_cast<const f32x4*>(F.beta + c0 + 4);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int row = wave + 4 * u;
        float v[8], sum = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { v[j] = (float)xa[u].v[j] + (float)xb[u].v[j]; sum += v[j]; }
        const float mu = wave_sum(sum) / K;
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = v[j] - mu; sq += d * d; }
        const float rs = rsqrtf(wave_sum(sq) / K + F.eps);
        bf16x8 h;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          h[j] = (bf16)((v[j] - mu) * rs * (j < 4 ? g0[j] : g1[j - 4]) + (j < 4 ? b0[j] : b1[j - 4]));
        if (row < M) {
          *reinterpret_cast<bf16x8*>(s_h + row * SK_LN_LD + c0) = h;
          if (blockIdx.x == 0) *reinterpret_cast<bf16x8*>(F.h_out + (int64_t)row * K + c0) = h;
        }
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int kk = kb + 32 * c + 8 * g;
        const bool ok = kk < K;
#pragma unroll
        for (int q = 0; q < MR; ++q)
          a[q][c].u = (rok[q] && ok) ? *reinterpret_cast<const uint4*>(s_h + (16 * q + r) * SK_LN_LD + kk) : z4;
      }
    } else {
      // (2b) the X chunks, also all in flight
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int kk = kb + 32 * c + 8 * g;
#pragma unroll
        for (int q = 0; q < MR; ++q)
          a[q][c].u = *reinterpret_cast<const uint4*>(rok[q] && kk < kend ? (const void*)(xr[q] + kk)
                                                                          : (const void*)g_zero_page);
      }
      // keep every load above the first MFMA (the scheduler would otherwise interleave
      // them and pay one memory round trip per pair)
      __builtin_amdgcn_sched_barrier(0);
    }
    if (ks == kbeg && !slab) {
      // the epilogue's own operands (bias, residual, PE row), in flight behind the
      // operand loads instead of a second round trip after the reduction
      const bool ec = enn < N;
      if (E.bias && ec) e_bias = E.bias[enn];
      if (E.res && ec) {
#pragma unroll
        for (int q = 0; q < MR; ++q)
          if (erow + 16 * q < M) e_res[q] = ld_any(E.res, (int64_t)(erow + 16 * q) * E.ldr + enn, E.res_dt);
      }
      if (F.pe && ec) e_pe = pe_al * F.pe[(int64_t)pe_t * N + enn];
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int q = 0; q < MR; ++q) acc[q] = SkT<TE>::mma(a[q][c].v, w[c].v, acc[q]);
  }
  // acc layout: row 4*(lane>>4) + i, col lane & 15
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < MR; ++q) red[wave][16 * q + 4 * g + i][r] = acc[q][i];
  __syncthreads();
  if (slab) {
#pragma unroll
    for (int hrow = 0; hrow < MR; ++hrow) {
      const int m = erow + 16 * hrow;
      if (m < M && enn < N)
        slab[((int64_t)blockIdx.y * M + m) * N + enn] =
            (red[0][m][ecol] + red[1][m][ecol]) + (red[2][m][ecol] + red[3][m][ecol]);
    }
    return;
  }
  // bias / residual were prefetched: the epilogue proper runs without them
  EpiParams Ep = E;
  Ep.bias = nullptr;
  Ep.res = nullptr;
  Ep.alpha = 1.f;
#pragma unroll
  for (int hrow = 0; hrow < MR; ++hrow) {
    const int row = erow + 16 * hrow, col = ecol;
    const int m = row, nn = enn;
    if (m < M && nn < N) {
      const float v = (red[0][row][col] + red[1][row][col]) + (red[2][row][col] + red[3][row][col]);
      float y = epi_value(Ep, seed, m, nn, E.alpha * v + e_bias + e_res[hrow]);
      y += e_pe;
      st_any(E.c, (int64_t)m * E.ldc + nn, E.c_dt, y);
      // a row past the batch stride (t >= t_max: a replay beyond the cache) is not written
      if (F.kv && nn >= F.kv_col0 && (int64_t)kv_t * F.kv_ld < F.kv_bstride)
        reinterpret_cast<TE*>(F.kv)[(int64_t)m * F.kv_bstride + (int64_t)kv_t * F.kv_ld + (nn - F.kv_col0)] = (TE)y;
      if (F.emit_mel && em_t < F.emit_tmax) {
        if (nn < F.emit_nmels) {
          // frames after an utterance's stop are zero (its post-net then sees zero padding at
          // its own length; this step's stop update is e + 1 > em_t, so no race on the read)
          const float ym = (F.emit_stop_len && F.emit_stop_len[m] <= em_t) ? 0.f : y;
          F.emit_mel[((int64_t)m * F.emit_tmax + em_t) * F.emit_nmels + nn] = ym;
          reinterpret_cast<TE*>(F.emit_prev)[(int64_t)m * F.emit_nmels + nn] = (TE)ym;
        } else if (nn == F.emit_nmels) {
          // the stop logit (+ an injected per-utterance bias); the first frame at or above the
          // threshold fixes the utterance's length (one thread owns row m's stop column)
          const float ys = F.emit_stop_bias ? y + F.emit_stop_bias[(int64_t)m * F.emit_tmax + em_t] : y;
          F.emit_stop[(int64_t)m * F.emit_tmax + em_t] = ys;
          if (F.emit_stop_len && ys >= F.emit_stop_thr && F.emit_stop_len[m] > em_t) F.emit_stop_len[m] = em_t + 1;
        }
      }
    }
  }
  if (F.emit_mel) {
    // every workgroup has read the step counter (it addressed its stores with it): the
    // last one to arrive advances it (and the dropout seed) and re-arms the counter
    __syncthreads();
    if (threadIdx.x == 0) {
      const int prev = __hip_atomic_fetch_add(F.emit_done, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      if (prev == (int)gridDim.x - 1) {
        *F.emit_done = 0;
        if (em_t < F.emit_tmax) {   // the counter saturates at t_max (replays past it emit nothing)
          *F.emit_t = em_t + 1;
          if (F.emit_seed) *F.emit_seed += 1u;
        }
      }
    }
  }
}

}  // namespace

namespace tt2g {

hipError_t launch_skinny(const tt2_gemm_args* a, const Epilogue& E, hipStream_t stream) {
  const EpiParams ep{E};
  SkinnyFuse F{reinterpret_cast<const bf16*>(a->a_ln_branch), a->a_ln_gamma, a->a_ln_beta,
               reinterpret_cast<bf16*>(a->a_ln_out), a->a_ln_eps, a->kv_cache, a->kv_t,
               a->kv_col0, a->kv_bstride, a->kv_ld, a->pe_table, a->pe_alpha, a->pe_t, a->emit_mel, a->emit_stop,
               a->emit_prev, a->emit_t, a->emit_seed, a->emit_done, a->emit_nmels, a->emit_tmax,
               a->emit_stop_bias, a->emit_stop_len, a->emit_stop_thr};
  const size_t lds = a->a_ln_gamma ? 32 * SK_LN_LD * sizeof(bf16) : 0;
  // split-K (splits > 1, main_only): raw partial slabs [splits][m][n] f32 in the workspace
  const int sp = a->splits > 1 ? a->splits : 1;
  const int kper = sp > 1 ? ((a->k + sp - 1) / sp + 31) / 32 * 32 : a->k;
  float* slab = sp > 1 ? reinterpret_cast<float*>(a->workspace) : nullptr;
  const dim3 grid((a->n + SK_COLS - 1) / SK_COLS, sp > 1 ? (a->k + kper - 1) / kper : 1);
  // per-wave K slice = NCH x 32: one pass for K <= 4 * NCH * 32
  const int nch = kper <= 128 ? 1 : kper <= 256 ? 2 : kper <= 512 ? 4 : kper <= 1024 ? 8 : 16;
#define TT2_SK(TE, NCH, LN, MR)                                                                              \
  hipLaunchKernelGGL((gemm_skinny_kernel<TE, NCH, LN, MR>), grid, dim3(NT), lds, stream,                    \
                   reinterpret_cast<const TE*>(a->a), a->lda, reinterpret_cast<const TE*>(a->b), a->ldb, ep, \
                   a->m, a->n, a->k, F, slab, kper)
#define TT2_SK_M(TE, MR)                      \
  if (nch == 1) TT2_SK(TE, 1, false, MR);     \
  else if (nch == 2) TT2_SK(TE, 2, false, MR); \
  else if (nch == 4) TT2_SK(TE, 4, false, MR); \
  else if (nch == 8) TT2_SK(TE, 8, false, MR); \
  else if (MR == 2) TT2_SK(TE, 16, false, 2);  \
  else TT2_SK(TE, 8, false, 4);   /* 64 rows: two passes of 8 chunks (16 would spill) */
  if (a->a_ln_gamma) TT2_SK(bf16, 4, true, 2);   // bf16, k == 512, m <= 32 (checked by the plan)
  else if (a->dtype_in == TT2_F16) {
    if (a->m <= 32) { TT2_SK_M(f16, 2) } else { TT2_SK_M(f16, 4) }
  } else {
    if (a->m <= 32) { TT2_SK_M(bf16, 2) } else { TT2_SK_M(bf16, 4) }
  }
#undef TT2_SK_M
#undef TT2_SK
  return hipGetLastError();
}

}  // namespace tt2g
