// attention_mono.hip -- monotonic alignment search over the raw attention scores of forwards
// already run (tt2_align_monotonic; head dim 64, gfx950).  A translation unit of its own, so
// that the device code of the other attention units stays what it was (it has its
// entry points with it); the score products reuse the v3 forward's building blocks
// (attention_v3.h), the walk over them is align_walk.h's.
#include "align_walk.h"
#include "attention_v3.h"

namespace {

// ---------------------------------------------------------- monotonic alignment search
// Viterbi over the raw scores of one (layer, head) per utterance (tt2_capi.h states the
// definition), in align_walk.h's launch shape: the producer waves form the [32 rows, Te] f32 score
// block of query block i + 1 while the DP wave walks block i (walk_block) and then the move bits
// backwards; the producers re-form the scores along the path for its log-probability.

// in-kernel timeline hooks (tools/mono_stamps.hip defines them; empty here)
#ifndef MONO_STAMP
#define MONO_STAMP(slot)
#endif

// MFMA producer: the head's K stays in LDS at the key capacities whose move bits leave it room
template <int KC> constexpr bool MONO_KRES = KC <= 256;

// the v3 forward's score products of one 64-key tile for the lane's query row (fq): K rows from
// the resident LDS copy, or straight from global in the same fragment layout
template <bool KRES>
TT2_DEV void mono_scores(f32x16 (&s)[2], const bf16x8 (&fq)[4], const bf16* cK, const RowBuf& K, int k0, int ql, int hi) {
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    zero16(s[kb]);
    if constexpr (KRES) {
#pragma unroll
      for (int st = 0; st < 4; ++st) mma32(rowfrag(cK, 32 * kb + ql, 2 * st + hi), fq[st], s[kb]);
    } else {
      bf16x8 fk[4];
      own_frags(fk, K, k0 + 32 * kb + ql, hi);
#pragma unroll
      for (int st = 0; st < 4; ++st) mma32(fk[st], fq[st], s[kb]);
    }
  }
}
// attn_align_kernel's scalar dot
template <typename T> TT2_DEV float mono_dot(const T* Qr, const T* Kr) {
  float dot = 0.f;
#pragma unroll 8
  for (int d = 0; d < D; ++d) dot += to_f32(Qr[d]) * to_f32(Kr[d]);
  return dot;
}
TT2_DEV uint64_t readlane64(uint64_t x, int l) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)x, l);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(x >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

// PROD 0: MFMA producer (bf16), 1: plain producer bf16, 2: plain producer f32
template <int KC, int PROD>
__global__ __launch_bounds__(WALK_NT) void align_mono_kernel(tt2_align_mono_args a) {
  using C = WalkCfg<KC>;
  using T = std::conditional_t<PROD == 2, float, bf16>;
  constexpr int R = C::R, SLD = C::SLD, SBUF = C::SBUF;
  constexpr bool KRES = MONO_KRES<KC>;
  constexpr int KBYTES = (PROD == 0 && KRES) ? KC * D * 2 : 16;
  __shared__ __attribute__((aligned(16))) char smem[KBYTES + 2 * SBUF * 4 + C::MOVE_BYTES + KC * 4];
  bf16* sK = reinterpret_cast<bf16*>(smem);
  float* sS = reinterpret_cast<float*>(smem + KBYTES);
  int* hist = reinterpret_cast<int*>(smem + KBYTES + 2 * SBUF * 4 + C::MOVE_BYTES);
  // after the DP the score buffers hold the path and the per-row log-probabilities
  int* pathL = reinterpret_cast<int*>(sS);
  float* termL = sS + SBUF;
  static_assert(SBUF >= TT2_MONO_MAX_FRAMES, "path / terms alias one score buffer each");

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ql = lane & 31, hi = lane >> 5;
  const int b = blockIdx.x;
  const int Ty = len_limit(a.tq, a.q_len, b);
  const int Tx = len_limit(a.tk, a.key_len, b);
  const int Te = min(Tx, Ty);
  const int li = a.sel ? a.sel[2 * b] : a.sel_layer;
  const int h = a.sel ? a.sel[2 * b + 1] : a.sel_head;
  int32_t* path = a.path + (int64_t)b * a.tq;
  int32_t* dur = a.durations + (int64_t)b * a.tk;
  if (Ty <= 0 || Tx <= 0 || li < 0 || li >= a.n_layers || h < 0 || h >= a.heads) {   // block-uniform
    for (int n = tid; n < a.tq; n += WALK_NT) path[n] = -1;
    for (int t = tid; t < a.tk; t += WALK_NT) dur[t] = 0;
    if (tid == 0) a.logp[b] = 0.f;
    return;
  }
  const T* Qp = reinterpret_cast<const T*>(a.q[li]) + (int64_t)b * a.tq * a.q_ld + h * D;
  const T* Kp = reinterpret_cast<const T*>(a.k[li]) + (int64_t)b * a.tk * a.k_ld + h * D;
  const float* lse = a.lse[li] + ((int64_t)b * a.heads + h) * a.tq;
  // (only the MFMA producer reads through the buffer views)
  const RowBuf Q = row_buf(reinterpret_cast<const bf16*>(Qp), a.q_ld, a.tq);
  const RowBuf K = row_buf(reinterpret_cast<const bf16*>(Kp), a.k_ld, a.tk);
  // move words: LDS when tq rows of them fit (block-uniform), else the caller's workspace
  const bool mv_lds = walk_move_in_lds(a.tq, a.tk);
  uint64_t* mvL = reinterpret_cast<uint64_t*>(smem + KBYTES + 2 * SBUF * 4);
  uint64_t* mvG = reinterpret_cast<uint64_t*>(a.workspace) + (int64_t)b * a.tq * R;
  const int ntile = (Te + 63) / 64, nblk = (Ty + WALK_RB - 1) / WALK_RB;

  for (int t = tid; t < KC; t += WALK_NT) hist[t] = 0;
  if constexpr (PROD == 0 && KRES) {
    if (w < WALK_NP) {
      uint4 rk[Stage3<64 * WALK_NP>::PER];
      for (int t = 0; t < ntile; ++t) {
        g2r3<64 * WALK_NP>(rk, K, 64 * t, tid);
        r2s3<64 * WALK_NP>(rk, sK + t * 64 * D, tid);
      }
    }
    __syncthreads();
  }

  // ---- score block i -> buffer i & 1 (producer waves)
  bf16x8 fqn[4];
  if constexpr (PROD == 0) own_frags(fqn, Q, ql, hi);
  auto produce = [&](int i) {
    float* S = sS + (i & 1) * SBUF;
    const int q0 = WALK_RB * i;
    if constexpr (PROD == 0) {
      bf16x8 fq[4];
#pragma unroll
      for (int st = 0; st < 4; ++st) fq[st] = fqn[st];
      own_frags(fqn, Q, q0 + WALK_RB + ql, hi);   // the next block's rows, in flight over this block and the barrier
      for (int t = w; t < ntile; t += WALK_NP) {
        f32x16 s[2];
        mono_scores<KRES>(s, fq, sK + t * 64 * D, K, 64 * t, ql, hi);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int g = 0; g < 4; ++g)   // accumulator rows 4g..4g+3 are keys 8g + 4hi + 0..3
            *reinterpret_cast<float4*>(S + ql * SLD + 64 * t + 32 * kb + 8 * g + 4 * hi) =
                make_float4(s[kb][4 * g], s[kb][4 * g + 1], s[kb][4 * g + 2], s[kb][4 * g + 3]);
      }
    } else {
      const int r = tid >> 3, c = tid & 7;   // 8 threads stride one row's keys
      if (q0 + r < Ty) {
        const T* Qr = Qp + (int64_t)(q0 + r) * a.q_ld;
        for (int t = c; t < Te; t += 8) S[r * SLD + t] = mono_dot<T>(Qr, Kp + (int64_t)t * a.k_ld);
      }
    }
  };

  // ---- the DP wave: rows of block i from buffer i & 1
  float v[R];
#pragma unroll
  for (int j = 0; j < R; ++j) v[j] = -INFINITY;
  auto consume = [&](int i, auto LDSC) {   // LDSC: the move words go to LDS (else to the workspace)
    const float* S = sS + (i & 1) * SBUF + lane * R;
    walk_block<R, SLD, decltype(LDSC)::value>(v, S, i, Ty, lane, mvL, mvG);
  };

  MONO_STAMP(0);
  for (int i = 0; i <= nblk; ++i) {
    if (w < WALK_NP) {
      if (i < nblk) produce(i);
    } else if (i > 0) {
      if (mv_lds) consume(i - 1, std::true_type{});
      else consume(i - 1, std::false_type{});
    }
    __syncthreads();
  }

  // ---- backtrack (the DP wave, which wrote the bits), CH frames at a time: lane i takes frame
  // nb - i and turns its R ballot words into one 64-bit window in key order that starts at key
  // tlo (a multiple of R at most CH - 1 + R - 1 <= 63 keys under the current key), all lanes at
  // once.  The serial part per frame is then two lane reads, a shift, an and and a subtract in
  // scalar registers; the frames' keys follow from the taken-move mask by a population count.
  MONO_STAMP(1);
  if (w == WALK_NP) {
    constexpr int CH = 64 - R;
    int t = __builtin_amdgcn_readfirstlane(Te - 1);
    for (int nb = Ty - 1; nb >= 0; nb -= CH) {
      const int n = nb - lane;
      const unsigned tlo = (unsigned)max(t - (CH - 1), 0) & ~(unsigned)(R - 1);
      unsigned wlo = 0, whi = 0;
      if (lane < CH && n >= 1) {   // (row 0 never moves)
        uint64_t wd[R];
        if (mv_lds) {
#pragma unroll
          for (int j = 0; j < R; ++j) wd[j] = mvL[n * R + j];
        } else {
#pragma unroll
          for (int j = 0; j < R; ++j) wd[j] = mvG[(int64_t)n * R + j];
        }
        unsigned x[R];
#pragma unroll
        for (int j = 0; j < R; ++j) x[j] = (unsigned)(wd[j] >> (tlo / R));
#pragma unroll
        for (int p = 0; p < 32; ++p) {   // window bit p <-> key tlo + p <-> word p % R, bit tlo / R + p / R
          wlo |= ((x[p % R] >> (p / R)) & 1u) << p;
          whi |= ((x[(p + 32) % R] >> ((p + 32) / R)) & 1u) << p;
        }
      }
      const int cnt = min(CH, nb + 1);
      unsigned idx = (unsigned)t - tlo;
      uint64_t taken = 0;   // bit i: the step from frame nb - i to the frame before it moved a key down
      for (int i = 0; i < cnt; ++i) {
        const uint64_t win = ((uint64_t)(unsigned)__builtin_amdgcn_readlane(whi, i) << 32) |
                             (unsigned)__builtin_amdgcn_readlane(wlo, i);
        const unsigned bit = (unsigned)(win >> idx) & 1u;
        taken |= (uint64_t)bit << i;
        idx -= bit;
      }
      const int mine = t - __popcll(taken & ((1ull << lane) - 1));
      t = __builtin_amdgcn_readfirstlane(t - __popcll(taken));
      if (lane < CH && n >= 0) {
        pathL[n] = mine;
        path[n] = mine;
        atomicAdd(&hist[mine], 1);
      }
    }
  }
  MONO_STAMP(2);
  __syncthreads();
  for (int n = Ty + tid; n < a.tq; n += WALK_NT) path[n] = -1;
  for (int t = tid; t < a.tk; t += WALK_NT) dur[t] = hist[t];

  // ---- ln P along the path: the producers re-form the scores they need
  const float c = a.scale * LOG2E;
  if (w < WALK_NP) {
    if constexpr (PROD == 0) {
      for (int i = w; i < nblk; i += WALK_NP) {
        const int row = WALK_RB * i + ql;
        const int t = row < Ty ? pathL[row] : -1;
        // 32 rows advance at most 31 keys: the block's keys lie in this tile and the next
        const int t0 = __builtin_amdgcn_readfirstlane(pathL[WALK_RB * i]) / 64;
        bf16x8 fq[4];
        own_frags(fq, Q, row, hi);
        float val = 0.f;
        for (int tt = t0; tt < min(t0 + 2, ntile); ++tt) {
          f32x16 s[2];
          mono_scores<KRES>(s, fq, sK + tt * 64 * D, K, 64 * tt, ql, hi);
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) val = 64 * tt + 32 * kb + crow(r, hi) == t ? s[kb][r] : val;
        }
        val = xor32_sum(val);   // the key lives in one lane half; the other adds 0
        if (hi == 0 && row < Ty) termL[row] = LN2 * (val * c - lse[row]);
      }
    } else {
      for (int n = tid; n < Ty; n += 64 * WALK_NP) {
        const float s = mono_dot<T>(Qp + (int64_t)n * a.q_ld, Kp + (int64_t)pathL[n] * a.k_ld);
        termL[n] = LN2 * (s * c - lse[n]);
      }
    }
  }
  __syncthreads();
  if (w == 0) {   // fixed order: lane-strided partial sums, then the shuffle tree
    float acc = 0.f;
    for (int n = lane; n < Ty; n += 64) acc += termL[n];
    acc = wave_sum(acc);
    if (lane == 0) a.logp[b] = acc / (float)Ty;
  }
  MONO_STAMP(3);
}

template <int PROD>
void mono_launch(const tt2_align_mono_args& a, hipStream_t s) {
  walk_by_kc(a.tk, [&](auto kc) {
    hipLaunchKernelGGL((align_mono_kernel<decltype(kc)::value, PROD>), dim3(a.batch), dim3(WALK_NT), 0, s, a);
  });
}
}  // namespace

extern "C" size_t tt2_align_monotonic_workspace_size(int batch, int tq, int tk) {
  if (batch <= 0 || tq <= 0 || tk <= 0 || tk > TT2_MONO_MAX_KEYS || walk_move_in_lds(tq, tk)) return 0;
  return (size_t)batch * walk_move_bytes(tq, tk);
}

extern "C" int tt2_align_monotonic(const tt2_align_mono_args* p, hipStream_t s) {
  const char* who = "tt2_align_monotonic";
  if (!p) return tt2_invalid(who, "args required");
  if (p->head_dim != D) return tt2_invalid(who, "head_dim must be 64");
  if (p->causal) return tt2_invalid(who, "monotonic alignment search is non-causal only");
  if (p->n_layers <= 0 || p->n_layers > TT2_GUIDE_MAX_LAYERS) return tt2_invalid(who, "needs 1..16 layers");
  if (p->dtype != TT2_DT_BF16 && p->dtype != TT2_DT_F32) return tt2_invalid(who, "dtype must be bf16 or f32");
  if (p->variant != 0 && p->variant != 1) return tt2_invalid(who, "variant must be 0 (auto) or 1 (plain producer)");
  if (p->batch < 0 || p->heads <= 0 || p->tq < 0 || p->tk < 0 || !(p->scale > 0.f) ||
      (int64_t)p->batch * p->heads > INT32_MAX)
    return tt2_invalid(who, "shape / scale");
  if (p->tk > TT2_MONO_MAX_KEYS) return tt2_invalid(who, "tk exceeds TT2_MONO_MAX_KEYS");
  if (p->tq > TT2_MONO_MAX_FRAMES) return tt2_invalid(who, "tq exceeds TT2_MONO_MAX_FRAMES");
  const int esz = p->dtype == TT2_DT_BF16 ? 2 : 4;
  if ((p->q_ld * esz) % 16 || (p->k_ld * esz) % 16 || p->q_ld < (int64_t)p->heads * D || p->k_ld < (int64_t)p->heads * D)
    return tt2_invalid(who, "leading dims must be 16-B multiples covering the heads");
  if (!p->path || !p->durations || !p->logp) return tt2_invalid(who, "path / durations / logp required");
  if (!p->sel && (p->sel_layer < 0 || p->sel_layer >= p->n_layers || p->sel_head < 0 || p->sel_head >= p->heads))
    return tt2_invalid(who, "fixed head outside the layers / heads");
  for (int l = 0; l < p->n_layers; ++l)
    if (!p->q[l] || !p->k[l] || !p->lse[l]) return tt2_invalid(who, "q / k / lse of a layer missing");
  const int rc = tt2_need_workspace(who, p->workspace, p->workspace_bytes,
                                    tt2_align_monotonic_workspace_size(p->batch, p->tq, p->tk), 8);
  if (rc != TT2_OK) return rc;
  const bool mfma = p->dtype == TT2_DT_BF16 && p->variant != 1;
  // the buffer views address rows with 32-bit byte offsets
  if (mfma && (((int64_t)p->tq * p->q_ld + D) * 2 > INT32_MAX || ((int64_t)p->tk * p->k_ld + D) * 2 > INT32_MAX))
    return tt2_invalid(who, "one batch element's q or k spans more than 2 GiB");
  if (p->batch == 0) return TT2_OK;
  if (mfma) mono_launch<0>(*p, s);
  else if (p->dtype == TT2_DT_BF16) mono_launch<1>(*p, s);
  else mono_launch<2>(*p, s);
  return tt2_check_launch(hipGetLastError(), who);
}
