// attention_mono.hip -- monotonic alignment search over the raw attention scores of forwards
// already run (tt2_align_monotonic; head dim 64, gfx950).  A translation unit of its own, so
// that the device code of the other attention units stays what it was (it has its
// entry points with it); the score products reuse the v3 forward's building blocks
// (attention_v3.h).
#include "attention_v3.h"

namespace {

// ---------------------------------------------------------- monotonic alignment search
// Viterbi over the raw scores of one (layer, head) per utterance (tt2_capi.h states the
// definition).  One work group per utterance: MONO_NP waves form the [32 rows, Te] f32 score
// block of query block i + 1 into LDS while one DP wave walks the 32 rows of block i.  The DP
// wave holds V across its lanes (lane L owns keys L*R .. L*R + R - 1), takes V[t - 1] of its
// first key from the lane below with one DPP wave shift, and writes the row's move bits as R
// ballots (bit L of word j <-> key L*R + j).  The same wave then walks the bits backwards, 64 - R
// frames per pass held one frame per lane, so the serial chain is lane reads and scalar ops.

constexpr int MONO_NP = 4;                    // score-producing waves
constexpr int MONO_NT = 64 * (MONO_NP + 1);   // + the DP wave
constexpr int MONO_RB = 32;                   // query rows per score block
constexpr float LN2 = 0.6931471805599453f;

// in-kernel timeline hooks (tools/mono_stamps.hip defines them; empty here)
#ifndef MONO_STAMP
#define MONO_STAMP(slot)
#endif

template <int KC> struct MonoCfg {            // KC: key capacity (tk rounded up)
  static constexpr int R = KC / 64;           // keys per DP lane
  static constexpr int SLD = KC + 4;          // score row stride in floats (spreads the producers' rows)
  static constexpr int SBUF = (MONO_RB + 1) * SLD;   // floats per score buffer (+ a row the DP's look-ahead may read)
  static constexpr bool KRES = KC <= 256;     // MFMA producer: the head's K stays in LDS
  static constexpr int MOVE_BYTES = KC == 128 ? 65536 : KC == 256 ? 49152 : 16384;
};
__host__ __device__ constexpr int mono_kc(int tk) { return tk <= 128 ? 128 : tk <= 256 ? 256 : 512; }
// bytes of move bits per utterance, and whether they fit the kernel's LDS share
__host__ __device__ inline size_t mono_move_bytes(int tq, int tk) { return (size_t)tq * (mono_kc(tk) / 64) * 8; }
__host__ __device__ inline bool mono_move_in_lds(int tq, int tk) {
  const int kc = mono_kc(tk);
  return mono_move_bytes(tq, tk) <= (size_t)(kc == 128 ? 65536 : kc == 256 ? 49152 : 16384);
}

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
__global__ __launch_bounds__(MONO_NT) void align_mono_kernel(tt2_align_mono_args a) {
  using C = MonoCfg<KC>;
  using T = std::conditional_t<PROD == 2, float, bf16>;
  constexpr int R = C::R, SLD = C::SLD, SBUF = C::SBUF;
  constexpr bool KRES = C::KRES;
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
    for (int n = tid; n < a.tq; n += MONO_NT) path[n] = -1;
    for (int t = tid; t < a.tk; t += MONO_NT) dur[t] = 0;
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
  const bool mv_lds = mono_move_in_lds(a.tq, a.tk);
  uint64_t* mvL = reinterpret_cast<uint64_t*>(smem + KBYTES + 2 * SBUF * 4);
  uint64_t* mvG = reinterpret_cast<uint64_t*>(a.workspace) + (int64_t)b * a.tq * R;
  const int ntile = (Te + 63) / 64, nblk = (Ty + MONO_RB - 1) / MONO_RB;

  for (int t = tid; t < KC; t += MONO_NT) hist[t] = 0;
  if constexpr (PROD == 0 && KRES) {
    if (w < MONO_NP) {
      uint4 rk[Stage3<64 * MONO_NP>::PER];
      for (int t = 0; t < ntile; ++t) {
        g2r3<64 * MONO_NP>(rk, K, 64 * t, tid);
        r2s3<64 * MONO_NP>(rk, sK + t * 64 * D, tid);
      }
    }
    __syncthreads();
  }

  // ---- score block i -> buffer i & 1 (producer waves)
  bf16x8 fqn[4];
  if constexpr (PROD == 0) own_frags(fqn, Q, ql, hi);
  auto produce = [&](int i) {
    float* S = sS + (i & 1) * SBUF;
    const int q0 = MONO_RB * i;
    if constexpr (PROD == 0) {
      bf16x8 fq[4];
#pragma unroll
      for (int st = 0; st < 4; ++st) fq[st] = fqn[st];
      own_frags(fqn, Q, q0 + MONO_RB + ql, hi);   // the next block's rows, in flight over this block and the barrier
      for (int t = w; t < ntile; t += MONO_NP) {
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
  auto ld_row = [&](float (&s)[R], const float* p) {
    if constexpr (R == 2) {
      const float2 x = *reinterpret_cast<const float2*>(p);
      s[0] = x.x; s[1] = x.y;
    } else {
#pragma unroll
      for (int q = 0; q < R / 4; ++q) {
        const float4 x = *reinterpret_cast<const float4*>(p + 4 * q);
        s[4 * q] = x.x; s[4 * q + 1] = x.y; s[4 * q + 2] = x.z; s[4 * q + 3] = x.w;
      }
    }
  };
  auto consume = [&](int i, auto LDSC) {   // LDSC: the move words go to LDS (else to the workspace)
    const float* S = sS + (i & 1) * SBUF + lane * R;
    const int n0 = MONO_RB * i, n1 = min(n0 + MONO_RB, Ty);
    // one DP row from scores s: the dependent chain is DPP shift -> compare -> select -> add
    auto row = [&](const float (&s)[R], int n) {
      // V[t - 1] of the lane's first key: the last key of the lane below (wave_shr:1; lane 0 keeps -inf)
      const float below = __int_as_float(__builtin_amdgcn_update_dpp(
          __float_as_int(-INFINITY), __float_as_int(v[R - 1]), 0x138, 0xF, 0xF, false));
      uint64_t bal[R];
#pragma unroll
      for (int j = R - 1; j >= 0; --j) {
        const float prev = j ? v[j - 1] : below;
        const bool m = prev > v[j];              // strict: a tie stays on the key
        bal[j] = __ballot(m);
        v[j] = s[j] + (m ? prev : v[j]);         // = s + max(V[t], V[t - 1]); the compare feeds both
      }
      if (lane == 0) {
        if constexpr (decltype(LDSC)::value) {
#pragma unroll
          for (int j = 0; j < R; ++j) mvL[n * R + j] = bal[j];
        } else {
#pragma unroll
          for (int j = 0; j < R; ++j) mvG[(int64_t)n * R + j] = bal[j];
        }
      }
    };
    float sa[R], sb[R];
    ld_row(sa, S);
    int n = n0;
    if (i == 0) {   // row 0: only key 0 can be reached
#pragma unroll
      for (int j = 0; j < R; ++j) v[j] = (lane == 0 && j == 0) ? sa[0] : -INFINITY;
      ld_row(sa, S + SLD);
      n = 1;
    }
    // two rows per trip, two register sets: each row's scores are read one row ahead of the chain
    // (after the block's last row the read falls on the buffer's spare row)
    for (; n + 1 < n1; n += 2) {
      ld_row(sb, S + (n + 1 - n0) * SLD);
      row(sa, n);
      ld_row(sa, S + (n + 2 - n0) * SLD);
      row(sb, n + 1);
    }
    if (n < n1) row(sa, n);
  };

  MONO_STAMP(0);
  for (int i = 0; i <= nblk; ++i) {
    if (w < MONO_NP) {
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
  if (w == MONO_NP) {
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
  for (int n = Ty + tid; n < a.tq; n += MONO_NT) path[n] = -1;
  for (int t = tid; t < a.tk; t += MONO_NT) dur[t] = hist[t];

  // ---- ln P along the path: the producers re-form the scores they need
  const float c = a.scale * LOG2E;
  if (w < MONO_NP) {
    if constexpr (PROD == 0) {
      for (int i = w; i < nblk; i += MONO_NP) {
        const int row = MONO_RB * i + ql;
        const int t = row < Ty ? pathL[row] : -1;
        // 32 rows advance at most 31 keys: the block's keys lie in this tile and the next
        const int t0 = __builtin_amdgcn_readfirstlane(pathL[MONO_RB * i]) / 64;
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
      for (int n = tid; n < Ty; n += 64 * MONO_NP) {
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
  const int kc = mono_kc(a.tk);
  if (kc == 128) hipLaunchKernelGGL((align_mono_kernel<128, PROD>), dim3(a.batch), dim3(MONO_NT), 0, s, a);
  else if (kc == 256) hipLaunchKernelGGL((align_mono_kernel<256, PROD>), dim3(a.batch), dim3(MONO_NT), 0, s, a);
  else hipLaunchKernelGGL((align_mono_kernel<512, PROD>), dim3(a.batch), dim3(MONO_NT), 0, s, a);
}
}  // namespace

extern "C" size_t tt2_align_monotonic_workspace_size(int batch, int tq, int tk) {
  if (batch <= 0 || tq <= 0 || tk <= 0 || tk > TT2_MONO_MAX_KEYS || mono_move_in_lds(tq, tk)) return 0;
  return (size_t)batch * mono_move_bytes(tq, tk);
}

extern "C" int tt2_align_monotonic(const tt2_align_mono_args* p, hipStream_t s) {
  const char* who = "tt2_align_monotonic";
  if (!p) return attn_err(who, "args required");
  if (p->head_dim != D) return attn_err(who, "head_dim must be 64");
  if (p->causal) return attn_err(who, "monotonic alignment search is non-causal only");
  if (p->n_layers <= 0 || p->n_layers > TT2_GUIDE_MAX_LAYERS) return attn_err(who, "needs 1..16 layers");
  if (p->dtype != TT2_DT_BF16 && p->dtype != TT2_DT_F32) return attn_err(who, "dtype must be bf16 or f32");
  if (p->variant != 0 && p->variant != 1) return attn_err(who, "variant must be 0 (auto) or 1 (plain producer)");
  if (p->batch < 0 || p->heads <= 0 || p->tq < 0 || p->tk < 0 || !(p->scale > 0.f) ||
      (int64_t)p->batch * p->heads > INT32_MAX)
    return attn_err(who, "shape / scale");
  if (p->tk > TT2_MONO_MAX_KEYS) return attn_err(who, "tk exceeds TT2_MONO_MAX_KEYS");
  if (p->tq > TT2_MONO_MAX_FRAMES) return attn_err(who, "tq exceeds TT2_MONO_MAX_FRAMES");
  const int esz = p->dtype == TT2_DT_BF16 ? 2 : 4;
  if ((p->q_ld * esz) % 16 || (p->k_ld * esz) % 16 || p->q_ld < (int64_t)p->heads * D || p->k_ld < (int64_t)p->heads * D)
    return attn_err(who, "leading dims must be 16-B multiples covering the heads");
  if (!p->path || !p->durations || !p->logp) return attn_err(who, "path / durations / logp required");
  if (!p->sel && (p->sel_layer < 0 || p->sel_layer >= p->n_layers || p->sel_head < 0 || p->sel_head >= p->heads))
    return attn_err(who, "fixed head outside the layers / heads");
  for (int l = 0; l < p->n_layers; ++l)
    if (!p->q[l] || !p->k[l] || !p->lse[l]) return attn_err(who, "q / k / lse of a layer missing");
  const size_t need = tt2_align_monotonic_workspace_size(p->batch, p->tq, p->tk);
  if (need && (!p->workspace || p->workspace_bytes < need || (reinterpret_cast<uintptr_t>(p->workspace) & 7)))
    return attn_err(who, ("workspace too small or misaligned: " + std::to_string(need) + " bytes needed").c_str());
  const bool mfma = p->dtype == TT2_DT_BF16 && p->variant != 1;
  // the buffer views address rows with 32-bit byte offsets
  if (mfma && (((int64_t)p->tq * p->q_ld + D) * 2 > INT32_MAX || ((int64_t)p->tk * p->k_ld + D) * 2 > INT32_MAX))
    return attn_err(who, "one batch element's q or k spans more than 2 GiB");
  if (p->batch == 0) return TT2_OK;
  if (mfma) mono_launch<0>(*p, s);
  else if (p->dtype == TT2_DT_BF16) mono_launch<1>(*p, s);
  else mono_launch<2>(*p, s);
  return tt2_check_launch(hipGetLastError(), who);
}
