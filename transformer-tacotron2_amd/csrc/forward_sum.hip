// forward_sum.hip -- the forward-sum alignment loss over a (frame, phoneme) score matrix: the total
// probability of all monotone alignments (tt2_forward_sum_fwd), its gradient and posterior
// (tt2_forward_sum_bwd) and its best path (tt2_forward_sum_path).  tt2_capi.h states the
// definition.  A translation unit of its own: no other kernel's code depends on it.  The launch
// shape is align_walk.h's: one work group per utterance, WALK_NP producer waves form 32-row blocks
// into double-buffered LDS while one wave walks the recurrence with a contiguous run of keys per
// lane and takes its neighbour's value by a DPP wave shift.
//
//   fsum_walk_kernel<KC, DIR>   DIR 0: the alpha pass.  The producers form ls = s - lse (the row
//                               log-sum-exp is theirs and goes to `lse`); the walker adds in log
//                               space, subtracts the row's maximum after every row, sums the maxima
//                               in float64 and stores the renormalised alpha.
//                               DIR 1: the beta pass, which is the alpha recurrence with rows and
//                               keys read backwards from (Ty - 1, Te - 1); it stores beta (the
//                               logaddexp before the row's ls is added) in walk order.
//   fsum_grad_kernel            a wave per row: gamma = softmax_t(alpha + beta), P = exp(s - lse),
//                               dscores = grad_loss * (P - gamma), +0 in the padding.
//   fsum_path_kernel<KC>        the best path: align_walk.h's Viterbi walk over the raw scores, the
//                               backtrack over its move bits, then ls along the path.
#include <limits.h>
#include <math.h>

#include "tt2_capi.h"
#include "tt2_internal.h"
#include "align_walk.h"

namespace {

constexpr float FS_NEG = -1e30f;            // a cell no path reaches (finite: NEG - NEG is 0, not NaN)
constexpr int FS_GRAD_ROWS = 4;             // fsum_grad_kernel: rows (waves) per work group
// rows between two renormalisations of the walker (a build knob for the measurement in DESIGN.md 5.14;
// the library is built with 1: the row's maximum is subtracted after every row)
#ifndef FS_RENORM
#define FS_RENORM 1
#endif

// wave_sum's lane pattern with max
TT2_DEV float fs_wave_max(float v) {
  v = fmaxf(v, dpp_f32<0xB1>(v));
  v = fmaxf(v, dpp_f32<0x4E>(v));
  v = fmaxf(v, dpp_f32<0x141>(v));
  v = fmaxf(v, dpp_f32<0x140>(v));
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// ln(e^a + e^b) for finite a, b (FS_NEG included), on the walker's serial chain: m + ln(1 + e) with
// e = exp(min - m) <= 1 through v_exp_f32, and ln(1 + e) through v_log_f32 or, below 2^-12 where 1 + e
// would drop e's low bits, its series e - e^2 / 2 (the next term is under 2^-37).  The absolute error
// is about 2^-24, the rounding of the sum itself once |m| reaches 1/2; ocml's expf and log1pf in its
// place measured 607 ns a row against this form's figure in DESIGN.md 5.14.
constexpr float FS_LOG2E = 1.4426950408889634f;
TT2_DEV float fs_lae(float a, float b) {
  const float m = fmaxf(a, b);
  const float e = __builtin_amdgcn_exp2f((fminf(a, b) - m) * FS_LOG2E);
  const float r = e < 0x1p-12f ? e * (1.f - 0.5f * e) : LN2 * __builtin_amdgcn_logf(1.f + e);
  return m + r;
}

// One wave: the keys t = lane + 64 k < Tx of a score row into x (-inf past Tx), and the row's
// log-sum-exp in two parts, the maximum m and ln sum exp(s - m) (returned): each lane's exponentials
// added with k ascending, the lanes by wave_sum's tree.  ls = (s - m) - that logarithm keeps the
// precision of a small ls where s - (m + logarithm) would round at the size of the scores.
template <int NK> TT2_DEV void fs_row_load(const float* row, int Tx, int lane, float (&x)[NK]) {
#pragma unroll
  for (int k = 0; k < NK; ++k) x[k] = lane + 64 * k < Tx ? row[lane + 64 * k] : -INFINITY;
}
template <int NK> TT2_DEV float fs_row_lse(int Tx, int lane, const float (&x)[NK], float& m) {
  m = -INFINITY;
#pragma unroll
  for (int k = 0; k < NK; ++k) m = fmaxf(m, x[k]);
  m = fs_wave_max(m);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k)
    if (lane + 64 * k < Tx) sum += expf(x[k] - m);
  return logf(wave_sum(sum));
}

// a lane's R consecutive floats to a row (walk_ld_row's counterpart)
template <int R> TT2_DEV void fs_st_row(float* p, const float (&s)[R]) {
  if constexpr (R == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(s[0], s[1]);
  } else {
#pragma unroll
    for (int q = 0; q < R / 4; ++q)
      *reinterpret_cast<float4*>(p + 4 * q) = make_float4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
  }
}

// Walk row m and walk key p are frame m and key p for DIR 0, frame Ty - 1 - m and key Te - 1 - p
// for DIR 1; keys at and past Te keep their place.
template <int KC, int DIR>
__global__ __launch_bounds__(WALK_NT) void fsum_walk_kernel(tt2_forward_sum_args a) {
  using C = WalkCfg<KC>;
  constexpr int R = C::R, NK = C::NK, SLD = C::SLD, SBUF = C::SBUF;
  __shared__ __attribute__((aligned(16))) float sS[2 * SBUF];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x;
  const int Ty = len_limit(a.tq, a.q_len, b);
  const int Tx = len_limit(a.tk, a.key_len, b);
  const int Te = min(Tx, Ty);
  float* lse = a.lse + (int64_t)b * a.tq;
  if constexpr (DIR == 0) {
    for (int n = Ty + tid; n < a.tq; n += WALK_NT) lse[n] = 0.f;
    if (Ty <= 0 || Tx <= 0) {   // block-uniform
      for (int n = tid; n < Ty; n += WALK_NT) lse[n] = 0.f;
      if (tid == 0) a.loss[b] = 0.f;
      return;
    }
  } else {
    if (Ty <= 0 || Tx <= 0) return;
  }
  const float* sc = a.scores + (int64_t)b * a.s_bs;
  float* out = DIR == 0 ? (a.alpha ? a.alpha + (int64_t)b * a.tq * a.a_ld : nullptr)
                        : static_cast<float*>(a.workspace) + (int64_t)b * a.tq * KC;
  const int nblk = (Ty + WALK_RB - 1) / WALK_RB;

  // ---- rows of block i -> buffer i & 1 (producer waves, a wave per row)
  auto produce = [&](int i) {
    float* S = sS + (i & 1) * SBUF;
    constexpr int PR = WALK_RB / WALK_NP;   // rows per producer wave, their loads issued together
    float x[PR][NK];
#pragma unroll
    for (int q = 0; q < PR; ++q) {
      const int m = WALK_RB * i + w + WALK_NP * q;
      if (m < Ty) fs_row_load<NK>(sc + (int64_t)(DIR ? Ty - 1 - m : m) * a.s_ld, Tx, lane, x[q]);
    }
#pragma unroll
    for (int q = 0; q < PR; ++q) {
      const int r = w + WALK_NP * q, m = WALK_RB * i + r;
      if (m >= Ty) break;
      const int n = DIR ? Ty - 1 - m : m;
      float mx;
      const float l = fs_row_lse<NK>(Tx, lane, x[q], mx);   // (both passes: the same bits of ls)
      if constexpr (DIR == 0) {
        if (lane == 0) lse[n] = mx + l;
      }
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int t = lane + 64 * k;
        S[r * SLD + (t < Te ? (DIR ? Te - 1 - t : t) : t)] = t < Te ? (x[q][k] - mx) - l : FS_NEG;
      }
    }
  };

  // ---- the walker: rows of block i from buffer i & 1
  float v[R];
  double off = 0.0;   // the sum of the rows' maxima (DIR 0)
#pragma unroll
  for (int j = 0; j < R; ++j) v[j] = FS_NEG;
  // renormalise row m (nv: its values, lab: the logaddexp they came from) and store it
  auto finish = [&](const float (&nv)[R], const float (&lab)[R], int m) {
    float mx = 0.f;
    if (FS_RENORM == 1 || m % FS_RENORM == 0) {
      mx = nv[0];
#pragma unroll
      for (int j = 1; j < R; ++j) mx = fmaxf(mx, nv[j]);
      mx = fs_wave_max(mx);
    }
#pragma unroll
    for (int j = 0; j < R; ++j) v[j] = fmaxf(nv[j] - mx, FS_NEG);
    if constexpr (DIR == 0) {
      off += (double)mx;
      if (out) {
        float* o = out + (int64_t)m * a.a_ld + lane * R;
#pragma unroll
        for (int j = 0; j < R; ++j)
          if (lane * R + j < Te) o[j] = v[j];
      }
    } else {
      fs_st_row<R>(out + (int64_t)m * KC + lane * R, lab);
    }
  };
  auto consume = [&](int i) {
    const float* S = sS + (i & 1) * SBUF + lane * R;
    auto row = [&](const float (&s)[R], int m) {
      // the value at p - 1 of the lane's first key: the last key of the lane below (wave_shr:1)
      const float below = __int_as_float(__builtin_amdgcn_update_dpp(
          __float_as_int(FS_NEG), __float_as_int(v[R - 1]), 0x138, 0xF, 0xF, false));
      float nv[R], lab[R];
#pragma unroll
      for (int j = R - 1; j >= 0; --j) {
        lab[j] = fs_lae(v[j], j ? v[j - 1] : below);
        nv[j] = s[j] + lab[j];
      }
      finish(nv, lab, m);
    };
    auto row0 = [&](const float (&s)[R]) {   // walk row 0: only walk key 0 can be reached
      float nv[R], lab[R];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const bool first = lane == 0 && j == 0;
        nv[j] = first ? s[0] : FS_NEG;
        lab[j] = first ? 0.f : FS_NEG;
      }
      finish(nv, lab, 0);
    };
    walk_rows<R, SLD>(S, i, Ty, row0, row);
  };

  for (int i = 0; i <= nblk; ++i) {
    if (w < WALK_NP) {
      if (i < nblk) produce(i);
    } else if (i > 0) {
      consume(i - 1);
    }
    __syncthreads();
  }

  if constexpr (DIR == 0) {
    if (w == WALK_NP) {   // ln Z = the offsets + the last row's value at key Te - 1
      const int p = Te - 1;
      float val = v[0];
#pragma unroll
      for (int j = 1; j < R; ++j) val = (p % R) == j ? v[j] : val;
      if (lane == p / R) a.loss[b] = (float)(0.0 - (off + (double)val));
    }
  }
}

// gamma and dscores of one row per wave, from alpha, the beta pass's workspace, the scores and lse
__global__ __launch_bounds__(64 * FS_GRAD_ROWS) void fsum_grad_kernel(tt2_forward_sum_args a, int kc, int blocks) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x / (unsigned)blocks;
  const int n = (blockIdx.x % (unsigned)blocks) * FS_GRAD_ROWS + w;
  if (n >= a.tq) return;   // wave-uniform
  const int Ty = len_limit(a.tq, a.q_len, b);
  const int Tx = len_limit(a.tk, a.key_len, b);
  const int Te = min(Tx, Ty);
  float* d = a.dscores ? a.dscores + (int64_t)b * a.d_bs + (int64_t)n * a.d_ld : nullptr;
  float* gm = a.gamma ? a.gamma + (int64_t)b * a.g_bs + (int64_t)n * a.g_ld : nullptr;
  if (n >= Ty || Tx <= 0) {
    for (int t = lane; t < a.tk; t += 64) {
      if (d) d[t] = 0.f;
      if (gm) gm[t] = 0.f;
    }
    return;
  }
  const float g = a.grad_loss ? a.grad_loss[b] : 1.f;
  const float* al = a.alpha + ((int64_t)b * a.tq + n) * a.a_ld;
  const float* be = static_cast<const float*>(a.workspace) + ((int64_t)b * a.tq + (Ty - 1 - n)) * kc;
  const float* row = a.scores + (int64_t)b * a.s_bs + (int64_t)n * a.s_ld;
  const float l = a.lse[(int64_t)b * a.tq + n];
  constexpr int NK = TT2_FSUM_MAX_KEYS / 64;
  float x[NK];
  float mx = FS_NEG;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int t = lane + 64 * k;
    x[k] = t < Te ? al[t] + be[Te - 1 - t] : FS_NEG;
    mx = fmaxf(mx, x[k]);
  }
  mx = fs_wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    x[k] = lane + 64 * k < Te ? expf(x[k] - mx) : 0.f;
    sum += x[k];
  }
  sum = wave_sum(sum);
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int t = lane + 64 * k;
    if (t < a.tk) {
      float gam = 0.f, dv = 0.f;
      if (t < Tx) {
        gam = x[k] / sum;
        dv = g * (expf(row[t] - l) - gam);
      }
      if (d) d[t] = dv;
      if (gm) gm[t] = gam;
    }
  }
}

// The best path over the raw scores: align_mono_kernel's search (attention_mono.hip) with the score
// block copied from memory and ls in place of ln P
template <int KC>
__global__ __launch_bounds__(WALK_NT) void fsum_path_kernel(tt2_forward_sum_args a) {
  using C = WalkCfg<KC>;
  constexpr int R = C::R, NK = C::NK, SLD = C::SLD, SBUF = C::SBUF;
  __shared__ __attribute__((aligned(16))) char smem[2 * SBUF * 4 + C::MOVE_BYTES + KC * 4];
  float* sS = reinterpret_cast<float*>(smem);
  int* hist = reinterpret_cast<int*>(smem + 2 * SBUF * 4 + C::MOVE_BYTES);
  // after the walk the score buffers hold the path and the per-row log-probabilities
  int* pathL = reinterpret_cast<int*>(sS);
  float* termL = sS + SBUF;
  static_assert(SBUF >= TT2_FSUM_MAX_FRAMES, "path / terms alias one score buffer each");

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x;
  const int Ty = len_limit(a.tq, a.q_len, b);
  const int Tx = len_limit(a.tk, a.key_len, b);
  const int Te = min(Tx, Ty);
  int32_t* path = a.path + (int64_t)b * a.tq;
  int32_t* dur = a.durations + (int64_t)b * a.tk;
  if (Ty <= 0 || Tx <= 0) {   // block-uniform
    for (int n = tid; n < a.tq; n += WALK_NT) path[n] = -1;
    for (int t = tid; t < a.tk; t += WALK_NT) dur[t] = 0;
    if (tid == 0) a.logp[b] = 0.f;
    return;
  }
  const float* sc = a.scores + (int64_t)b * a.s_bs;
  const bool mv_lds = walk_move_in_lds(a.tq, a.tk);
  uint64_t* mvL = reinterpret_cast<uint64_t*>(smem + 2 * SBUF * 4);
  uint64_t* mvG = reinterpret_cast<uint64_t*>(a.workspace) + (int64_t)b * a.tq * R;
  const int nblk = (Ty + WALK_RB - 1) / WALK_RB;

  for (int t = tid; t < KC; t += WALK_NT) hist[t] = 0;

  auto produce = [&](int i) {
    float* S = sS + (i & 1) * SBUF;
    constexpr int PR = WALK_RB / WALK_NP;   // rows per producer wave, their loads issued together
    float x[PR][NK];
#pragma unroll
    for (int q = 0; q < PR; ++q) {
      const int n = WALK_RB * i + w + WALK_NP * q;
      if (n < Ty) fs_row_load<NK>(sc + (int64_t)n * a.s_ld, Te, lane, x[q]);
    }
#pragma unroll
    for (int q = 0; q < PR; ++q) {
      const int r = w + WALK_NP * q;
      if (WALK_RB * i + r >= Ty) break;
#pragma unroll
      for (int k = 0; k < NK; ++k) S[r * SLD + lane + 64 * k] = x[q][k];
    }
  };

  float v[R];
#pragma unroll
  for (int j = 0; j < R; ++j) v[j] = -INFINITY;
  auto consume = [&](int i, auto LDSC) {   // LDSC: the move words go to LDS (else to the workspace)
    const float* S = sS + (i & 1) * SBUF + lane * R;
    walk_block<R, SLD, decltype(LDSC)::value>(v, S, i, Ty, lane, mvL, mvG);
  };

  for (int i = 0; i <= nblk; ++i) {
    if (w < WALK_NP) {
      if (i < nblk) produce(i);
    } else if (i > 0) {
      if (mv_lds) consume(i - 1, std::true_type{});
      else consume(i - 1, std::false_type{});
    }
    __syncthreads();
  }

  // ---- backtrack (the walker wave, which wrote the bits), CH frames at a time
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
  __syncthreads();
  for (int n = Ty + tid; n < a.tq; n += WALK_NT) path[n] = -1;
  for (int t = tid; t < a.tk; t += WALK_NT) dur[t] = hist[t];

  // ---- ls along the path: a wave per row forms the row's log-sum-exp as the forward does, LB rows'
  // loads issued together
  constexpr int LB = 4;
  for (int n0 = w * LB; n0 < Ty; n0 += (WALK_NP + 1) * LB) {
    float x[LB][NK], sp[LB];
#pragma unroll
    for (int q = 0; q < LB; ++q) {
      const int n = n0 + q;
      if (n < Ty) {
        const float* row = sc + (int64_t)n * a.s_ld;
        fs_row_load<NK>(row, Tx, lane, x[q]);
        sp[q] = row[pathL[n]];
      }
    }
#pragma unroll
    for (int q = 0; q < LB; ++q) {
      const int n = n0 + q;
      if (n >= Ty) break;
      float mx;
      const float l = fs_row_lse<NK>(Tx, lane, x[q], mx);
      if (lane == 0) termL[n] = (sp[q] - mx) - l;
    }
  }
  __syncthreads();
  if (w == 0) {   // fixed order: lane-strided partial sums, then the tree
    float acc = 0.f;
    for (int n = lane; n < Ty; n += 64) acc += termL[n];
    acc = wave_sum(acc);
    if (lane == 0) a.logp[b] = acc / (float)Ty;
  }
}

// What the three entries refuse alike
int fs_check(const char* who, const tt2_forward_sum_args* p) {
  if (!p) return tt2_invalid(who, "args required");
  if (p->batch < 0 || p->tq < 0 || p->tk < 0) return tt2_invalid(who, "negative batch / tq / tk");
  if (p->tk > TT2_FSUM_MAX_KEYS) return tt2_invalid(who, "tk above TT2_FSUM_MAX_KEYS");
  if (p->tq > TT2_FSUM_MAX_FRAMES) return tt2_invalid(who, "tq above TT2_FSUM_MAX_FRAMES");
  if (p->s_ld < p->tk) return tt2_invalid(who, "s_ld < tk");
  return TT2_OK;
}

template <int DIR> void fs_walk_launch(const tt2_forward_sum_args& a, hipStream_t s) {
  walk_by_kc(a.tk, [&](auto kc) {
    hipLaunchKernelGGL((fsum_walk_kernel<decltype(kc)::value, DIR>), dim3(a.batch), dim3(WALK_NT), 0, s, a);
  });
}

}  // namespace

extern "C" size_t tt2_forward_sum_bwd_workspace_size(int batch, int tq, int tk) {
  if (batch <= 0 || tq <= 0 || tk <= 0 || tk > TT2_FSUM_MAX_KEYS) return 0;
  return (size_t)batch * tq * walk_kc(tk) * sizeof(float);
}

extern "C" size_t tt2_forward_sum_path_workspace_size(int batch, int tq, int tk) {
  if (batch <= 0 || tq <= 0 || tk <= 0 || tk > TT2_FSUM_MAX_KEYS || walk_move_in_lds(tq, tk)) return 0;
  return (size_t)batch * walk_move_bytes(tq, tk);
}

extern "C" int tt2_forward_sum_fwd(const tt2_forward_sum_args* p, hipStream_t s) {
  const char* who = "tt2_forward_sum_fwd";
  const int rc = fs_check(who, p);
  if (rc != TT2_OK) return rc;
  if (p->alpha && p->a_ld < p->tk) return tt2_invalid(who, "a_ld < tk");
  if (p->batch == 0) return TT2_OK;
  if (!p->loss) return tt2_invalid(who, "loss required");
  if (p->tq > 0 && !p->lse) return tt2_invalid(who, "lse required");
  if (p->tq > 0 && p->tk > 0 && !p->scores) return tt2_invalid(who, "scores required");
  fs_walk_launch<0>(*p, s);
  return tt2_check_launch(hipGetLastError(), who);
}

extern "C" int tt2_forward_sum_bwd(const tt2_forward_sum_args* p, hipStream_t s) {
  const char* who = "tt2_forward_sum_bwd";
  int rc = fs_check(who, p);
  if (rc != TT2_OK) return rc;
  if (p->a_ld < p->tk) return tt2_invalid(who, "a_ld < tk");
  if (p->dscores && p->d_ld < p->tk) return tt2_invalid(who, "d_ld < tk");
  if (p->gamma && p->g_ld < p->tk) return tt2_invalid(who, "g_ld < tk");
  const int blocks = (p->tq + FS_GRAD_ROWS - 1) / FS_GRAD_ROWS;
  if ((int64_t)p->batch * blocks > INT_MAX) return tt2_invalid(who, "more than 2^31 - 1 work groups");
  rc = tt2_need_workspace(who, p->workspace, p->workspace_bytes,
                          tt2_forward_sum_bwd_workspace_size(p->batch, p->tq, p->tk), 16);
  if (rc != TT2_OK) return rc;
  if (p->batch == 0 || p->tq == 0 || p->tk == 0) return TT2_OK;
  if (!p->dscores && !p->gamma) return tt2_invalid(who, "dscores or gamma required");
  if (!p->scores || !p->lse || !p->alpha) return tt2_invalid(who, "scores, lse and alpha required");
  fs_walk_launch<1>(*p, s);
  rc = tt2_check_launch(hipGetLastError(), who);
  if (rc != TT2_OK) return rc;
  hipLaunchKernelGGL(fsum_grad_kernel, dim3((unsigned)(p->batch * blocks)), dim3(64 * FS_GRAD_ROWS), 0, s, *p,
                     walk_kc(p->tk), blocks);
  return tt2_check_launch(hipGetLastError(), who);
}

extern "C" int tt2_forward_sum_path(const tt2_forward_sum_args* p, hipStream_t s) {
  const char* who = "tt2_forward_sum_path";
  int rc = fs_check(who, p);
  if (rc != TT2_OK) return rc;
  rc = tt2_need_workspace(who, p->workspace, p->workspace_bytes,
                          tt2_forward_sum_path_workspace_size(p->batch, p->tq, p->tk), 8);
  if (rc != TT2_OK) return rc;
  if (p->batch == 0) return TT2_OK;
  if (!p->logp || (p->tq > 0 && !p->path) || (p->tk > 0 && !p->durations))
    return tt2_invalid(who, "path, durations and logp required");
  if (p->tq > 0 && p->tk > 0 && !p->scores) return tt2_invalid(who, "scores required");
  walk_by_kc(p->tk, [&](auto kc) {
    hipLaunchKernelGGL(fsum_path_kernel<decltype(kc)::value>, dim3(p->batch), dim3(WALK_NT), 0, s, *p);
  });
  return tt2_check_launch(hipGetLastError(), who);
}
