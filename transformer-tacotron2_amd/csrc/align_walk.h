// align_walk.h -- the walk over a (frame, key) score matrix that monotonic alignment search
// (attention_mono.hip) and the forward-sum loss (forward_sum.hip) share: its launch shape, the
// geometry of the score buffers and the move bits, the walker's row loop and the best path's row
// step.  Depends on tt2_common.h alone; the names are unit-local, as the kernels that use them.
//
// One work group per utterance: WALK_NP producer waves form the [WALK_RB rows, KC] f32 score block
// of row block i + 1 into LDS while one walker wave walks the rows of block i.  The walker holds
// its values across its lanes (lane L owns keys L*R .. L*R + R - 1) and takes the value at t - 1 of
// its first key from the lane below with one DPP wave shift.  The best-path walker writes a row's
// move bits as R ballots (bit L of word j <-> key L*R + j); the same wave then walks the bits
// backwards, 64 - R frames per pass held one frame per lane, so the serial chain is lane reads and
// scalar ops.  (The backtrack, the path / durations / logp writes and the producer / walker loop
// are written out in both best-path kernels: as functions they compiled to other instructions,
// DESIGN.md 5.16.)
#pragma once
#include <type_traits>

#include "tt2_common.h"

namespace {

constexpr int WALK_NP = 4;                    // score-producing waves
constexpr int WALK_NT = 64 * (WALK_NP + 1);   // + the walker wave
constexpr int WALK_RB = 32;                   // rows per score block
// the producers split a block's rows evenly (forward_sum.hip) or form all 32 with one 32x32 MFMA
// tile row per lane (attention_mono.hip); the walker is wave WALK_NP
static_assert(WALK_NP == 4 && WALK_RB == 32 && WALK_NT == 320, "the producers are written for this shape");

// bytes of LDS a best-path kernel of key capacity kc keeps for move bits: at 128 every length up
// to 4096 frames, above it what the score buffers and attention_mono.hip's resident K leave of 160 KiB
__host__ __device__ constexpr int walk_move_lds(int kc) { return kc == 128 ? 65536 : kc == 256 ? 49152 : 16384; }

template <int KC> struct WalkCfg {            // KC: key capacity (tk rounded up)
  static constexpr int R = KC / 64;           // keys per walker lane
  static constexpr int NK = KC / 64;          // keys per producer lane (strided by 64)
  static constexpr int SLD = KC + 4;          // score row stride in floats (spreads the producers' rows)
  static constexpr int SBUF = (WALK_RB + 1) * SLD;   // floats per score buffer (+ a row the walker's look-ahead may read)
  static constexpr int MOVE_BYTES = walk_move_lds(KC);
};
__host__ __device__ constexpr int walk_kc(int tk) { return tk <= 128 ? 128 : tk <= 256 ? 256 : 512; }
// bytes of move bits per utterance, and whether they fit the kernel's LDS share
__host__ __device__ inline size_t walk_move_bytes(int tq, int tk) { return (size_t)tq * (walk_kc(tk) / 64) * 8; }
__host__ __device__ inline bool walk_move_in_lds(int tq, int tk) {
  return walk_move_bytes(tq, tk) <= (size_t)walk_move_lds(walk_kc(tk));
}
// f(std::integral_constant<int, KC>) for the key capacity of tk keys
template <typename F> void walk_by_kc(int tk, F&& f) {
  const int kc = walk_kc(tk);
  if (kc == 128) f(std::integral_constant<int, 128>{});
  else if (kc == 256) f(std::integral_constant<int, 256>{});
  else f(std::integral_constant<int, 512>{});
}

// a lane's R consecutive floats of an LDS row
template <int R> TT2_DEV void walk_ld_row(float (&s)[R], const float* p) {
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
}

// The walker's rows of block i, from the lane's place S in the block's buffer: first(s) for row 0
// (block 0), row(s, n) for every other row n < Ty.  Two rows per trip, two register sets: each
// row's scores are read one row ahead of the chain (after the block's last row the read falls on
// the buffer's spare row).
template <int R, int SLD, typename First, typename Row>
TT2_DEV void walk_rows(const float* S, int i, int Ty, First&& first, Row&& row) {
  const int n0 = WALK_RB * i, n1 = min(n0 + WALK_RB, Ty);
  float sa[R], sb[R];
  walk_ld_row<R>(sa, S);
  int n = n0;
  if (i == 0) {
    first(sa);
    walk_ld_row<R>(sa, S + SLD);
    n = 1;
  }
  for (; n + 1 < n1; n += 2) {
    walk_ld_row<R>(sb, S + (n + 1 - n0) * SLD);
    row(sa, n);
    walk_ld_row<R>(sa, S + (n + 2 - n0) * SLD);
    row(sb, n + 1);
  }
  if (n < n1) row(sa, n);
}

// One block of the best-path (Viterbi) walk: rows of block i from the lane's place S in the block's
// buffer, the lane's values in v, a row's move bits as R ballots (bit L of word j <-> key L*R + j)
// to row n of mvL (LDSC: the kernel's LDS) or of mvG (the caller's workspace).
template <int R, int SLD, bool LDSC>
TT2_DEV void walk_block(float (&v)[R], const float* S, int i, int Ty, int lane, uint64_t* mvL, uint64_t* mvG) {
  // one row from scores s: the dependent chain is DPP shift -> compare -> select -> add
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
      if constexpr (LDSC) {
#pragma unroll
        for (int j = 0; j < R; ++j) mvL[n * R + j] = bal[j];
      } else {
#pragma unroll
        for (int j = 0; j < R; ++j) mvG[(int64_t)n * R + j] = bal[j];
      }
    }
  };
  auto first = [&](const float (&s)[R]) {   // row 0: only key 0 can be reached
#pragma unroll
    for (int j = 0; j < R; ++j) v[j] = (lane == 0 && j == 0) ? s[0] : -INFINITY;
  };
  walk_rows<R, SLD>(S, i, Ty, first, row);
}

}  // namespace
