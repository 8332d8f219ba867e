// attention_v3.h -- the v3 (32x32x16 bf16 MFMA) building blocks shared by the v3 forward, the v3
// backward, the alignment statistics and the monotonic search (attention_fwd3.hip,
// attention_bwd3.hip, attention_align.hip, attention_mono.hip): accumulator type, tile swizzle,
// buffer views, register-staged tile copies, operand fragments.
//
// v3 kernels (bf16): v_mfma_f32_32x32x16_bf16 with "swapped" products.  Every product
// puts the streamed dimension (keys in dQ / forward, queries in dK-dV) on the MFMA rows
// and the wave's own 32 rows (queries, or keys) on the lane:
//   forward  S^T = K Q^T      O^T  += V^T  P^T
//   dQ       S^T = K Q^T, dP^T = V dO^T,   dQ^T += K^T dS^T
//   dK, dV   S   = Q K^T, dP  = dO V^T,    dV^T += dO^T P,  dK^T += Q^T dS
// The 32x32 accumulator then holds, per lane, 16 streamed rows crow(r, hi) =
// (r&3) + 8(r>>2) + 4hi of ONE own row, and those 16 values ARE the B operand of the
// next product once its A operand is read transposed (ds_read_b64_tr_b16) from rows
// base + {4hi + 0..3} and base + {8 + 4hi + 0..3}.  P and dS never leave registers,
// softmax statistics are per lane (one xor-32 shuffle per tile), and each LDS fragment
// feeds a 32-row MFMA (32 FLOP per LDS byte: the LDS array is not the bound).
// Tiles are 64 rows x 64 bf16 in LDS with the chunk swizzle below, double-buffered and
// register-staged (global loads for tile t+1 in flight while tile t computes).
#pragma once
#include "attention_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

TT2_DEV void mma32(const bf16x8& a, const bf16x8& b, f32x16& c) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
TT2_DEV float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// 16-B chunk c of tile row r lives at slot c ^ swz(r), swz(r) = h((r >> 1) & 7) with
// h(x) = ((x & 1) << 2) | (x >> 1).  Row reads (ds_read_b128: 16 distinct rows mod 16
// per lane group) and 4-row transposed reads (ds_read_b64_tr_b16: rows 4i..4i+3 x one
// 4-chunk half per 32-lane group) are both bank-conflict-free.
TT2_DEV int swz(int r) {
  const int x = (r >> 1) & 7;
  return ((x & 1) << 2) | (x >> 1);
}
TT2_DEV int toff(int r, int col) { return r * D + ((((col >> 3) ^ swz(r))) << 3) + (col & 7); }

template <int NTH> struct Stage3 { static constexpr int PER = 64 * 8 / NTH; };

// Buffer view of one (batch, head) slice of a [T rows][ld] bf16 matrix: rows >= T fall
// outside num_records and load as zeros (no per-row branches or exec masking).
struct RowBuf {
  __amdgpu_buffer_rsrc_t rs;
  int ldb;   // row stride in bytes
};
TT2_DEV RowBuf row_buf(const bf16* base, int64_t ld, int T) {
  RowBuf r;
  r.ldb = (int)(ld * 2);
  const int bytes = T > 0 ? (T - 1) * r.ldb + D * 2 : 0;
  r.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(base), (short)0, bytes, 0x00020000);
  return r;
}
TT2_DEV uint4 buf_ld16(const RowBuf& b, int row, int chunk) {
  auto v = __builtin_amdgcn_raw_buffer_load_b128(b.rs, row * b.ldb + chunk * 16, 0, 0);
  return make_uint4(v[0], v[1], v[2], v[3]);
}

template <int NTH>
TT2_DEV void g2r3(uint4 (&r)[Stage3<NTH>::PER], const RowBuf& g, int row0, int tid) {
#pragma unroll
  for (int i = 0; i < Stage3<NTH>::PER; ++i) {
    const int c = tid + NTH * i;
    r[i] = buf_ld16(g, row0 + (c >> 3), c & 7);
  }
}
template <int NTH>
TT2_DEV void r2s3(const uint4 (&r)[Stage3<NTH>::PER], bf16* s, int tid) {
#pragma unroll
  for (int i = 0; i < Stage3<NTH>::PER; ++i) {
    const int c = tid + NTH * i, rr = c >> 3, cc = c & 7;
    *reinterpret_cast<uint4*>(s + rr * D + ((cc ^ swz(rr)) << 3)) = r[i];
  }
}
// A operand rows: X[row][16 st + 8 hi + j]
TT2_DEV bf16x8 rowfrag(const bf16* t, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(t + row * D + ((chunk ^ swz(row)) << 3));
}
// A operand X^T[d = 32 db + (lane & 31)][k = 8 hi + j], k <-> tile row base + 8(j>>2) + 4hi + (j&3)
TT2_DEV bf16x8 trfrag(const bf16* t, int base, int db, int lane) {
  typedef __attribute__((address_space(3))) short4v lds_s4;
  const int hi = lane >> 5, q = (lane >> 2) & 3, p = lane & 3, g = (lane >> 4) & 1;
  const int col = 32 * db + 16 * g + 4 * p;
  const int r0 = base + 4 * hi + q;
  short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(t + toff(r0, col)));
  short4v up = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(t + toff(r0 + 8, col)));
  union { short4v s[2]; bf16x8 v; } u;
  u.s[0] = lo;
  u.s[1] = up;
  return u.v;
}
// own-row fragments: X[row][16 st + 8 hi + j], st = 0..3 (zeros past the last row)
TT2_DEV void own_frags(bf16x8 (&f)[4], const RowBuf& X, int row, int hi) {
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    union { uint4 u; bf16x8 v; } x;
    x.u = buf_ld16(X, row, 2 * st + hi);
    f[st] = x.v;
  }
}
// value of lane l ^ 32 combined with lane l's: v_permlane32_swap instead of ds_bpermute
TT2_DEV float xor32_max(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
TT2_DEV float xor32_sum(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
TT2_DEV int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }
// store the lane's 16 accumulator rows (d = 32 db + crow) of one output row
TT2_DEV void store_rowT(bf16* row, const f32x16 (&acc)[2], float sc, int hi) {
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      bf16x4 x;
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = (bf16)(acc[db][4 * rr + i] * sc);
      *reinterpret_cast<bf16x4*>(row + 32 * db + 8 * rr + 4 * hi) = x;
    }
}
TT2_DEV void zero16(f32x16& x) {
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = 0.f;
}

}  // namespace
