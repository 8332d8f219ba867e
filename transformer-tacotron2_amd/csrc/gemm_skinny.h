// gemm_skinny.h -- what the opt-in ffn_decode kernel (gemm_ffn_decode.hip) borrows from the
// skinny decode GEMM (gemm_skinny.hip): the column block and the element-type traits.
#pragma once
#include "gemm_common.h"

namespace {

constexpr int SK_COLS = 16;

// element type of the skinny path: bf16 (the engine's dtype) or f16 (the fp16 decode step)
template <typename TE> struct SkT;
template <> struct SkT<bf16> {
  typedef bf16x8 V;
  static TT2_DEV f32x4 mma(V a, V b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct SkT<f16> {
  typedef f16x8 V;
  static TT2_DEV f32x4 mma(V a, V b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

}  // namespace
