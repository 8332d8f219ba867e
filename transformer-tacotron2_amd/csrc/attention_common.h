// attention_common.h -- what the attention translation units (attention*.hip) share.
//
// Fused scaled-dot-product attention, head dim 64 (gfx950).  One kernel family serves the three
// attention blocks of the path (SURVEY 8(a) a3 encoder self-attention, a6 decoder causal
// self-attention, a7 encoder-decoder cross-attention): Q/K/V are read in place from the fused
// projection outputs (row stride + head offset), masks are a per-batch key length and an optional
// causal flag, and the score matrix is never written to HBM (online softmax over 64-key tiles).
//
// One file per kernel family:
//   attention_v1.hip     the generic f32 / bf16 kernels (forward, prep, dQ, dK/dV; 16x16 MFMA) and
//                        the probabilities diagnostic
//   attention_fwd3.hip   the bf16 v3 forward (32x32x16 MFMA, attention_v3.h), with the ATTN_STAMP hook
//   attention_bwd3.hip   the v3 backward: dQ, dK/dV and fused bodies and kernels
//   attention_align.hip  guided-attention loss reduction, alignment statistics, durations
//   attention_mono.hip   monotonic alignment search (its own entry points)
//   attention.hip        host only: validation, the variant / parts rules, every extern "C" entry
// A family keeps its kernels in an anonymous namespace and exports host launchers (namespace tt2a,
// below) that take the C-ABI structs and plain scalars, so no unit refers to another unit's kernels
// (no relocatable device code).  Here: the tile constants, the kernels' argument structs and their
// conversion from the C ABI, the key limit, the guided-attention weight.
//
// Backward (no atomics, bitwise reproducible): a dQ kernel walks key tiles per query block, a
// dK/dV kernel walks query tiles per key block; both recompute P from the saved LSE (log2 domain,
// scores pre-multiplied by scale*log2(e); a row with no visible key stores +inf so every recomputed
// probability is exactly 0 and the output row is 0, SURVEY 8(b) mask convention).  delta =
// rowsum(dO * O) comes from attn_bwd_prep (v1) or from the v3 dQ kernel, which runs first.
#pragma once
#include <math.h>

#include <type_traits>

#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace tt2a {

// ---- per-family launchers.  The caller (attention.hip) has validated the request and chosen the
// kernel; a launcher converts the arguments, derives the grid and launches.  g: NULL for the plain
// instantiation, else the guided one.  nw: waves per work group of a v3 kernel (2 or 4). ----
// attention_v1.hip (bf16 or f32 by p->dtype)
void launch_fwd1(const tt2_attn_args* p, const tt2_attn_guide* g, hipStream_t s);
void launch_bwd_prep1(const tt2_attn_args* p, const tt2_attn_guide* g, hipStream_t s);
void launch_bwd_dq1(const tt2_attn_args* p, const tt2_attn_guide* g, hipStream_t s);
void launch_bwd_dkdv1(const tt2_attn_args* p, const tt2_attn_guide* g, hipStream_t s);
void launch_probs(const tt2_attn_args* p, float* probs, hipStream_t s);
// attention_fwd3.hip
void launch_fwd3(const tt2_attn_args* p, const tt2_attn_guide* g, int nw, hipStream_t s);
// attention_bwd3.hip (fused: nkb key blocks, then nqb query blocks, of 128 rows)
void launch_bwd_dq3(const tt2_attn_args* p, const tt2_attn_guide* g, int nw, hipStream_t s);
void launch_bwd_dkdv3(const tt2_attn_args* p, const tt2_attn_guide* g, int nw, hipStream_t s);
void launch_bwd_fused3(const tt2_attn_args* p, const tt2_attn_guide* g, int nkb, int nqb, hipStream_t s);
// attention_align.hip (align: nw 0 is the plain kernel, bf16 or f32 by p->dtype)
void launch_guide_loss(const tt2_guide_loss_args* p, bool vec, hipStream_t s);
void launch_align(const tt2_align_args* p, int nw, hipStream_t s);
void launch_align_dur(const tt2_align_dur_args* p, hipStream_t s);
constexpr int ALIGN_DUR_MAX_PAIRS = 1024;   // (layer, head) pairs align_dur_kernel's LDS table holds

}  // namespace tt2a

namespace {

constexpr int D = 64;     // head dim
constexpr int BQ = 64;    // query rows per workgroup (v1)
constexpr int BKV = 64;   // keys per tile
constexpr int NT = 256;
constexpr float LOG2E = 1.4426950408889634f;

// The kernels' argument types.  Unit-local names (as the kernels themselves), so a kernel's
// symbol does not depend on which unit holds it; they never cross units.
struct AttnArgs {
  const void* q; const void* k; const void* v; const void* o; const void* dout;
  void* out; void* dq; void* dk; void* dv;
  float* lse; float* delta;
  int64_t q_ld, k_ld, v_ld, o_ld, do_ld, dq_ld, dk_ld, dv_ld;
  const int32_t* key_len;
  int B, H, Tq, Tk, causal;
  float scale;
};
// the guided (G) instantiations' kernel argument: the same plus tt2_attn_guide
struct AttnArgsG : AttnArgs {
  const int32_t* q_len;   // valid query rows per batch (NULL: Tq)
  float* grow;            // [B*H, Tq] g = sum_t P W of each row (forward writes, backward reads)
  const float* gcoef;     // device kappa (backward)
  float gk;               // log2(e) / (2 sigma^2)
  int gheads;             // heads h < gheads are guided
};
template <bool G> using ArgsT = std::conditional_t<G, AttnArgsG, AttnArgs>;

// the C ABI's request as the kernels take it (G: g is non-NULL and checked by the caller)
template <bool G> ArgsT<G> to_args(const tt2_attn_args* p, const tt2_attn_guide* g = nullptr) {
  ArgsT<G> a;
  a.q = p->q; a.k = p->k; a.v = p->v; a.o = p->o; a.dout = p->dout;
  a.out = p->o_out; a.dq = p->dq; a.dk = p->dk; a.dv = p->dv;
  a.lse = p->lse; a.delta = p->delta;
  a.q_ld = p->q_ld; a.k_ld = p->k_ld; a.v_ld = p->v_ld; a.o_ld = p->o_ld; a.do_ld = p->do_ld;
  a.dq_ld = p->dq_ld; a.dk_ld = p->dk_ld; a.dv_ld = p->dv_ld;
  a.key_len = p->key_len;
  a.B = p->batch; a.H = p->heads; a.Tq = p->tq; a.Tk = p->tk; a.causal = p->causal;
  a.scale = p->scale;
  if constexpr (G) {
    a.q_len = g->q_len; a.grow = g->rows; a.gcoef = g->coef;
    a.gk = LOG2E / (2.f * g->sigma * g->sigma);
    a.gheads = g->heads;
  }
  return a;
}
// f(std::bool_constant<G>, the kernels' arguments) for the plain (g NULL) or the guided request
template <typename F> void with_args(const tt2_attn_args* p, const tt2_attn_guide* g, F f) {
  if (g) f(std::true_type{}, to_args<true>(p, g));
  else f(std::false_type{}, to_args<false>(p));
}

// the visible keys of batch element b (len_limit: tt2_common.h).  (Taking the arguments by
// reference is deliberate: with len_limit called on a.Tk / a.key_len at the call sites, the plain
// v1 forward, dQ and probs kernels compiled to different code.)
TT2_DEV int key_limit(const AttnArgs& a, int b) { return len_limit(a.Tk, a.key_len, b); }

// Guided attention (diagonal loss on the cross-attention, G instantiations): the weight of
// query n, key t of utterance b is W[n, t] = 1 - exp(-(t / Tx_b - n / Ty_b)^2 / (2 sigma^2)),
// Tx_b the visible keys and Ty_b the valid query rows.  Evaluated in registers from the lane's
// indices: tk = t * rk, nq = n * rq, one exp2 with log2(e) / (2 sigma^2) folded into gk.
struct Guide {
  float rk, rq;   // 1 / Tx_b, 1 / Ty_b (0 for an empty utterance)
  int qlim;       // Ty_b
  bool sel;       // this block's head is guided (block-uniform)
};
TT2_DEV Guide guide_of(const AttnArgsG& a, int b, int h, int klim) {
  Guide g;
  g.qlim = len_limit(a.Tq, a.q_len, b);
  // block-uniform, but computed by the vector ALU: moved to scalar registers by hand
  g.rk = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(klim > 0 ? 1.f / (float)klim : 0.f)));
  g.rq = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(g.qlim > 0 ? 1.f / (float)g.qlim : 0.f)));
  g.sel = h < a.gheads && klim > 0 && g.qlim > 0;
  return g;
}
template <bool FAST> TT2_DEV float guide_w(float tk, float nq, float gk) {
  const float x = tk - nq;
  const float e = -(x * x) * gk;
  return 1.f - (FAST ? __builtin_amdgcn_exp2f(e) : exp2f(e));
}

}  // namespace
