// attention.hip -- the attention entry points: request validation and kernel choice (host only, no
// device code).  Every family's rules live here -- which kernel serves a request (variant, dtype,
// the 2-wave / 4-wave auto rule), the guided-argument checks, the `parts` rules, the shape limits
// of the alignment kernels -- and the family units (attention_common.h has the map) only convert
// the arguments, derive the grid and launch.
#include "attention_common.h"

using namespace tt2a;

namespace {

int validate(const tt2_attn_args* p) {
  if (p->head_dim != D) return tt2_set_error(TT2_E_INVALID, "tt2_attn: head_dim must be 64");
  const int esz = p->dtype == TT2_DT_BF16 ? 2 : 4;
  const int64_t lds[] = {p->q_ld, p->k_ld, p->v_ld};
  for (int64_t ld : lds)
    if ((ld * esz) % 16) return tt2_set_error(TT2_E_INVALID, "tt2_attn: leading dims must be 16-B multiples");
  return TT2_OK;
}

// guided launches: non-causal only (the loss is defined on encoder-decoder attention)
int check_guide(const tt2_attn_args* p, const tt2_attn_guide* g, bool bwd, const char* who) {
  if (!g) return tt2_invalid(who, "guide required");
  if (p->causal) return tt2_invalid(who, "guided attention is non-causal only");
  if (!g->rows || (bwd && !g->coef)) return tt2_invalid(who, "guide rows / coef required");
  if (!(g->sigma > 0.f) || g->heads < 0 || g->heads > p->heads)
    return tt2_invalid(who, "guide needs sigma > 0 and 0 <= heads <= the attention's heads");
  return TT2_OK;
}

// Waves per work group of the v3 kernel that serves `rows` rows (queries, or keys in dK / dV) of
// each of `slices` (batch, head[, layer]) slices; 0: the v1 kernel.
// variant: 0 auto (bf16 -> v3, f32 -> v1), 1 v1, 2 v3 with 2 waves/workgroup, 3 v3 with 4.
int v3_waves(int dtype, int variant, int rows, int64_t slices, bool fwd) {
  if (dtype != TT2_DT_BF16 || variant == 1) return 0;
  if (variant == 2) return 2;
  if (variant == 3) return 4;
  // auto: the forward shares each K/V tile across 4 waves (128 queries) while that
  // still gives two workgroups per CU; the backward kernels (buffer-unrolled loops)
  // measure fastest with 4-wave workgroups at every shape of the workload.
  const int64_t wg4 = (int64_t)((rows + 127) / 128) * slices;
  return !fwd || wg4 >= 512 ? 4 : 2;
}
int v3_waves(const tt2_attn_args* p, int rows, bool fwd) {
  return v3_waves(p->dtype, p->variant, rows, (int64_t)p->batch * p->heads, fwd);
}

int attn_fwd(const tt2_attn_args* p, const tt2_attn_guide* g, bool guided, hipStream_t s, const char* who) {
  if (int rc = validate(p)) return rc;
  if (!p->o_out || !p->lse) return tt2_invalid(who, "out/lse required");
  if (guided)
    if (int rc = check_guide(p, g, false, who)) return rc;
  if (p->batch * p->tq == 0) return TT2_OK;
  const int nw = v3_waves(p, p->tq, true);
  if (nw) launch_fwd3(p, g, nw, s);
  else launch_fwd1(p, g, s);
  return tt2_check_launch(hipGetLastError(), who);
}

int attn_bwd(const tt2_attn_args* p, const tt2_attn_guide* g, bool guided, hipStream_t s, const char* who) {
  if (int rc = validate(p)) return rc;
  if (!p->dq || !p->dk || !p->dv || !p->delta || !p->lse || !p->o || !p->dout)
    return tt2_invalid(who, "missing buffer");
  if (guided)
    if (int rc = check_guide(p, g, true, who)) return rc;
  if (p->batch * p->tq == 0) return TT2_OK;
  const int nq = v3_waves(p, p->tq, false), nk = v3_waves(p, p->tk, false);
  // the v3 dQ kernel computes delta = rowsum(dO * O) itself (and stores it for dK / dV).
  // Non-causal: dQ and dK / dV workgroups in one launch (the causal case gained nothing
  // from the same fusion)
  if (nq == 4 && nk == 4 && !p->causal) {
    // parts: both halves (the dK / dV blocks compute delta themselves, the dQ blocks do not
    // publish it), or one of them alone
    const int nkb = p->parts == 1 ? 0 : (p->tk + 127) / 128, nqb = p->parts == 2 ? 0 : (p->tq + 127) / 128;
    launch_bwd_fused3(p, g, nkb, nqb, s);
    return tt2_check_launch(hipGetLastError(), who);
  }
  if (p->parts != 0)
    return tt2_invalid(who, p->dtype == TT2_DT_BF16 ? "parts needs the non-causal bf16 launch (4-wave v3)" : "parts needs bf16");
  if (nq == 0) launch_bwd_prep1(p, g, s);
  if (nq) launch_bwd_dq3(p, g, nq, s);
  else launch_bwd_dq1(p, g, s);
  if (nk) launch_bwd_dkdv3(p, g, nk, s);
  else launch_bwd_dkdv1(p, g, s);
  return tt2_check_launch(hipGetLastError(), who);
}

}  // namespace

extern "C" int tt2_attn_fwd(const tt2_attn_args* p, hipStream_t s) {
  return attn_fwd(p, nullptr, false, s, "tt2_attn_fwd");
}

extern "C" int tt2_attn_fwd_guided(const tt2_attn_args* p, const tt2_attn_guide* g, hipStream_t s) {
  return attn_fwd(p, g, true, s, "tt2_attn_fwd_guided");
}

extern "C" int tt2_attn_bwd(const tt2_attn_args* p, hipStream_t s) {
  return attn_bwd(p, nullptr, false, s, "tt2_attn_bwd");
}

extern "C" int tt2_attn_bwd_guided(const tt2_attn_args* p, const tt2_attn_guide* g, hipStream_t s) {
  return attn_bwd(p, g, true, s, "tt2_attn_bwd_guided");
}

extern "C" int tt2_attn_probs(const tt2_attn_args* p, float* probs, hipStream_t s) {
  if (int rc = validate(p)) return rc;
  if (!p->lse || !probs) return tt2_set_error(TT2_E_INVALID, "tt2_attn_probs: lse / probs required");
  if (p->batch * p->tq * p->tk == 0) return TT2_OK;
  launch_probs(p, probs, s);
  return tt2_check_launch(hipGetLastError(), "tt2_attn_probs");
}

extern "C" int tt2_guided_attn_loss(const tt2_guide_loss_args* p, hipStream_t s) {
  const char* who = "tt2_guided_attn_loss";
  if (!p || !p->term || !p->coef) return tt2_invalid(who, "term / coef required");
  if (p->n_layers < 0 || p->n_layers > TT2_GUIDE_MAX_LAYERS) return tt2_invalid(who, "too many layers");
  if (p->batch < 0 || p->tq < 0 || p->tk < 0 || p->heads <= 0 || p->guide_heads < 0 || p->guide_heads > p->heads ||
      (int64_t)p->heads * p->tq > INT32_MAX)
    return tt2_invalid(who, "shape");
  for (int l = 0; l < p->n_layers; ++l)
    if (!p->rows[l]) return tt2_invalid(who, "rows buffer missing");
  bool vec = ((int64_t)p->guide_heads * p->tq) % 4 == 0 && ((int64_t)p->heads * p->tq) % 4 == 0;
  for (int l = 0; l < p->n_layers; ++l) vec = vec && reinterpret_cast<uintptr_t>(p->rows[l]) % 16 == 0;
  launch_guide_loss(p, vec, s);
  return tt2_check_launch(hipGetLastError(), who);
}

extern "C" int tt2_attn_align(const tt2_align_args* p, hipStream_t s) {
  const char* who = "tt2_attn_align";
  if (!p) return tt2_invalid(who, "args required");
  if (p->head_dim != D) return tt2_invalid(who, "head_dim must be 64");
  if (p->causal) return tt2_invalid(who, "alignment statistics are non-causal only");
  if (p->n_layers < 0 || p->n_layers > TT2_GUIDE_MAX_LAYERS) return tt2_invalid(who, "too many layers");
  if (p->dtype != TT2_DT_BF16 && p->dtype != TT2_DT_F32) return tt2_invalid(who, "dtype must be bf16 or f32");
  if (p->batch < 0 || p->heads <= 0 || p->tq < 0 || p->tk < 0 || !(p->scale > 0.f) ||
      (int64_t)p->batch * p->heads > INT32_MAX)
    return tt2_invalid(who, "shape / scale");
  const int esz = p->dtype == TT2_DT_BF16 ? 2 : 4;
  if ((p->q_ld * esz) % 16 || (p->k_ld * esz) % 16 || p->q_ld < (int64_t)p->heads * D || p->k_ld < (int64_t)p->heads * D)
    return tt2_invalid(who, "leading dims must be 16-B multiples covering the heads");
  if (!p->pmax || !p->amax) return tt2_invalid(who, "pmax / amax required");
  for (int l = 0; l < p->n_layers; ++l)
    if (!p->q[l] || !p->k[l] || !p->lse[l]) return tt2_invalid(who, "q / k / lse of a layer missing");
  if (p->n_layers == 0 || p->batch == 0 || p->tq == 0) return TT2_OK;
  const int BH = p->batch * p->heads;
  // the forward's rule: four waves share each K tile while that still fills the chip
  const int nw = v3_waves(p->dtype, p->variant, p->tq, (int64_t)BH * p->n_layers, true);
  // the v3 kernel's buffer views address rows with 32-bit byte offsets
  if (nw && (((int64_t)p->tq * p->q_ld + D) * 2 > INT32_MAX || ((int64_t)p->tk * p->k_ld + D) * 2 > INT32_MAX))
    return tt2_invalid(who, "one batch element's q or k spans more than 2 GiB");
  if (!nw && BH > 65535) return tt2_invalid(who, "the plain kernel takes at most 65535 (batch, head) pairs");
  launch_align(p, nw, s);
  return tt2_check_launch(hipGetLastError(), who);
}

extern "C" int tt2_align_durations(const tt2_align_dur_args* p, hipStream_t s) {
  const char* who = "tt2_align_durations";
  if (!p) return tt2_invalid(who, "args required");
  if (!p->pmax || !p->amax || !p->focus || !p->sel || !p->sel_focus || !p->durations)
    return tt2_invalid(who, "missing buffer");
  if (p->n_layers <= 0 || p->n_layers > TT2_GUIDE_MAX_LAYERS) return tt2_invalid(who, "needs 1..16 layers");
  if (p->batch < 0 || p->heads <= 0 || p->tq < 0 || p->tk < 0 ||
      (int64_t)p->n_layers * p->heads > ALIGN_DUR_MAX_PAIRS)
    return tt2_invalid(who, "shape");
  if (p->mode != 0 && p->mode != 1) return tt2_invalid(who, "mode must be 0 (best head) or 1 (fixed head)");
  if (p->mode == 1 && (p->sel_layer < 0 || p->sel_layer >= p->n_layers || p->sel_head < 0 || p->sel_head >= p->heads))
    return tt2_invalid(who, "fixed head outside the layers / heads");
  if (p->batch == 0) return TT2_OK;
  launch_align_dur(p, s);
  return tt2_check_launch(hipGetLastError(), who);
}
