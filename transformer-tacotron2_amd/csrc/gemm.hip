// gemm.hip -- the GEMM's host side: request validation, the planner, the route from a request to
// the one kernel that runs it, and tt2_gemm.  The kernels live one family per unit
// (gemm_common.h has the map); this unit holds no device code.
//
//   C[m, n] = epi( alpha * sum_k A(m, k) * B(n, k) )
//
// A(m,k) is K-contiguous (A[m*lda + k]) or M-contiguous (A[k*lda + m]);
// likewise B(n,k).  That covers every product of the training step:
//   linear fwd   Y  = X  W^T      (A K-contig, B K-contig)
//   linear dgrad dX = dY W        (A K-contig, B N-contig)
//   linear wgrad dW = dY^T X      (A M-contig, B N-contig)
// and the Conv1d(k5) layers as implicit GEMMs: with channels-last activations
// x[(b*T + t)*C + c] and weights packed [Cout][tap][Cin], the im2col row of
// output frame (b,t) is the overlapping window x[(b*T+t-pad)*C ...], i.e. an
// operand with ld = C and a per-chunk validity test 0 <= t + tap - pad < T.
//
#include "gemm_common.h"

using tt2g::Epilogue;
using tt2g::Operand;

#ifndef TT2_G10_AUTO
#define TT2_G10_AUTO 1
#endif
#ifndef TT2_G11_AUTO   // the auto plan takes v11 where it would take v7 and v11 is eligible
#define TT2_G11_AUTO 1
#endif
#ifndef G11_MAX_K       // ... up to this K (one MFMA wave per SIMD loses to v7's two at long K:
#define G11_MAX_K 1024  // 12800 x 512 x 2048 30.3 -> 30.9 us; K = 512: -7 %)
#endif

extern "C" size_t tt2_gemm_workspace_size(const tt2_gemm_args* a) {
  if (a->splits <= 1) return 0;
  return (size_t)a->splits * a->m * (a->n + (a->a_ksum ? 1 : 0)) * sizeof(float);
}

// v7 epilogue form: 13 = straight from registers; auto (and 14) = through the LDS C image
// (-1.7 % step time)
static bool g7_lds_epi(int variant) { return variant != 13; }

// Kernel selection (also exported as tt2_gemm_plan): 1 v1 register-staged, 2 v2
// LDS-DMA 128^2, 3 skinny (M <= 64), 13 v7 warp-specialised 256x128 (auto; variant 14
// forces its LDS-image epilogue, 13 its register epilogue), 15 v8 64x64, 16 v10 256x256 NT.
// Returns -1 (error set) for an unsupported fusion request.
#ifndef G8_SPLIT_TO_V7
#define G8_SPLIT_TO_V7 1
#endif
#ifndef G8_AUTO_TILES   // auto plan: v8 when v7 would run at most this many tiles
#define G8_AUTO_TILES 64
#endif
#ifndef G8_SPLIT_MIN_K   // only the long-K ones (the encoder's K = 2048 products run faster unsplit on v8)
#define G8_SPLIT_MIN_K 4096
#endif
namespace tt2g {
int gemm_plan(const tt2_gemm_args* a) {
  const int var = a->kernel_variant;
  const int64_t a_inner = a->trans_a ? a->m : a->k, b_inner = a->trans_b ? a->n : a->k;
  // skinny split-K exists only as raw partial slabs (main_only) for tt2_ln_combine
  const bool half_in = a->dtype_in == TT2_BF16 || a->dtype_in == TT2_F16;
  const bool skinny = half_in && a->m <= 64 && !a->trans_a && !a->trans_b && a->k % 8 == 0 &&
                      a->a_conv_t == 0 && (a->splits <= 1 || a->main_only) && (var == 0 || var == 3);
  if (skinny && a->splits > 1 && (a->a_ln_gamma || a->kv_cache || a->pe_table || a->emit_mel ||
                                  a->k % (32 * a->splits) != 0))
    return tt2_set_error(TT2_E_INVALID, "tt2_gemm: skinny split-K slabs need k % (32 splits) == 0, no fusions"), -1;
  if ((a->a_ln_gamma || a->kv_cache) && !skinny)
    return tt2_set_error(TT2_E_INVALID, "tt2_gemm: a_ln / kv fusions need the skinny path (bf16, m <= 64, NT)"), -1;
  if (a->dtype_in == TT2_F16 && !skinny)
    return tt2_set_error(TT2_E_INVALID, "tt2_gemm: f16 operands only on the skinny decode path (m <= 64, NT)"), -1;
  if (a->a_ln_gamma && (a->dtype_in != TT2_BF16 || a->k != 512 || a->lda != a->k || a->m > 32 || !a->a_ln_branch ||
                        !a->a_ln_beta ||
                        !a->a_ln_out))
    return tt2_set_error(TT2_E_INVALID, "tt2_gemm: a_ln needs k == lda == 512, m <= 32, branch, beta and out"), -1;
  if (a->kv_cache && (!a->kv_t || a->dtype_out != a->dtype_in))
    return tt2_set_error(TT2_E_INVALID, "tt2_gemm: kv scatter needs kv_t and an output of the input dtype"), -1;
  if ((a->pe_table || a->emit_mel) && !skinny)
    return tt2_set_error(TT2_E_INVALID, "tt2_gemm: pe / emit epilogues need the skinny path (bf16, m <= 64, NT)"), -1;
  if (a->pe_table && (!a->pe_alpha || !a->pe_t))
    return tt2_set_error(TT2_E_INVALID, "tt2_gemm: pe epilogue needs pe_alpha and pe_t"), -1;
  if (a->emit_mel && (!a->emit_stop || !a->emit_prev || !a->emit_t || !a->emit_done || a->emit_nmels >= a->n ||
                      a->emit_nmels <= 0 || a->emit_tmax <= 0))
    return tt2_set_error(TT2_E_INVALID, "tt2_gemm: emit epilogue needs stop/prev/t/done and n > emit_nmels"), -1;
  if (skinny) return 3;
  // LDS-DMA kernels: bf16, every 16-B chunk either fully inside or fully outside its row
  const bool v2 = a->dtype_in == TT2_BF16 && var != 1 && a_inner % 8 == 0 && b_inner % 8 == 0;
  if (a->a_ksum && !(v2 && a->trans_a && a->a_conv_t == 0))
    return tt2_set_error(TT2_E_INVALID, "tt2_gemm: a_ksum needs bf16, trans_a, no conv A, the LDS-DMA kernel"), -1;
  if (!v2) return 1;
  // The 256-row-tile kernel needs per-lane byte offsets that fit 32 bits.  Auto = v7, the
  // warp-specialised 256 x 128 kernel (fastest on every GEMM of the training step:
  // 1.2-1.6x v2; a 256 x 256 / 256 x 128 kernel whose 8 waves both load and multiply was
  // measured slower on every step shape and removed).
  // v7 also takes implicit-im2col operands (its loaders track tap / time per copy)
  // when every conv has C >= 64 and T >= 64 (one wrap per 64-deep K step)
  auto conv_ok = [](int t, int c) { return t == 0 || (t >= 64 && c >= 64); };
  const bool v7ok = conv_ok(a->a_conv_t, a->a_conv_c) && conv_ok(a->b_conv_t, a->b_conv_c) &&
                    (int64_t)(a->trans_a ? a->k : a->m) * a->lda * 2 < (1LL << 31) &&
                    (int64_t)(a->trans_b ? a->k : a->n) * a->ldb * 2 < (1LL << 31);
  // v8 (64 x 64 tiles): K-contiguous A (conv allowed), no k-sums, bf16 C; forced by variant 15
  // (v8 never writes split-K slabs: a request for raw partial slabs stays on v7)
  const bool v8ok = !a->trans_a && !a->a_ksum && a->b_conv_t == 0 && a->dtype_out == TT2_BF16 && a->n % 8 == 0 &&
                    !(a->splits > 1 && a->main_only) &&
                    (int64_t)a->m * a->lda * 2 < (1LL << 31) &&
                    (int64_t)(a->trans_b ? a->k : a->n) * a->ldb * 2 < (1LL << 31);
  // auto: v8 when v7 would run at most 64 tiles (the encoder's 2048-row products with N = 512,
  // the post-net's 80-channel conv): 1.4-1.6x v7 there, slower once v7 has >= 96 tiles
  // (a long-K split-K request goes to v7, which splits: v8 has no split-K and ran it unsplit —
  // the encoder's memory K/V dgrad, 2048 x 512 x 6144: 70 us unsplit on 256 64x64 tiles)
  const int64_t tiles7 = (int64_t)((a->m + 255) / 256) * ((a->n + 127) / 128);
  const bool split_v7 = G8_SPLIT_TO_V7 && a->splits > 1 && v7ok && a->k >= G8_SPLIT_MIN_K;
  if (v8ok && a->m >= 64 && (var == 15 || (var == 0 && tiles7 <= G8_AUTO_TILES && !split_v7))) return 15;
  // v10 (256 x 256, NT, bf16 C, K % 64 == 0, N % 256 == 0, no split / conv / k-sums; its epilogue
  // options are checked at launch): forced by variant 16; auto for the wide products
  const bool v10ok = v7ok && !a->trans_a && !a->trans_b && a->a_conv_t == 0 && !a->a_ksum &&
                     a->dtype_out == TT2_BF16 && a->splits <= 1 && a->n % 256 == 0 && a->k % 64 == 0 &&
                     !a->res && !a->gate && a->beta == 0.f && a->act != ACT_TANH &&
                     reinterpret_cast<uintptr_t>(a->c) % 16 == 0 && a->ldc % 8 == 0 &&
                     reinterpret_cast<uintptr_t>(a->bias) % 16 == 0;
  // auto: when its rounds of the chip (one tile per CU) take less time than v7's, a v10 tile
  // costing ~1.7 v7 tiles (in-step work-group spans, tools/gemm_wgt.py): the decoder FFN1
  // forward (2 vs 4 rounds), the memory K/V projection (1 vs 2), large squares; not QKV (2 vs 3)
  const int64_t cus = tt2_cu_count();
  const int64_t rounds7 = (tiles7 + cus - 1) / cus, rounds10 = ((a->m + 255) / 256 * (a->n / 256) + cus - 1) / cus;
  if (v10ok && (var == 16 || (var == 0 && TT2_G10_AUTO && 17 * rounds10 < 10 * rounds7))) return 16;
  // v11 (v7's tile, 4 MFMA + 8 loader waves; NT, bf16 C, K % 64 == 0, N % 128 == 0, bias / ReLU /
  // dropout epilogues only, checked at launch): forced by variant 17; auto where v7 would run
  const bool v11ok = v7ok && !a->trans_a && a->a_conv_t == 0 && a->b_conv_t == 0 && !a->a_ksum &&
                     a->dtype_out == TT2_BF16 && a->splits <= 1 && a->n % 128 == 0 && a->k % 64 == 0 &&
                     a->beta == 0.f && a->act != ACT_TANH && !a->col_stats && !a->bn_bwd &&
                     (a->trans_b ? !a->bias && !a->act && !a->drop_thr && !(a->res && a->gate)
                                 : !a->res && !a->gate) &&
                     reinterpret_cast<uintptr_t>(a->c) % 16 == 0 && a->ldc % 8 == 0 &&
                     reinterpret_cast<uintptr_t>(a->bias) % 16 == 0;
  // (auto: the forward's NT products only; on the activation gradients, with the residual / gate
  // tile staged, v11 measured 3-5 % slower than v7 and the step 1 % slower: profiles/r06_v11_ab.txt)
  if (v11ok && (var == 17 || (var == 0 && TT2_G11_AUTO && a->k <= G11_MAX_K && !a->trans_b))) return 17;
  if ((var == 13 || var == 14 || var == 0) && v7ok) return 13;
  return 2;
}
}  // namespace tt2g

extern "C" int tt2_gemm_plan(const tt2_gemm_args* a) { return tt2g::gemm_plan(a); }

// Vectorised epilogue: rows of C / res / gate start 16-B aligned at every 8th column.
static bool epi_vec_ok(const tt2_gemm_args* a) {
  auto ok = [](const void* p, int64_t ld, int dt) {
    if (!p) return true;
    const int esz = dt == TT2_BF16 ? 2 : 4;
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (ld * esz) % 16 == 0 && (8 * esz) % 16 == 0;
  };
  return a->dtype_out != TT2_F16 && a->res_dtype != TT2_F16 && a->gate_dtype != TT2_F16 &&
         ok(a->c, a->ldc, a->dtype_out) && ok(a->res, a->ldr, a->res_dtype) && ok(a->gate, a->ldg, a->gate_dtype) &&
         (reinterpret_cast<uintptr_t>(a->bias) % 16 == 0);
}

// The route of a request: the kernel that launches (a gemm_plan code; -1: error set), for v10 /
// v11 its epilogue code, and for a fused-statistics request (col_stats / bn_bwd) the chunk height
// that kernel writes (0: no kernel of the route can carry the statistics).  It starts from the
// planner's choice and applies what the planner leaves to the launch:
//  - v8 stores C and reads res / gate in 16-B chunks: rows that are not vector-aligned take the
//    forced-v7 plan (v7, or v2);
//  - fused statistics run on v8 (64-row chunks) when the plan takes it, else on v7's LDS-image
//    epilogue (256-row chunks: NT, n % 128 == 0, not variant 13); neither can with split-K, f32 C
//    or unaligned rows;
//  - an option set v10 / v11 do not fuse takes the forced-v7 plan.  (v10's plan condition implies
//    every term of g10_code but one: epi_vec_ok also refuses an f16 res_dtype / gate_dtype on a
//    null res / gate, so that fallback stays.)
// tt2_gemm switches on the result; tt2_gemm_stats_rows answers from the same call.
struct Route { int kernel, code, stats_rows; };

static int replan(const tt2_gemm_args* a, int variant) {
  tt2_gemm_args b = *a;
  b.kernel_variant = variant;
  return tt2g::gemm_plan(&b);
}

static Route gemm_route(const tt2_gemm_args* a, bool stats) {
  Route r{tt2g::gemm_plan(a), 0, 0};
  if (r.kernel < 0) return r;
  const bool vec = epi_vec_ok(a);
  if (r.kernel == 15 && !vec) r.kernel = replan(a, 13);
  if (stats) {
    auto al = [](const void* p, int64_t ld) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (ld * 2) % 16 == 0; };
    bool ok = a->splits <= 1 && a->dtype_out == TT2_BF16 && al(a->c, a->ldc) && a->n % 8 == 0 &&
              (reinterpret_cast<uintptr_t>(a->col_stats) & 3) == 0;
    if (ok && r.kernel != 15) {
      // (a forced-v7 plan that fails leaves the planner's kernel: the caller reports that the
      // statistics cannot be carried, not the re-plan's own error)
      ok = (r.kernel == 13 || replan(a, 14) == 13) && !a->trans_a && !a->trans_b &&
           g7_lds_epi(a->kernel_variant) && a->n % 128 == 0;
      if (ok) r.kernel = 13;
    }
    r.stats_rows = !ok ? 0 : r.kernel == 15 ? 64 : 256;
    return r;
  }
  if (r.kernel == 16 && (r.code = tt2g::g10_code(a, vec)) < 0) r.kernel = replan(a, 13);
  if (r.kernel == 17 && (r.code = tt2g::g11_code(a, vec)) < 0) r.kernel = replan(a, 13);
  return r;
}

extern "C" int32_t tt2_gemm_stats_rows(const tt2_gemm_args* a) { return gemm_route(a, true).stats_rows; }

// Validate one GEMM request and build its operand / epilogue descriptors.
int tt2g::gemm_prep(const tt2_gemm_args* a, Operand& A, Operand& B, Epilogue& ep) {
  const int esz = a->dtype_in == TT2_F32 ? 4 : 2;
  const int E = 16 / esz;
  auto misaligned = [&](const void* p, int64_t ld) {
    return (reinterpret_cast<uintptr_t>(p) % 16) != 0 || (ld * esz) % 16 != 0;
  };
  if (!a->a || !a->b || !a->c) return tt2_set_error(TT2_E_INVALID, "tt2_gemm: null operand");
  if (misaligned(a->a, a->lda) || misaligned(a->b, a->ldb))
    return tt2_set_error(TT2_E_INVALID, "tt2_gemm: operands must be 16-B aligned with 16-B multiple leading dims");
  if (a->a_conv_t > 0 && (a->trans_a || a->a_conv_c % E != 0 || a->lda != a->a_conv_c))
    return tt2_set_error(TT2_E_INVALID, "tt2_gemm: conv A needs K-contiguous A, lda == C, C % chunk == 0");
  if (a->b_conv_t > 0 && (!a->trans_b || a->b_conv_c % E != 0 || a->ldb != a->b_conv_c))
    return tt2_set_error(TT2_E_INVALID, "tt2_gemm: conv B needs N-contiguous B, ldb == C, C % chunk == 0");
  if (a->splits > 1 && (!a->workspace || a->ws_bytes < tt2_gemm_workspace_size(a)))
    return tt2_set_error(TT2_E_INVALID, "tt2_gemm: split-K workspace too small");

  A = Operand{a->a, a->lda, 0, 0, a->a_conv_t, a->a_conv_c, a->a_conv_pad};
  B = Operand{a->b, a->ldb, 0, 0, a->b_conv_t, a->b_conv_c, a->b_conv_pad};
  if (!a->trans_a) { A.outer_max = a->m; A.inner_max = a->k; } else { A.outer_max = a->k; A.inner_max = a->m; }
  if (!a->trans_b) { B.outer_max = a->n; B.inner_max = a->k; } else { B.outer_max = a->k; B.inner_max = a->n; }
  if (a->k <= 0) return tt2_set_error(TT2_E_INVALID, "tt2_gemm: k must be > 0");

  ep = Epilogue{};
  ep.c = a->c; ep.ldc = a->ldc; ep.c_dt = a->dtype_out;
  ep.bias = a->bias;
  ep.res = a->res; ep.ldr = a->ldr; ep.res_dt = a->res_dtype;
  ep.gate = a->gate; ep.ldg = a->ldg; ep.gate_dt = a->gate_dtype; ep.gate_scale = a->gate_scale;
  ep.alpha = a->alpha; ep.beta = a->beta; ep.act = a->act;
  ep.drop = drop_of(a);
  if (ep.drop.thr && !ep.drop.seed) return tt2_set_error(TT2_E_INVALID, "tt2_gemm: dropout without seed");
  ep.n_log = a->n;
  ep.ksum = a->a_ksum;
  ep.ksum_beta = a->a_ksum_beta;
  ep.main_only = a->main_only;
  ep.cstats = a->col_stats;
  if (const tt2_bn_args* bn = a->bn_bwd) {
    if (bn->dtype != TT2_DT_BF16 || bn->c != a->n || bn->m != a->m || !bn->y || !bn->mean || !bn->rstd ||
        !bn->gamma || !bn->beta || !bn->workspace || a->col_stats || (bn->drop_thr && !bn->drop_seed))
      return tt2_set_error(TT2_E_INVALID, "tt2_gemm: bn_bwd needs a bf16 BatchNorm of this GEMM's m x n, its "
                                          "y / mean / rstd / gamma / beta, a chunk-sums workspace, no col_stats");
    ep.bnb.y = reinterpret_cast<const bf16*>(bn->y);
    ep.bnb.mean = bn->mean; ep.bnb.rstd = bn->rstd; ep.bnb.gamma = bn->gamma; ep.bnb.beta = bn->beta;
    ep.bnb.part = reinterpret_cast<float*>(bn->workspace);
    ep.bnb.drop = drop_of(bn);
    ep.bnb.act = bn->act;
  }
  ep.vec = epi_vec_ok(a);
  return TT2_OK;
}

extern "C" int tt2_gemm(const tt2_gemm_args* a, hipStream_t stream) {
  ProbeDisarm disarm;
  if (a->m <= 0 || a->n <= 0) return TT2_OK;
  Operand A, B;
  Epilogue ep;
  if (const int rc = tt2g::gemm_prep(a, A, B, ep); rc != TT2_OK) return rc;
  float* ws = reinterpret_cast<float*>(a->workspace);
  const int sp = a->splits > 1 ? a->splits : 1;
  const bool stats = ep.cstats || ep.bnb.part;   // fused BatchNorm statistics: v8's or v7's image epilogue
  const Route r = gemm_route(a, stats);
  if (r.kernel < 0) return TT2_E_INVALID;   // message already set
  if (stats) {
    if (!r.stats_rows)
      return tt2_set_error(TT2_E_INVALID, "tt2_gemm: col_stats / bn_bwd need the v8 path or v7's LDS-image path "
                                          "(bf16 C, 16-B aligned rows, no split-K; v7: NT and n % 128 == 0)");
    const int rp = r.stats_rows;
    if (a->bn_bwd && a->bn_bwd->ws_bytes < (size_t)((a->m + rp - 1) / rp) * 2 * a->n * sizeof(float))
      return tt2_set_error(TT2_E_INVALID, "tt2_gemm: bn_bwd workspace smaller than its chunk sums");
  }
  const bool a_kc = !a->trans_a, b_kc = !a->trans_b;
  const int m = a->m, n = a->n, k = a->k;
  switch (r.kernel) {
    case 3:   // skinny-M weight-streaming path (decode step)
      return tt2_check_launch(tt2g::launch_skinny(a, ep, stream), "tt2_gemm(skinny)");
    case 16:
      return tt2_check_launch(tt2g::launch10(A, B, ep, m, n, k, r.code, stream), "tt2_gemm(v10)");
    case 17:
      return tt2_check_launch(tt2g::launch11(A, B, ep, m, n, k, b_kc, r.code, stream), "tt2_gemm(v11)");
    case 15:
      return tt2_check_launch(tt2g::launch8(b_kc, A, B, ep, m, n, k, stream), "tt2_gemm(v8)");
    case 13:
      return tt2_check_launch(tt2g::launch7(a_kc, b_kc, A, B, ep, m, n, k, sp, ws, stream,
                                            g7_lds_epi(a->kernel_variant)), "tt2_gemm(v7)");
    case 2:
      return tt2_check_launch(tt2g::launch2(a_kc, b_kc, A, B, ep, m, n, k, sp, ws, stream), "tt2_gemm");
    default:
      return tt2_check_launch(tt2g::launch1(a->dtype_in == TT2_BF16, a_kc, b_kc, A, B, ep, m, n, k, sp, ws, stream),
                              "tt2_gemm");
  }
}
