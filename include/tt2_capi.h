/* tt2_capi.h -- C ABI of libtt2.so, the MI355X (gfx950) kernel library behind the
 * Transformer-TTS mel path (encoder -> decoder -> post-net).
 *
 * The reference (keonlee9420/Transformer-tacotron2, /root/reference/README.md:1-3)
 * ships no code, so it has no FFI to mirror; this ABI is the boundary SURVEY.md
 * section 8(b) defines: one entry point per fused block of the path, plain
 * pointers and sizes, no torch types.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - Every device buffer (inputs, outputs, workspace) is allocated by the caller;
 *    nothing allocates on the hot path, so every call is hipGraph-capturable.
 *  - Calls are stream-ordered on the caller's stream and reentrant.
 *  - Return 0 (TT2_OK) or a negative TT2_E_* code; tt2_last_error() returns a
 *    thread-local message for the last failure on this thread.
 *  - dtype fields: TT2_DT_F32 = 0, TT2_DT_BF16 = 1, TT2_DT_F16 = 2 (decode step only).  Activations are
 *    channels-last row-major [rows, channels]; rows = batch * time.
 *  - Dropout: keep(idx) = hash(seed, site, idx) >= thr; thr = 0
 *    disables it.  seed points to a device uint32.
 */
#ifndef TT2_CAPI_H
#define TT2_CAPI_H
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TT2_OK 0
#define TT2_E_INVALID -1
#define TT2_E_LAUNCH -2
#define TT2_E_HIP -3

#define TT2_DT_F32 0
#define TT2_DT_BF16 1
#define TT2_DT_F16 2   /* decode step only: skinny GEMM, decode attention, ln_combine, cast2d */

/* ------------------------------------------------------------------ runtime */
const char* tt2_last_error(void);
int tt2_version(void);
int tt2_init(int device);

/* --------------------------------------------------------------------- GEMM
 * C[m,n] = epi(alpha * sum_k A(m,k) B(n,k)), epi = (+bias[n]) (+res[m,n]) (act)
 *          (*gate: res==0 ? 0 : gate_scale) (dropout) (+beta*C[m,n]).
 * trans_a = 0: A(m,k) = a[m*lda + k]; 1: a[k*lda + m].  trans_b likewise for B(n,k).
 * a_conv_t > 0: A is the implicit im2col of a channels-last sequence batch
 *   (time = m % a_conv_t, tap = k / a_conv_c, zero outside [0, T)); b_conv_* the
 *   same for an N-contiguous B (wgrad of a conv).
 * splits > 1: split-K with an f32 workspace of tt2_gemm_workspace_size() bytes.
 * Replaces the nn.Linear / nn.Conv1d products of SURVEY 8(a) rows a1, a3-a9, a11. */
typedef struct tt2_gemm_args {
  const void* a; const void* b; void* c;
  const float* bias;
  const void* res; const void* gate;
  const uint32_t* drop_seed;
  void* workspace; size_t ws_bytes;
  int64_t lda, ldb, ldc, ldr, ldg;
  int32_t m, n, k;
  int32_t dtype_in, dtype_out, res_dtype, gate_dtype;
  int32_t trans_a, trans_b;
  int32_t act;          /* 0 none, 1 relu, 2 tanh */
  int32_t splits;
  float alpha, beta, gate_scale;
  uint32_t drop_site, drop_thr;
  float drop_scale;
  int32_t a_conv_t, a_conv_c, a_conv_pad;
  int32_t b_conv_t, b_conv_c, b_conv_pad;
  int32_t kernel_variant;  /* 0 auto, 1 register-staged (any shape), 2 LDS-DMA 128x128 (bf16, 8-aligned inner
                              dims), 13 / 14 warp-specialised 256x128 (same, conv C, T >= 64; the auto choice
                              when eligible) with its register / LDS-image epilogue (auto: LDS image),
                              15 64x64 (K-contiguous A; auto for <= 64 v7 tiles), 16 256x256 (NT, bf16 C,
                              N % 256 == 0, K % 64 == 0, bias / ReLU / dropout epilogues only; auto when
                              its rounds of the chip cost less than v7's), 17 256x128 with 8 loader waves
                              (NT, bf16 C, N % 128 == 0, K % 64 == 0, the same epilogues; auto where v7 would
                              run) */
  /* optional fused row sums of op(A) over k: a_ksum[m] = a_ksum_beta * a_ksum[m] + sum_k A(m, k)
   * (f32).  With A = dY^T of a weight-gradient GEMM this is the bias gradient, taken from the
   * A tiles already staged in LDS.  Requires bf16, trans_a, no conv on A. */
  float* a_ksum;
  float a_ksum_beta;
  /* decode-step fusions, skinny path only (bf16, m <= 64 (LN prologue m <= 32), A and B K-contiguous):
   * - LayerNorm prologue on A: when a_ln_gamma != NULL the GEMM multiplies
   *   h = LN(A + a_ln_branch) (row-wise over the k = 512 columns, eps a_ln_eps) instead of A,
   *   and writes h to a_ln_out [m, k] (ld k);
   * - KV-cache scatter epilogue: when kv_cache != NULL, output columns n >= kv_col0 are also
   *   stored to kv_cache[m * kv_bstride + (*kv_t) * kv_ld + (n - kv_col0)] (dtype_in); a step
   *   past the cache ((*kv_t) * kv_ld >= kv_bstride) stores nothing there. */
  const void* a_ln_branch;
  const float* a_ln_gamma;
  const float* a_ln_beta;
  void* a_ln_out;
  float a_ln_eps;
  void* kv_cache;
  const int32_t* kv_t;
  int32_t kv_col0;
  int64_t kv_bstride, kv_ld;
  /* measurement hook: with splits > 1, launch only the main kernel (partials stay in
   * the workspace, C is not written), so a per-kernel timing excludes the reduce */
  int32_t main_only;
  /* more decode-step epilogues, skinny path only:
   * - scaled positional encoding: when pe_table != NULL, out[m, n] += (*pe_alpha) *
   *   pe_table[(*pe_t) * n_cols + n] after the rest of the epilogue (f32 table [T][n]);
   * - frame emit (the mel/stop heads GEMM): when emit_mel != NULL, with t = *emit_t < emit_tmax,
   *   columns n < emit_nmels also go to emit_mel[(m * emit_tmax + t) * emit_nmels + n] (f32) and
   *   emit_prev[m * emit_nmels + n] (dtype_in, the next step's pre-net input), column emit_nmels to
   *   emit_stop[m * emit_tmax + t]; the last workgroup to finish then sets *emit_t = t + 1,
   *   *emit_seed += 1 (if non-NULL) and re-zeroes *emit_done (a device int the caller zeroes
   *   once).  Replaces the tt2_decode_emit launch. */
  const float* pe_table;
  const float* pe_alpha;
  const int32_t* pe_t;
  float* emit_mel;
  float* emit_stop;
  void* emit_prev;
  int32_t* emit_t;
  uint32_t* emit_seed;
  int32_t* emit_done;
  int32_t emit_nmels, emit_tmax;
  /* frame emit, stop handling: emit_stop_bias (optional f32 [m][emit_tmax]) is added to the stop
   * logit before it is stored (per-utterance length injection); emit_stop_len (optional int32 [m])
   * records t + 1 at the first frame whose stop logit >= emit_stop_thr (entries the caller set to
   * INT32_MAX mean "still running"). */
  const float* emit_stop_bias;
  int32_t* emit_stop_len;
  float emit_stop_thr;
  /* fused BatchNorm statistics: when col_stats != NULL, each 256-row chunk r of the stored
   * (bf16) output C also leaves its column moments, col_stats[(2 r) * n + j] = mean and
   * col_stats[(2 r + 1) * n + j] = sum over the chunk's rows of (C - mean)^2 (rows < m only),
   * in the chunk layout tt2_batchnorm_fwd reads with stats_rows = the chunk's rows.  A chunk is the
   * kernel's tile height, tt2_gemm_stats_rows(): 64 rows on the 64 x 64 kernel (plan 15), else 256
   * on the 256 x 128 LDS-image path (bf16 C, A and B K-contiguous, n % 128 == 0); bf16 C, 16-B
   * aligned rows and no split-K either way.  Other requests fail with TT2_E_INVALID. */
  float* col_stats;
  /* fused BatchNorm backward sums: when bn_bwd != NULL, C is that BatchNorm's dout (the gradient
   * of its output: bn_bwd->y is its input, mean / rstd / gamma / beta / act / dropout as for
   * tt2_batchnorm_bwd, c == n, m == m), and each 256-row chunk r of the stored (bf16) C leaves the
   * column sums of dpre = dout * keep * act'(z) and of dpre * xhat in bn_bwd->workspace
   * ([r][2][n], the layout tt2_batchnorm_bwd reads with stats_rows = tt2_gemm_stats_rows()).  The
   * tt2_bn_args struct is read during the call only.  Same path restrictions as col_stats. */
  const struct tt2_bn_args* bn_bwd;
} tt2_gemm_args;
#define TT2_GEMM_STATS_ROWS 256   /* the 256 x 128 kernel's chunk (tt2_gemm_stats_rows) */

size_t tt2_gemm_workspace_size(const tt2_gemm_args* a);
/* Rows per chunk of a col_stats / bn_bwd request's statistics (the kernel's tile height): 64 on
 * the 64 x 64 kernel, 256 on the 256 x 128 one, 0 when the request cannot fuse them.  Host-only. */
int32_t tt2_gemm_stats_rows(const tt2_gemm_args* a);
int tt2_gemm(const tt2_gemm_args* a, hipStream_t stream);
/* Kernel tt2_gemm would launch for these args (no device work): 1 register-staged
 * 128x128 (any dtype), 2 LDS-DMA 128x128 (bf16), 3 skinny decode (m <= 64),
 * 13 warp-specialised 256x128, 15 64x64; -1 invalid. */
int tt2_gemm_plan(const tt2_gemm_args* a);

/* Grouped GEMM: up to 8 independent problems in ONE launch of the v7 kernel (every
 * problem must be v7-eligible -- tt2_gemm_plan(p) == 13 -- and share trans_a/trans_b;
 * each problem's own splits / workspace; one grouped split-K reduce follows).  Used for
 * the weight gradients of a layer, which share K = tokens.  Replaces the per-linear
 * weight-gradient calls of the reference's autograd backward (see tt2_gemm). */
int tt2_gemm_grouped(const tt2_gemm_args* probs, int32_t n, hipStream_t stream);

/* Measurement probe (bench.py's live roofline): tt2_probe_arm() makes the next main GEMM
 * kernel (v7 / grouped v7 / v8 / LDS-DMA 128x128) launched on this thread by the NEXT
 * tt2_gemm / tt2_gemm_grouped call record its timing and returns the slot.  Eager: start /
 * stop events ride in the kernel's own dispatch (its execution, as rocprofv3 reports it),
 * read by tt2_probe_ms (-1 if no probe-capable kernel consumed the slot, or under capture).
 * Eager and under stream capture alike, v7 / v8 kernels also record their own span on the
 * device wall clock (tt2_probe_span_ms); nothing is added to a captured graph, so each
 * replay of it re-times the launch inside the replayed step.  Any path of that call
 * disarms the probe; tt2_probe_reset() frees every slot. */
int tt2_probe_arm(void);
float tt2_probe_ms(int slot);
/* The same launch's span as the kernel records it on the device wall clock (first workgroup
 * start to last wave end, no stream event around it): ms, -1 if unavailable.  Reading
 * re-arms the slot's record, so a graph replayed again records afresh. */
float tt2_probe_span_ms(int slot);
/* The raw span record of a slot (measurement tools): per work group {start, end} on the device
 * wall clock (hipDeviceAttributeWallClockRate kHz), copied to out[2 * groups]; returns the
 * number of work groups, -groups - 1 if cap is too small, -1 if the slot has no record.  Read
 * it before tt2_probe_span_ms, which clears the record. */
int tt2_probe_span_records(int slot, unsigned long long* out, int cap);
/* u64 slots per work group in tt2_probe_span_records' output: 2 ({start, end}); 32 in the
 * in-step GEMM phase build (-DTT2_PHASE=1, tools/g7_phases.py: s_memtime stamps of the K
 * steps and the epilogue after the pair). */
int tt2_probe_span_width(void);
void tt2_probe_reset(void);

/* ---------------------------------------------------------------- attention
 * Scaled dot-product attention over heads of width 64, read in place from
 * projection outputs: head h of row (b, t) of Q is q[(b*tq + t)*q_ld + 64h].
 * Key j of batch b is visible iff j < key_len[b] (key_len may be NULL) and,
 * if causal, j <= t.  A row with no visible key outputs 0.
 * lse: [batch*heads, tq] f32, log2-domain log-sum-exp of scale*log2(e)*QK^T
 * (+inf for empty rows); written by fwd, read by bwd.
 * bwd: delta [batch*heads, tq] f32 scratch; dq/dk/dv may alias column slices
 * of one fused gradient buffer.  Replaces SURVEY 8(a) a3, a6, a7 (+ a11). */
typedef struct tt2_attn_args {
  const void* q; const void* k; const void* v;
  const void* o;      /* bwd: forward output */
  const void* dout;   /* bwd: gradient of the output */
  void* o_out;        /* fwd: output */
  void* dq; void* dk; void* dv;
  float* lse; float* delta;
  int64_t q_ld, k_ld, v_ld, o_ld, do_ld, dq_ld, dk_ld, dv_ld;
  const int32_t* key_len;
  int32_t batch, heads, head_dim, tq, tk, causal, dtype;
  float scale;
  int32_t variant;   /* 0 auto (bf16: v3 32x32 swapped MFMA products; f32: v1), 1 v1 (P through LDS),
                        2 v3 with 2-wave workgroups, 3 v3 with 4-wave workgroups (bf16 only) */
  int32_t parts;     /* bwd: 0 dQ and dK / dV, 1 dQ only, 2 dK / dV only (the non-causal bf16 launch,
                        whose two halves share no state: two streams may run them side by side) */
} tt2_attn_args;

/* Alignment diagnostics: probs[b*H + h][q][j] (f32) of a forward already run with these
 * args, recomputed from q, k and the saved lse (exactly 0 where masked). */
int tt2_attn_probs(const tt2_attn_args* a, float* probs, hipStream_t stream);
int tt2_attn_fwd(const tt2_attn_args* a, hipStream_t stream);
int tt2_attn_bwd(const tt2_attn_args* a, hipStream_t stream);

/* Guided attention (diagonal loss on encoder-decoder attention, SpeechT5 / ESPnet convention),
 * folded into the non-causal forward and backward.  For utterance b with Tx = min(tk,
 * key_len[b]) visible keys and Ty = min(tq, q_len[b]) valid query rows,
 *   W[n, t] = 1 - exp(-(t / Tx - n / Ty)^2 / (2 sigma^2)),
 * the forward also stores g[n] = sum_t P[n, t] W[n, t] into rows ([batch*heads, tq] f32; exactly 0
 * for heads >= `heads`, rows n >= Ty and rows with no visible key), and the backward differentiates
 * out + kappa * sum g:  dS = P (dP + kappa W - (delta + kappa g))  on those heads and rows, with
 * kappa read from device memory (coef; tt2_guided_attn_loss writes it).  o_out and lse of the guided
 * forward equal tt2_attn_fwd's bit for bit; the guided backward leaves delta + kappa g in the delta
 * scratch (kappa g counted on the guided heads' valid rows only; parts = 2 alone runs no dQ block
 * and leaves the scratch untouched).  Same variants and parts as the plain calls.
 * Refused (TT2_E_INVALID, nothing is launched or written): a NULL guide; causal != 0; rows NULL;
 * coef NULL in the backward; sigma <= 0 or NaN; heads < 0 or heads > the attention's heads. */
typedef struct tt2_attn_guide {
  const int32_t* q_len;   /* [batch] valid query rows (may be NULL: tq) */
  float* rows;            /* g, [batch*heads, tq] f32: written by fwd, read by bwd */
  const float* coef;      /* device kappa (bwd only) */
  float sigma;
  int32_t heads;          /* heads h < heads are guided (0 <= heads <= the attention's heads) */
} tt2_attn_guide;
int tt2_attn_fwd_guided(const tt2_attn_args* a, const tt2_attn_guide* g, hipStream_t stream);
int tt2_attn_bwd_guided(const tt2_attn_args* a, const tt2_attn_guide* g, hipStream_t stream);

/* The guided-attention term of a step, one fixed-order reduction launch (no atomics):
 *   N     = n_layers * guide_heads * sum_b Tx_b * Ty_b   (from the device lengths)
 *   term  = scale * (sum of rows[l] over the guided heads) / N     (0 if N = 0)
 *   coef  = scale * grad_scale / N   (kappa for tt2_attn_bwd_guided; 0 if N = 0)
 *   loss_out[0] += term              (loss_out may be NULL; untouched if N = 0)
 * Lengths are cut to [0, tk] / [0, tq].  Each rows[l] holds whole [batch*heads, tq] rows and the
 * guided heads' rows are summed whole (the forward leaves exactly 0 past Ty_b), the other heads'
 * rows are not read.
 * Refused (TT2_E_INVALID, nothing is launched or written): NULL args, term or coef; n_layers < 0 or
 * n_layers > TT2_GUIDE_MAX_LAYERS; batch, tq or tk < 0; heads <= 0; guide_heads < 0 or guide_heads >
 * heads; heads * tq above INT32_MAX; a NULL rows[l] with l < n_layers. */
#define TT2_GUIDE_MAX_LAYERS 16
typedef struct tt2_guide_loss_args {
  const float* rows[TT2_GUIDE_MAX_LAYERS];   /* the guided layers' g buffers, [batch*heads, tq] f32 each */
  const int32_t* key_len; const int32_t* q_len;   /* [batch], device (NULL: tk / tq) */
  float* loss_out; float* term; float* coef;
  int32_t n_layers, batch, heads, guide_heads, tq, tk;
  float scale;
  float grad_scale;   /* multiplies kappa (1/world_size under data parallelism) */
} tt2_guide_loss_args;
int tt2_guided_attn_loss(const tt2_guide_loss_args* a, hipStream_t stream);

/* Alignment statistics of forwards already run (encoder-decoder attention; no attention matrix is
 * stored): one launch for n_layers layers, each with its own q, k and saved log2-LSE (the k of
 * layer l is usually a column slice of one wide buffer, row stride k_ld).  For layer slot i,
 * (b, h) and query row n:
 *   pmax[i][b*heads + h][n] = max_t P[n, t] = exp2(s_max * scale * log2(e) - lse[n])   (f32)
 *   amax[i][b*heads + h][n] = the key index of that maximum, the LOWEST index on exact ties (int32)
 * Keys t >= key_len[b] are masked as in tt2_attn_fwd.  Rows n >= q_len[b] and rows whose LSE is
 * +inf (no visible key) give pmax = 0 exactly and amax = -1.  key_len and q_len may be NULL (tk /
 * tq).  Non-causal only: causal != 0 is refused (TT2_E_INVALID), as are scale <= 0 and
 * n_layers > TT2_GUIDE_MAX_LAYERS.  variant as in tt2_attn_args: 0 auto (bf16: the MFMA kernel,
 * whose scores are formed exactly as the v3 forward forms them; f32: the plain kernel), 1 the
 * plain kernel (one work group per row), 2 / 3 the MFMA kernel with 2 / 4 waves per work group.
 * Refused (TT2_E_INVALID, nothing is launched or written): NULL args; head_dim != 64; causal != 0;
 * n_layers < 0 or n_layers > TT2_GUIDE_MAX_LAYERS; a dtype other than bf16 or f32; batch, tq or tk
 * < 0, heads <= 0, scale <= 0 or NaN, batch * heads above INT32_MAX; q_ld or k_ld that is no
 * multiple of 16 bytes or is below heads * 64; NULL pmax or amax; a NULL q[l], k[l] or lse[l] with
 * l < n_layers; for the MFMA kernel one batch element's q or k spanning more than 2 GiB
 * ((tq * q_ld + 64) * 2 bytes above INT32_MAX, likewise tk * k_ld); for the plain kernel more than
 * 65535 (batch, head) pairs. */
typedef struct tt2_align_args {
  const void* q[TT2_GUIDE_MAX_LAYERS];      /* per layer: [batch*tq, >= heads*64], row stride q_ld */
  const void* k[TT2_GUIDE_MAX_LAYERS];      /* per layer: [batch*tk, >= heads*64], row stride k_ld */
  const float* lse[TT2_GUIDE_MAX_LAYERS];   /* per layer: [batch*heads, tq] f32, as the forward saved it */
  int64_t q_ld, k_ld;
  const int32_t* key_len; const int32_t* q_len;   /* [batch], device (NULL: tk / tq) */
  float* pmax;      /* [n_layers, batch*heads, tq] f32 */
  int32_t* amax;    /* [n_layers, batch*heads, tq] int32 */
  int32_t n_layers, batch, heads, head_dim, tq, tk, dtype, causal;
  float scale;
  int32_t variant;
} tt2_align_args;
int tt2_attn_align(const tt2_align_args* a, hipStream_t stream);

/* Focus rates and phoneme durations from tt2_attn_align's output (the FastSpeech teacher
 * procedure), one work group per utterance, fixed summation order and integer counts only, so
 * the results are bit-identical run to run.  With Ty_b = min(tq, q_len[b]) valid rows:
 *   focus[i][b][h] = mean over n < Ty_b of pmax[i][b*heads + h][n]     (0 if Ty_b = 0)
 *   mode 0: sel[b] = {layer slot, head} of utterance b's greatest focus (lowest flat index
 *           slot*heads + head on ties);  mode 1: sel[b] = {sel_layer, sel_head} for every b
 *   sel_focus[b]    = focus of the chosen head
 *   durations[b][t] = #{n < Ty_b : amax of the chosen head at n == t}, t < tk   (int32)
 * durations[b][t] is exactly 0 for t >= key_len[b], and sum_t durations[b][t] = Ty_b whenever
 * utterance b has a visible key (else 0).  An amax entry that is negative or at or past
 * min(tk, key_len[b]) counts nowhere; pmax / amax rows n >= Ty_b are not read.
 * Refused (TT2_E_INVALID, nothing is launched or written): NULL args; a NULL pmax, amax, focus,
 * sel, sel_focus or durations; n_layers < 1 or n_layers > TT2_GUIDE_MAX_LAYERS; batch, tq or tk < 0,
 * heads <= 0, n_layers * heads above 1024; a mode other than 0 or 1; in mode 1 a sel_layer outside
 * [0, n_layers) or a sel_head outside [0, heads). */
typedef struct tt2_align_dur_args {
  const float* pmax; const int32_t* amax;         /* [n_layers, batch*heads, tq] */
  const int32_t* key_len; const int32_t* q_len;   /* [batch], device (NULL: tk / tq) */
  float* focus;          /* [n_layers, batch, heads] f32 */
  int32_t* sel;          /* [batch, 2] int32 */
  float* sel_focus;      /* [batch] f32 */
  int32_t* durations;    /* [batch, tk] int32 */
  int32_t n_layers, batch, heads, tq, tk;
  int32_t mode, sel_layer, sel_head;
} tt2_align_dur_args;
int tt2_align_durations(const tt2_align_dur_args* a, hipStream_t stream);

/* Monotonic alignment search (Viterbi over the raw scores of forwards already run; no attention
 * matrix is stored).  One work group per utterance.  For utterance b the (layer slot, head) is
 * sel[2b], sel[2b+1] read on the device (as tt2_align_durations writes it), or sel_layer /
 * sel_head when sel is NULL.  With Ty = clamp(q_len[b], 0, tq), Tx = clamp(key_len[b], 0, tk),
 * Te = min(Tx, Ty) and s[n, t] the unscaled f32 score q_n . k_t (bf16, variant 0: the v3 forward's
 * MFMA sequence; f32 or variant 1: tt2_attn_align's scalar dot), the path pi maximises
 * sum_n s[n, pi(n)] over pi(0) = 0, pi(Ty-1) = Te-1, pi(n+1) - pi(n) in {0, 1}:
 *   V[0][0] = s[0][0], V[0][t>0] = -inf, V[n][t] = s[n][t] + max(V[n-1][t], V[n-1][t-1]),
 *   move[n][t] = V[n-1][t-1] > V[n-1][t]   (strict: a tie stays on the same key),
 *   backtrack from (Ty-1, Te-1): pi(n-1) = pi(n) - move[n][pi(n)].
 * Every row's log-sum-exp is common to all paths and scale > 0, so this is the maximum-likelihood
 * monotone path of log P.  Outputs:
 *   path[b][n]      = pi(n) for n < Ty, -1 for n >= Ty
 *   durations[b][t] = #{n : pi(n) = t}  (0 for t >= Te; the row sums to Ty; >= 1 for every t < Tx
 *                     when Ty >= Tx)
 *   logp[b]         = mean over n < Ty of ln 2 * (s[n, pi(n)] * scale * log2(e) - lse[n])  (f32,
 *                     fixed summation order)
 * Ty = 0, Tx = 0 or a sel entry outside [0, n_layers) x [0, heads) gives path = -1, durations = 0
 * and logp = 0 for that utterance (nothing is read through such an entry).  Results are
 * bit-identical run to run (integer counts, no floating-point atomics).
 * Limits: head_dim 64, non-causal, scale > 0, 1..16 layers, tk <= TT2_MONO_MAX_KEYS,
 * tq <= TT2_MONO_MAX_FRAMES, leading dims and the 2 GiB span as in tt2_attn_align.  The move bits
 * (tq rows of C/32 words, C = tk rounded up to 128, 256 or 512) stay in LDS when they fit;
 * otherwise they go to `workspace` (8-B aligned, tt2_align_monotonic_workspace_size bytes, which is
 * 0 when LDS suffices); a smaller workspace is refused (TT2_E_INVALID).
 * variant: 0 auto (bf16: MFMA score producer, f32: plain), 1 the plain scalar-dot producer. */
#define TT2_MONO_MAX_KEYS 512
#define TT2_MONO_MAX_FRAMES 4096
typedef struct tt2_align_mono_args {
  const void* q[TT2_GUIDE_MAX_LAYERS];      /* as tt2_align_args */
  const void* k[TT2_GUIDE_MAX_LAYERS];
  const float* lse[TT2_GUIDE_MAX_LAYERS];
  int64_t q_ld, k_ld;
  const int32_t* key_len; const int32_t* q_len;   /* [batch], device (NULL: tk / tq) */
  const int32_t* sel;      /* [batch, 2] (layer slot, head), device (NULL: sel_layer / sel_head) */
  int32_t* path;           /* [batch, tq] int32 */
  int32_t* durations;      /* [batch, tk] int32 */
  float* logp;             /* [batch] f32 */
  void* workspace; size_t workspace_bytes;
  int32_t n_layers, batch, heads, head_dim, tq, tk, dtype, causal, sel_layer, sel_head, variant;
  float scale;
} tt2_align_mono_args;
size_t tt2_align_monotonic_workspace_size(int batch, int tq, int tk);
int tt2_align_monotonic(const tt2_align_mono_args* a, hipStream_t stream);

/* Dynamic time warping between two feature sequences per utterance (the alignment under
 * mel-cepstral distortion, MCD-DTW).  One work group per utterance pair.  For utterance b with
 * Na = clamp(a_len[b], 0, ta) and Nb = clamp(b_len[b], 0, tb):
 *   cost        c[i][j] = sqrt(sum_{k=c0}^{c1-1} (a[i][k] - b[j][k])^2), formed from the differences
 *               in f32 with an IEEE-rounded square root (a perfect square comes out exact);
 *   recurrence  D[0][0] = c[0][0], otherwise D[i][j] = c[i][j] + min over the existing predecessors
 *               (i-1, j-1), (i-1, j), (i, j-1), in f32 with one add per cell.  The predecessor is the
 *               diagonal if its D is <= both others, else up (i-1, j) if its D is <= left's, else
 *               left: a tie prefers diagonal, then up, then left;
 *   total[b]    = D[Na-1][Nb-1];
 *   length[b]   = L, the number of cells on the path that follows the chosen predecessors back from
 *               (Na-1, Nb-1) to (0, 0); max(Na, Nb) <= L <= Na + Nb - 1.  It is carried through the
 *               recurrence beside D, so without a path no move bits and no workspace are needed;
 *   path        (when path_a and path_b are given) path_a[b][k], path_b[b][k] for k < L are the
 *               path's cells in forward order, (0, 0) first and (Na-1, Nb-1) last; entries from L
 *               up to ta + tb - 2 are -1.
 * Na = 0 or Nb = 0 gives total 0, length 0 and a path of -1; nothing is read through that
 * utterance's pointers.  Only rows < Na / Nb and columns [c0, c1) of a and b are read.  Results
 * are bit-identical run to run (no floating-point atomics, no hand-off between work groups).
 * The path needs `workspace` (4-B aligned) of tt2_dtw_workspace_size bytes for the move codes:
 * 2 bits per cell, 16 rows of one column per word.  The size is 0 without a path or with a zero
 * dimension.  Refused with TT2_E_INVALID before any launch: ta or tb > TT2_DTW_MAX_FRAMES or < 0,
 * c1 - c0 outside 1..TT2_DTW_MAX_FEATS, c0 < 0, a_ld or b_ld < c1, batch < 0, exactly one path
 * pointer, a path with a workspace below the size query, a null total or length (or a null a / b
 * with rows to read).  batch, ta or tb = 0 succeeds; with ta or tb = 0 total and length are
 * written as 0. */
#define TT2_DTW_MAX_FRAMES 2048
#define TT2_DTW_MAX_FEATS  32
typedef struct tt2_dtw_args {
  const float* a; const float* b;              /* [batch, ta, a_ld], [batch, tb, b_ld] f32, row-major */
  const int32_t* a_len; const int32_t* b_len;  /* [batch] or NULL (= ta / tb); clamped to [0, ta] / [0, tb] */
  float* total; int32_t* length;               /* [batch] */
  int32_t* path_a; int32_t* path_b;            /* [batch, ta + tb - 1], or both NULL: no path wanted */
  void* workspace; size_t workspace_bytes;
  int64_t a_ld, b_ld;                          /* floats per row, >= c1 */
  int32_t batch, ta, tb, c0, c1;               /* features [c0, c1) enter the cost; 1 <= c1 - c0 <= TT2_DTW_MAX_FEATS */
} tt2_dtw_args;
size_t tt2_dtw_workspace_size(int batch, int ta, int tb, int want_path);
int tt2_dtw(const tt2_dtw_args* a, hipStream_t stream);

/* YIN pitch (de Cheveigne & Kawahara 2002, steps 1-5, without the best-local-estimate step) and
 * RMS energy per frame, on the padded sample buffer tt2_reflect_pad produces.  One wave per frame.
 * Frame (b, f) is y[j] = x[b * utt_stride + f * hop + j], j < TT2_YIN_FRAME: with hop 256 the
 * samples of mel frame f.  The integration window is W = TT2_YIN_WINDOW and tau <= TT2_YIN_MAX_LAG,
 * so W + tau stays inside the frame.  All arithmetic is f32:
 *   d(tau)    = sum_{j<W} (y[j] - y[j + tau])^2 for tau = 1 .. tau_max, d(0) = 0;
 *   S(tau)    = sum_{k=1..tau} d(k);
 *   d'(0)     = 1, d'(tau) = (d(tau) * tau) / S(tau) when S(tau) > 0, else 1: one multiply and one
 *               correctly rounded divide;
 *   search    ascending over [tau_min, tau_max]: the first tau with d'(tau) < threshold; while
 *               tau + 1 <= tau_max and d'(tau + 1) < d'(tau) (strictly), step to tau + 1.  That
 *               tau is the lag and the frame is voiced.  Without such a tau the frame is unvoiced
 *               and the lag is the lowest tau that attains the minimum of d' over the range;
 *   aper      = d'(lag), the same bits;
 *   f0        = 0 when unvoiced.  Voiced with tau_min < lag < tau_max: with a, b, c = d'(lag - 1),
 *               d'(lag), d'(lag + 1), off = 0.5 (a - c) / ((a - b) + (c - b)) (the search makes
 *               a > b and c >= b, so the denominator is positive) and f0 = sr / (lag + off).
 *               Voiced with the lag at an end of the range: f0 = sr / lag;
 *   energy    = sqrt((sum_{j<1024} y[j]^2) * 2^-10), an IEEE-rounded square root.
 * d(tau) is summed over j ascending with one fma per term (the difference is rounded, its square
 * is not); S(tau) is a running sum over 8 lags plus a scan over groups of 8, and the energy's sum a
 * tree: fixed orders, not the sequential one.  Where d, S and d * tau are exactly representable
 * (small integer samples) every output bit is defined by the above.
 * Frames with f >= clamp(frames[b], 0, t) write f0 = 0, lag = -1, aper = 1, energy = 0, read
 * nothing, and leave their cmnd row untouched.  A valid frame reads exactly its 1024 samples and
 * writes cmnd[0 .. tau_max] of its row, nothing after.  A frame with a non-finite sample has
 * f0 = 0; its other outputs are unspecified.  Results are bit-identical run to run (no
 * floating-point atomics).
 * Refused with TT2_E_INVALID before any launch: 1 <= tau_min <= tau_max <= TT2_YIN_MAX_LAG
 * violated; hop < 1, utt_stride < 0, batch < 0 or t < 0; sr or threshold not finite and positive;
 * a null f0, lag, aper or energy, or a null x with frames to read; cmnd with cmnd_ld <
 * tau_max + 1; more than 2^31 - 1 work groups (batch * ceil(t / 4)).  batch = 0 or t = 0 succeeds
 * without a launch. */
#define TT2_YIN_FRAME   1024
#define TT2_YIN_WINDOW  512
#define TT2_YIN_MAX_LAG 511
typedef struct tt2_yin_args {
  const float* x;            /* padded samples; frame (b, f) at x + b*utt_stride + f*hop, 1024 floats */
  const int32_t* frames;     /* [batch] valid frames, device, or NULL (= t) */
  float* f0; int32_t* lag; float* aper; float* energy;   /* [batch, t] */
  float* cmnd;               /* optional [batch, t, cmnd_ld]: d'(0..tau_max) of every valid frame */
  int64_t utt_stride, cmnd_ld;
  int32_t batch, t, hop, tau_min, tau_max;
  float sr, threshold;
} tt2_yin_args;
int tt2_yin(const tt2_yin_args* a, hipStream_t stream);

/* Viterbi pitch tracking over the d' that tt2_yin writes to `cmnd`: one path per utterance through
 * the lags and one unvoiced state, instead of tt2_yin's decision per frame.  One work group per
 * utterance.  For utterance b, N = clamp(frames[b], 0, t) (frames NULL: N = t).  The states are the
 * lags tau in [tau_min, tau_max] plus one unvoiced state; c(f, tau) = cmnd[(b * t + f) * cmnd_ld + tau];
 * p = the `pos` table (f32, [tau_max + 1], device); J, W, C = jump, switch_cost, unvoiced.  All
 * arithmetic is f32:
 *   V[0][tau] = c(0, tau)                    U[0] = C
 *   A[f][tau] = min over tau' of ( V[f-1][tau'] + J * |p[tau] - p[tau']| ); the lowest tau' wins a tie
 *   V[f][tau] = c(f, tau) + ( U[f-1] + W if that is strictly less than A[f][tau], else A[f][tau] )
 *   m[f]      = min over tau' of V[f-1][tau'] (the lowest tau' on a tie)
 *   U[f]      = C + ( m[f] + W if that is strictly less than U[f-1], else U[f-1] )
 *   end       unvoiced if U[N-1] is strictly less than min over tau of V[N-1][tau], else the lowest
 *             tau of that minimum
 *   cost[b]   = the end state's value; 0 when N = 0.
 * |p[tau] - p[tau']| is one subtraction; J times it plus V is one fma here (two rounded operations
 * give the same bits wherever the product is exact).  A minimum of f32 values does not depend on
 * the order in which it is taken, and the kernel splits it across waves.  The path follows the
 * recorded decisions back from the end state:
 *   lag[b][f]  the lag of a voiced frame, 0 for an unvoiced frame f < N, -1 for f >= N;
 *   f0[b][f]   0 when unvoiced or f >= N.  Voiced with lag tau and a, b, c = c(f, tau - 1), c(f, tau),
 *              c(f, tau + 1): if tau_min < tau < tau_max, a > b and c >= b, then f0 = sr / (tau + off),
 *              off = 0.5 (a - c) / ((a - b) + (c - b)), tt2_yin's operations with IEEE divides;
 *              otherwise f0 = sr / tau.  (The tracked lag need not be a local minimum of d'.)
 * Only columns [tau_min, tau_max] of rows f < N of cmnd are read; every element of f0 and lag with
 * f < t is written.  A non-finite cmnd value in a valid frame leaves that utterance's outputs
 * unspecified, but every lag written is -1, 0 or inside the range, nothing is read or written out
 * of bounds and the other utterances are unaffected.  Results are bit-identical run to run (no
 * floating-point atomics, no hand-off between work groups).
 * `workspace` (4-B aligned) of tt2_pitch_track_workspace_size bytes holds the value history the
 * backtrack reads: per utterance [t][tau_max - tau_min + 2] f32, V of the lags then U.  The size is
 * 0 when batch or t is 0 (or the lag range is malformed).
 * Refused with TT2_E_INVALID before any launch: t > TT2_PITCH_TRACK_MAX_FRAMES; 1 <= tau_min <=
 * tau_max <= TT2_YIN_MAX_LAG violated; batch < 0 or t < 0; cmnd_ld < tau_max + 1; sr not finite and
 * positive; jump, switch_cost or unvoiced not finite or negative; a null f0, lag, cost or pos; a
 * null cmnd with frames to read; a workspace below the size query.  batch = 0 or t = 0 succeeds
 * without a kernel launch; with t = 0 and batch > 0 cost is set to 0 (a memset on the stream). */
#define TT2_PITCH_TRACK_MAX_FRAMES 4096
typedef struct tt2_pitch_track_args {
  const float* cmnd;         /* [batch, t, cmnd_ld] f32: d' as tt2_yin writes it */
  const int32_t* frames;     /* [batch] valid frames, device, or NULL (= t) */
  const float* pos;          /* [tau_max + 1] f32, device: the position of each lag on the jump axis */
  float* f0; int32_t* lag;   /* [batch, t] */
  float* cost;               /* [batch] */
  void* workspace; size_t workspace_bytes;
  int64_t cmnd_ld;           /* floats per row, >= tau_max + 1 */
  int32_t batch, t, tau_min, tau_max;
  float sr, jump, switch_cost, unvoiced;   /* `switch` of the definition: a keyword in C */
} tt2_pitch_track_args;
size_t tt2_pitch_track_workspace_size(int batch, int t, int tau_min, int tau_max);
int tt2_pitch_track(const tt2_pitch_track_args* a, hipStream_t stream);

/* Sample-rate conversion by a rational factor up / down with a polyphase FIR bank: one launch for a
 * batch of utterances, no host synchronisation.  For sr_in -> sr_out, g = gcd(sr_in, sr_out),
 * up = sr_out / g and down = sr_in / g.  `bank` is [up, bank_ld] f32: row r holds the 2 * half + 1
 * taps of the outputs n with n mod up = r, tap k = -half .. half at column k + half.  The bank is the
 * caller's; tt2.audio.resample_bank designs the Kaiser-windowed sinc
 *   h(t) = c sinc(c t) w(c t / zeros),  c = rolloff * min(1, up / down),  sinc(x) = sin(pi x) / (pi x),
 *   w(u) = I0(beta sqrt(1 - u^2)) / I0(beta) for |u| < 1, else 0,  half = ceil(zeros / c),
 *   bank[r][k + half] = h(k - f_r),  f_r = ((r * down) mod up) / up,
 * in float64, rounded once to f32.  For utterance b, len_b = clamp(lens[b], 0, n_in) (lens NULL:
 * n_in) and out_b = min(ceil(len_b * up / down), n_out), the ceiling in 64-bit arithmetic.  For
 * n = q * up + r < out_b, with i0 = q * down + floor(r * down / up) (= floor(n * down / up)),
 *   y[b][n] = sum_{k = -half .. half} bank[r][k + half] * x[b][i0 + k],
 * where a sample with i0 + k outside [0, len_b) counts as 0 and is not read.  All arithmetic is f32.
 * The sum is one accumulator that starts at +0 and takes k ascending from -half to half with one fma
 * per tap (the product is not rounded), the taps of samples outside the utterance included (an fma
 * with 0).  The order does not depend on the tiling, so an output value does not depend on batch,
 * n_out or the utterance's position in the batch; results are bit-identical run to run (no atomics),
 * and where every product and partial sum is exactly representable every output bit is defined by
 * the above.  y[b][n] is exactly 0 for out_b <= n < n_out; nothing is written at or past column
 * n_out of a row; out_lens[b] = out_b when out_lens is given.  No sample at an index >= len_b is
 * read, and no element outside [0, x_ld) of a row.  Every index that can reach n * down is 64-bit.
 * Refused with TT2_E_INVALID before any launch: up < 1, down < 1 or up > TT2_RESAMPLE_MAX_PHASES;
 * half < 0 or 2 * half + 1 > TT2_RESAMPLE_MAX_TAPS; batch, n_in or n_out negative; x_ld < n_in,
 * y_ld < n_out or bank_ld < 2 * half + 1; a null bank or y, or a null x with samples to read
 * (batch, n_out and n_in all positive); more than 2^31 - 1 work groups.  batch = 0 or n_out = 0
 * succeeds without a launch (out_lens is then not written); n_in = 0 with n_out > 0 launches and
 * zero-fills. */
#define TT2_RESAMPLE_MAX_TAPS   256   /* 2*half + 1 */
#define TT2_RESAMPLE_MAX_PHASES 1024  /* up */
typedef struct tt2_resample_args {
  const float* x;          /* [batch, x_ld] */
  const int32_t* lens;     /* [batch] valid input samples, device, or NULL (= n_in) */
  const float* bank;       /* [up, bank_ld] f32, row r = taps k = -half..half */
  float* y;                /* [batch, y_ld] */
  int32_t* out_lens;       /* optional [batch] */
  int64_t x_ld, y_ld, bank_ld;
  int32_t batch, n_in, n_out, up, down, half;
} tt2_resample_args;
int tt2_resample(const tt2_resample_args* a, hipStream_t stream);

/* Leading and trailing silence trimming of a batch of utterances, on frame energies relative to the
 * utterance's loudest frame (librosa.effects.trim's rule with ref = np.max): three launches, no host
 * synchronisation.  For utterance b, len_b = clamp(lens[b], 0, n_in) (lens NULL: n_in).  The frame
 * length is frame = 2 * r * hop; F_b = 0 when len_b = 0, otherwise F_b = 1 + len_b / hop (integer
 * division).  Frame f covers the samples [f * hop - r * hop, f * hop + r * hop) within [0, len_b):
 * centred, zero-padded frames, the grid of librosa.feature.rms(center=True, pad_mode="constant").
 * Samples outside the utterance count as 0 and are not read.
 *   Frame energy.  e[b][f] is the f32 sum of x^2 over the frame, taken through blocks: block j is
 * the samples [j * hop, (j + 1) * hop) within [0, len_b), n of them.  Sample i of a block belongs to
 * lane (i / 4) mod 64; a lane adds its squares (each rounded to f32) to one accumulator from +0 with
 * i ascending, and the 64 accumulators are added in one fixed tree.  The order depends on hop and n
 * alone, never on batch, on the utterance's position, on n_in or on the row's alignment.  e[b][f] is
 * the sum, from +0 in ascending block order, of the sums of blocks f - r .. f + r - 1; blocks outside
 * [0, ceil(len_b / hop)) contribute +0.  Where every square and partial sum is exactly representable
 * in f32, every bit is thereby defined.
 *   Decision.  emax_b = max over f < F_b of e[b][f].  Frame f is loud iff e[b][f] > ratio * emax_b
 * (one f32 multiply, a strict compare): an all-zero utterance has no loud frame, and a frame exactly
 * on the threshold is silent.  With f0 the lowest and f1 the highest loud frame,
 *   start_b = max(0, f0 * hop - keep),  end_b = min(len_b, (f1 + 1) * hop + keep)
 * in 64-bit arithmetic; with no loud frame start_b = end_b = 0.  Interior silence is kept.
 *   Outputs.  out_b = min(end_b - start_b, n_out); y[b][i] = x[b][start_b + i] for i < out_b (the
 * sample's bits, copied) and exactly +0 for out_b <= i < n_out; nothing is written at or past column
 * n_out of a row.  out_lens[b] = out_b and start[b] = start_b where those pointers are given;
 * energy[b][f] = e[b][f] for f < F_b and 0 for F_b <= f < n_in / hop + 1 when energy is given.  No
 * sample at an index >= len_b is read.  A non-finite sample leaves that utterance's outputs
 * unspecified; even then nothing is read or written out of bounds,
 * 0 <= start <= start + out_b <= len_b holds, and other utterances are unaffected.  Results are
 * bit-identical run to run (no floating-point atomics).
 *   `workspace` (16-B aligned) of tt2_trim_workspace_size(batch, n_in, hop) bytes holds the block
 * sums and each utterance's (start, out).
 *   Refused with TT2_E_INVALID before any launch: hop < 1; r < 1 or r > TT2_TRIM_MAX_R; 2 * r * hop
 * beyond int32; keep < 0; ratio not finite, < 0 or > 1; batch, n_in or n_out negative; x_ld < n_in or
 * y_ld < n_out; energy given with energy_ld < n_in / hop + 1; a null y; a null x with samples to read
 * (batch, n_out and n_in all positive); a workspace below the size query; more than 2^31 - 1 work
 * groups.  batch = 0 or n_out = 0 succeeds without a launch (out_lens, start and energy are then not
 * written); n_in = 0 with n_out > 0 launches, zero-fills and writes out_lens = start = 0. */
#define TT2_TRIM_MAX_R 16   /* frame = 2 * r * hop */
typedef struct tt2_trim_args {
  const float* x;          /* [batch, x_ld] */
  const int32_t* lens;     /* [batch] valid input samples, device, or NULL (= n_in) */
  float* y;                /* [batch, y_ld] */
  int32_t* out_lens;       /* optional [batch] */
  int32_t* start;          /* optional [batch] */
  float* energy;           /* optional [batch, energy_ld] */
  void* workspace; size_t workspace_bytes;
  int64_t x_ld, y_ld, energy_ld;
  int32_t batch, n_in, n_out, hop, r, keep;
  float ratio;
} tt2_trim_args;
size_t tt2_trim_workspace_size(int batch, int n_in, int hop);
int tt2_trim(const tt2_trim_args* a, hipStream_t stream);

/* Integrated loudness of a batch of utterances by the gating of ITU-R BS.1770-4 over a two-section
 * weighting filter, and a gain to a target level under a peak ceiling: five launches, no host
 * synchronisation.  For utterance b, len_b = clamp(lens[b], 0, n_in) (lens NULL: n_in); samples at or
 * past len_b are never read.  All arithmetic is IEEE float64 unless it says f32: at the K-weighting's
 * pole radius of 0.989 (22.05 kHz) f32 carries do not survive a chunked evaluation.
 *   Filter.  coef holds b0 b1 b2 a1 a2 of section 1, then of section 2 (a0 = 1); section 2 reads
 * section 1's output.  Each is y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2] from zero
 * state at n = 0.  It is evaluated in transposed direct form II, per sample and with fma(a, b, c) one
 * rounding:
 *   y1 = fma(b0, x, z1);  z1' = fma(b1, x, fma(-a1, y1, z2));  z2' = fma(-a2, y1, b2 * x)
 * and the same for section 2 on y1 with state (w1, w2).  One sample advances s = (z1, z2, w1, w2) by
 * s' = A s + B x, so the utterance is cut into chunks of 16 samples (chunk c holds samples 16 c ..
 * 16 c + 15) and segments of 64 chunks: every chunk is run from zero state, the end states e are
 * combined over a segment by an inclusive Kogge-Stone scan, at distance d = 1, 2, .. 32 chunk c with
 * c mod 64 >= d taking e_c <- M_d e_(c-d) + e_c, M_d = A^(16 d), each row of the product
 * fma(m3, v3, fma(m2, v2, fma(m1, v1, fma(m0, v0, e)))); the segments' end states are combined by the
 * same scan with A^(1024 d), 64 segments a round, the first of a round taking the state that enters
 * the round; then the scan over a segment's chunks is repeated with the segment's first chunk run
 * from the segment's entry state, which gives every chunk's exact entry state, and every chunk is run
 * from it.  The powers of A come from coef alone: A by its entries (-a1, 1; -a2, 0 for a section,
 * b1' - a1' b0' and b2' - a2' b0' of section 2 under z1), then repeated squaring with each element a
 * sum of four products in ascending index order.  The order depends on len_b and coef alone, never
 * on batch, on the utterance's position, on n_in, x_ld or the row's alignment.
 *   Energy.  sub[b][j] is the sum of y^2 (each square rounded) over the samples [j * step,
 * (j + 1) * step), for j < S_b = len_b / step (integer division; a partial last sub-block is not
 * used).  It is the sum, from +0 in ascending segment order, of one piece per segment that the
 * sub-block touches; a piece's sample i (counted from the piece's first) belongs to lane i mod 64, a
 * lane adds its own from +0 with i ascending, and the 64 lanes are added in one fixed xor tree.
 * Block j < N_b = max(0, S_b - 3) has the sum E_j = ((sub[j] + sub[j+1]) + sub[j+2]) + sub[j+3].
 *   Gates.  Block j passes the absolute gate iff E_j > abs_sum (strict).  G1 = (the sum of the passing
 * E_j from +0, j ascending) / their count.  Block j passes both gates iff it passes the absolute gate
 * and E_j > rel_ratio * G1 (one multiply, strict); G2 is the mean of those, formed the same way, and
 * ms_b = G2 / (4 * step).  When no block passes (N_b = 0, silence, everything gated) the utterance is
 * unmeasured.  A block exactly on a threshold fails it.
 *   Results.  loud_b = f32(-0.691 + 10 * log10(ms_b)), -inf when unmeasured.  peak_b = max |x| over
 * the valid samples, exact, 0 for len_b = 0.  g_b = f32(min(sqrt(target_ms / ms_b), ceiling /
 * peak_b)), the ceiling term absent when peak_b = 0; limited_b = 1 iff the ceiling term is strictly
 * the smaller.  Unmeasured: g_b = 1, limited_b = 0.  (The two f32 roundings, of g_b and of g_b * x, can
 * carry the largest sample one f32 ulp past ceiling.)
 *   Outputs.  y[b][i] = g_b * x[b][i] (one f32 multiply; for g_b = 1 the sample's own bits) for
 * i < min(len_b, n_out) and exactly +0 for the remaining columns below n_out; nothing is written at
 * or past column n_out.  y NULL measures only.  loud, gain, peak [batch] f32 and limited [batch]
 * int32 are written where given.  energy[b][j] = f32(sub[b][j]) for j < S_b and 0 for
 * S_b <= j <= n_in / step when given.  A non-finite sample leaves that utterance's outputs
 * unspecified; even then nothing is read or written out of bounds and other utterances are
 * unaffected.  Results are bit-identical run to run (no floating-point atomics), and no work group
 * waits on another inside a kernel.
 *   `workspace` (16-B aligned) of tt2_loudness_workspace_size(batch, n_in, step) bytes holds the
 * gains, and per segment a state, a peak and its pieces, and the sub-block sums.
 *   Refused with TT2_E_INVALID before any launch: step < 1 or 4 * step beyond int32; batch, n_in or
 * n_out negative; x_ld < n_in; y given with y_ld < n_out; energy given with energy_ld < n_in / step
 * + 1; a coefficient that is not finite; abs_sum negative or not finite; rel_ratio outside [0, 1];
 * target_ms or ceiling not finite or <= 0; a null x with samples to read (batch and n_in positive);
 * every output null; a workspace below the size query; more than 2^31 - 1 work groups.  batch = 0
 * succeeds without a launch. */
typedef struct tt2_loudness_args {
  const float* x;          /* [batch, x_ld] */
  const int32_t* lens;     /* [batch] valid input samples, device, or NULL (= n_in) */
  float* y;                /* optional [batch, y_ld] */
  float* loud;             /* optional [batch] */
  float* gain;             /* optional [batch] */
  float* peak;             /* optional [batch] */
  int32_t* limited;        /* optional [batch] */
  float* energy;           /* optional [batch, energy_ld] */
  void* workspace; size_t workspace_bytes;
  int64_t x_ld, y_ld, energy_ld;
  int32_t batch, n_in, n_out, step;
  double coef[10];
  double abs_sum, rel_ratio, target_ms;
  float ceiling;
} tt2_loudness_args;
size_t tt2_loudness_workspace_size(int batch, int n_in, int step);
int tt2_loudness(const tt2_loudness_args* a, hipStream_t stream);

/* ---------------------------------------------------------- length regulator
 * Phoneme states and integer durations to frame states (FastSpeech's length regulator), and the
 * gradient of that expansion: three entries, one launch each, no workspace, no host synchronisation,
 * no floating-point atomics; results are bit-identical run to run.
 *   tt2_regulate_plan.  For utterance b, Tx_b = clamp(key_len[b], 0, tx) (key_len NULL: tx) and
 * d'[b][t] = max(durations[b][t], 0) for t < Tx_b; entries at t >= Tx_b are not read and count as 0.
 * S[b][t] is the sum of d'[b][u] over u <= t in 64-bit integers (two phonemes of 2^31 - 1 frames do
 * not wrap).  ends[b][t] = min(S[b][t], n_out) is written for every t < tx, so it is constant from
 * Tx_b - 1 on and all 0 when Tx_b = 0.  frames[b] = ends[b][tx - 1] (0 when tx = 0);
 * total[b] = min(S[b][tx - 1], 2^31 - 1) (0 when tx = 0), so that total > frames shows a truncation
 * at n_out.  index[b][n] is the lowest t with ends[b][t] > n for n < frames[b] (a phoneme of zero
 * duration owns no frame) and -1 for frames[b] <= n < n_out.  index, frames and total are optional;
 * nothing is written at or past column tx of ends or column n_out of index.  One work group scans
 * one utterance with its ends in LDS, which is the limit tx <= TT2_REGULATE_MAX_PHONEMES (16 KB).
 *   tt2_regulate_fwd (map = index).  y[b][n][c] = h[b][index[b][n]][c] where 0 <= index[b][n] < tx,
 * the element's bits copied (-0, denormals, infinities and NaN payloads survive), and exactly +0
 * where the index is outside [0, tx), for n < n_out and c < dim; src = h, dst = y.  Nothing is
 * written at or past column dim of a row or row n_out of an utterance; whatever index holds, nothing
 * is read out of bounds; rows of h that no frame names are not read.
 *   tt2_regulate_bwd (map = ends).  With s = clamp(ends[b][t-1], 0, n_out) (0 for t = 0) and
 * e = clamp(ends[b][t], 0, n_out): dh[b][t][c] = from_f32(acc), where the f32 accumulator acc starts
 * at +0 and adds to_f32(dy[b][n][c]) for n = s, s + 1, .., e - 1 in ascending n, one IEEE f32 add
 * each (no contraction, no reordering), and is rounded once, to nearest even, to the output dtype at
 * the end; e <= s gives exactly +0.  src = dy, dst = dh.  dh is written for every t < tx and c < dim
 * (the rows past Tx_b hold +0: ends is constant there); rows of dy at or past ends[b][tx - 1] are not
 * read (ends as tt2_regulate_plan writes them).  Every bit of dh is thereby defined for any input.
 * This is the gradient of the expansion with respect to h, and on its own the sum of frame values
 * per phoneme.  The cost of a phoneme is proportional to its duration and a phoneme is summed by one
 * lane per column, so the longest phoneme of a launch is its tail; long runs are not split, because
 * that would change the order of the sum.
 *   Row element (b, r, c) of src or dst is at base + b * bs + r * ld + c, in elements of `dtype`
 * (TT2_DT_F32 or TT2_DT_BF16, the same for both): activations may be column slices of wider
 * buffers.  Any dim and any element alignment work; rows move in 16-byte chunks where both bases sit
 * on 16 bytes and every ld, bs and dim is a whole number of chunks, element by element otherwise,
 * with the same result.
 *   Refused with TT2_E_INVALID before any launch, with a message that starts with the entry's name:
 * null args; batch, tx, n_out or dim negative; tx > TT2_REGULATE_MAX_PHONEMES; dur_ld < tx,
 * ends_ld < tx, index given with index_ld < n_out (plan); src_ld < dim, dst_ld < dim, map_ld < n_out
 * (fwd) or < tx (bwd); a dtype other than f32 / bf16; more than 2^31 - 1 work groups; then, where
 * the call has something to do, a null pointer it would read or write: durations or ends with
 * tx > 0 (plan), dst, and src or map with tx > 0 (fwd) or n_out > 0 (bwd).
 *   Zero sizes.  batch = 0 succeeds without a launch, in all three.  plan with n_out = 0 still writes
 * ends (all 0), frames and total; with tx = 0 it writes frames = total = 0 and index = -1.  fwd with
 * n_out = 0 or dim = 0 succeeds without a launch, and with tx = 0 writes +0 to every row (src and
 * map may be NULL).  bwd with tx = 0 or dim = 0 succeeds without a launch, and with n_out = 0 writes
 * +0 to every row of dh (src and map may be NULL). */
#define TT2_REGULATE_MAX_PHONEMES 4096
typedef struct tt2_regulate_plan_args {
  const int32_t* durations;  /* [batch, dur_ld] */
  const int32_t* key_len;    /* [batch] valid phonemes, device, or NULL (= tx) */
  int32_t* ends;             /* [batch, ends_ld] */
  int32_t* index;            /* optional [batch, index_ld] */
  int32_t* frames;           /* optional [batch] */
  int32_t* total;            /* optional [batch] */
  int64_t dur_ld, ends_ld, index_ld;
  int32_t batch, tx, n_out;
} tt2_regulate_plan_args;
typedef struct tt2_regulate_args {
  const void* src;           /* fwd: h [batch, tx, dim]; bwd: dy [batch, n_out, dim] */
  void* dst;                 /* fwd: y [batch, n_out, dim]; bwd: dh [batch, tx, dim] */
  const int32_t* map;        /* fwd: index [batch, map_ld]; bwd: ends [batch, map_ld] */
  int64_t src_ld, src_bs, dst_ld, dst_bs, map_ld;   /* row and batch strides, in elements */
  int32_t batch, tx, n_out, dim, dtype;
} tt2_regulate_args;
int tt2_regulate_plan(const tt2_regulate_plan_args* a, hipStream_t stream);
int tt2_regulate_fwd(const tt2_regulate_args* a, hipStream_t stream);
int tt2_regulate_bwd(const tt2_regulate_args* a, hipStream_t stream);

/* ---------------------------------------------------------- forward-sum alignment loss
 * The total probability of all monotone alignments of a (frame, phoneme) score matrix, its
 * posterior, its gradient and its best path: the teacher-free alignment learning of RAD-TTS /
 * FastPitch 1.1 / JETS (CTC over the phoneme sequence without a useful blank; Badlani et al. 2021).
 * One work group per utterance, no host synchronisation, no floating-point atomics and every order
 * fixed: all outputs are bit-identical run to run.
 *   Inputs.  For utterance b, Ty = clamp(q_len[b], 0, tq), Tx = clamp(key_len[b], 0, tk) and
 * Te = min(Tx, Ty); a NULL length vector means tq / tk.  Score s[n][t] (f32) is at
 * scores + b * s_bs + n * s_ld + t, the strides in elements, so [B, 1, Ty, Tx] tensors and column
 * slices go in as they are.  ls[n][t] = s[n][t] - ln sum_{u < Tx} exp s[n][u]: the log-softmax runs
 * over the utterance's own phonemes only and is fused; a caller with a prior passes
 * scores + log_prior.  Rows n >= Ty and columns t >= Tx are never read.
 *   Paths.  tt2_align_monotonic's set: pi(0) = 0, pi(Ty-1) = Te-1, pi(n+1) - pi(n) in {0, 1}.
 *   Partition and loss.  Z = sum_pi prod_n exp ls[n][pi(n)], loss[b] = -ln Z in nats; 0 when Ty = 0
 * or Tx = 0.
 *   Posterior.  gamma[n][t] = P(pi(n) = t) = exp(alpha[n][t] + beta[n][t] - ln Z) with
 *     alpha[0][0] = ls[0][0], alpha[n][t] = ls[n][t] + logaddexp(alpha[n-1][t], alpha[n-1][t-1]),
 *     beta[Ty-1][Te-1] = 0,
 *     beta[n][t] = logaddexp(ls[n+1][t] + beta[n+1][t], ls[n+1][t+1] + beta[n+1][t+1]).
 * Every row of gamma sums to 1.
 *   Gradient.  dscores[n][t] = grad_loss[b] * (P[n][t] - gamma[n][t]) with P = exp ls: every path
 * visits every row once, so this is the exact gradient with respect to the raw scores.  grad_loss is
 * a device vector [batch]; NULL means 1.
 *   Padding.  gamma and dscores are exactly +0 for n >= Ty or t >= Tx; they are written for every
 * n < tq, t < tk and nothing at or past column tk.
 *   Numerics.  ls is formed as (s - m) - ln sum exp(s - m) with m the row's maximum, which keeps the
 * precision of a small ls; lse = m + that logarithm.  alpha and beta are carried relative to a per-row offset, the row's maximum, which is
 * subtracted after every row; the offsets are summed in float64, so the stored values stay O(ln Tx)
 * near the mass.  A cell no path reaches holds -1e30 instead of -inf.  gamma[n][.] is the softmax
 * over t of the stored alpha + beta, in which the offsets cancel.
 *   tt2_forward_sum_fwd writes loss [batch], the row log-sum-exps lse [batch, tq] (0 for n >= Ty)
 * and, unless alpha is NULL, the renormalised alpha [batch, tq, a_ld] for n < Ty, t < Te (its other
 * cells are left as they were; only tt2_forward_sum_bwd reads it).  A loss-only call (alpha NULL)
 * gives the same loss bit for bit.  No workspace.
 *   tt2_forward_sum_bwd reads scores, lse and alpha as tt2_forward_sum_fwd left them, runs the beta
 * pass into `workspace` (16-B aligned, tt2_forward_sum_bwd_workspace_size bytes) and writes dscores
 * and / or gamma (either may be NULL, not both) in a second, element-parallel launch.
 *   tt2_forward_sum_path is the binarisation: V, move (strict: a tie stays) and the backtrack are
 * tt2_align_monotonic's, over the raw f32 s with one add per cell and no renormalisation.
 *     path[b][n]      = pi(n) for n < Ty, -1 for n >= Ty
 *     durations[b][t] = #{n : pi(n) = t}, 0 for t >= Te
 *     logp[b]         = (sum over n < Ty of ls[n][pi(n)]) / Ty, the sum in a fixed order
 * Ty = 0 or Tx = 0 gives -1, 0 and 0.  The move bits stay in LDS when they fit, as in
 * tt2_align_monotonic; otherwise they go to `workspace` (8-B aligned,
 * tt2_forward_sum_path_workspace_size bytes, 0 when LDS suffices).
 *   Contract.  Scores are finite.  NaN or +-inf inside one utterance may make that utterance's
 * outputs NaN; every other utterance's outputs stay bit-identical.
 *   Limits: tk <= TT2_FSUM_MAX_KEYS, tq <= TT2_FSUM_MAX_FRAMES, f32 scores and gradients only.
 *   Refused with TT2_E_INVALID before any launch, with a message that starts with the entry's name:
 * null args; batch, tq or tk negative; tq or tk over the limits; s_ld < tk; alpha given (fwd) or
 * needed (bwd) with a_ld < tk; dscores given with d_ld < tk, gamma given with g_ld < tk; more than
 * 2^31 - 1 work groups; a workspace that is too small or misaligned; then, where the call has
 * something to do, a null pointer it would read or write: loss (fwd, batch > 0), lse (fwd with
 * tq > 0; bwd), scores (batch, tq and tk positive), alpha (bwd), both of dscores and gamma (bwd),
 * path with tq > 0, durations with tk > 0 and logp (path).
 *   Zero sizes.  batch = 0 succeeds without a launch, in all three.  With tq = 0 or tk = 0, fwd writes
 * loss = 0 (and lse = 0), bwd has nothing to write and succeeds without a launch, and path writes
 * path = -1, durations = 0 and logp = 0 where they exist. */
#define TT2_FSUM_MAX_KEYS 512
#define TT2_FSUM_MAX_FRAMES 4096
typedef struct tt2_forward_sum_args {
  const float* scores;       /* s[b][n][t] at scores + b * s_bs + n * s_ld + t */
  const int32_t* q_len; const int32_t* key_len;   /* [batch], device (NULL: tq / tk) */
  float* loss;               /* [batch]: fwd writes */
  float* lse;                /* [batch, tq]: fwd writes, bwd reads */
  float* alpha;              /* [batch, tq, a_ld]: fwd writes (optional), bwd reads */
  const float* grad_loss;    /* [batch], device (NULL: 1): bwd reads */
  float* dscores;            /* d[b][n][t] at dscores + b * d_bs + n * d_ld + t: bwd writes (optional) */
  float* gamma;              /* the same with g_bs, g_ld: bwd writes (optional) */
  int32_t* path;             /* [batch, tq]: path writes */
  int32_t* durations;        /* [batch, tk]: path writes */
  float* logp;               /* [batch]: path writes */
  void* workspace; size_t workspace_bytes;
  int64_t s_ld, s_bs, a_ld, d_ld, d_bs, g_ld, g_bs;   /* in elements */
  int32_t batch, tq, tk;
} tt2_forward_sum_args;
size_t tt2_forward_sum_bwd_workspace_size(int batch, int tq, int tk);
size_t tt2_forward_sum_path_workspace_size(int batch, int tq, int tk);
int tt2_forward_sum_fwd(const tt2_forward_sum_args* a, hipStream_t stream);
int tt2_forward_sum_bwd(const tt2_forward_sum_args* a, hipStream_t stream);
int tt2_forward_sum_path(const tt2_forward_sum_args* a, hipStream_t stream);

/* ---------------------------------------------------------- Gaussian upsampling
 * The soft length regulator (Non-Attentive Tacotron, Parallel Tacotron; ESPnet's GaussianUpsampling
 * in JETS and VITS): phoneme states to frame states through softmax weights that are a function of
 * two per-phoneme vectors and the frame index, and the gradient with respect to the states and to
 * both vectors (and to an optional bias).  An attention whose scores are analytic: the
 * [frames, phonemes] weight matrix is never written, forward or backward.  No host synchronisation,
 * no floating-point atomics, every reduction order fixed: all outputs are bit-identical run to run.
 *   Lengths.  For utterance b, Tx_b = clamp(key_len[b], 0, tx) and Ty_b = clamp(q_len[b], 0, n_out);
 * both are device vectors and NULL means tx / n_out.
 *   Per-phoneme inputs.  center, prec and (optional) bias are f32 [batch, p_ld] with finite values
 * and prec >= 0; entries at t >= Tx_b are never read.
 *   Frame position.  x_n = n + offset, with offset a float argument.
 *     e[n][t] = bias[t] - prec[t] * (x_n - center[t])^2         t < Tx_b   (bias NULL: 0)
 *     W[n][.] = softmax over t < Tx_b of e[n][.]                 (row maximum subtracted)
 *     y[n][c] = sum_{t < Tx_b} W[n][t] * h[t][c]                 n < Ty_b, c < dim
 *     lse[n]  = ln sum_t exp e[n][t]                             n < Ty_b
 * y is accumulated in f32 and rounded once to the output dtype.  y and lse are exactly +0 for
 * Ty_b <= n < n_out and when Tx_b = 0; nothing is written at or past column dim or row n_out; rows
 * of h at t >= Tx_b are never read.  ESPnet's convention is prec = delta, bias NULL, offset = 0;
 * Non-Attentive Tacotron's is prec = 1 / (2 sigma^2), bias = -ln sigma, offset = 1.
 *   tt2_gauss_upsample_fwd writes y and lse in one launch (online softmax over phoneme tiles).  With
 * a bf16 dtype the weights of a tile enter the matrix product rounded to bf16 (relative to the
 * running row maximum), the products are exact and the accumulation is f32; with f32 every product is
 * an f32 product.
 *   tt2_gauss_upsample_bwd reads h, center, prec, bias, dy, and the y and lse the forward left.  With
 * delta[n] = sum_c dy[n][c] y[n][c], dW[n][t] = sum_c dy[n][c] h[t][c] and dE = W o (dW - delta),
 * all sums over n < Ty_b:
 *     dh[t][c]   =  sum_n W[n][t] dy[n][c]
 *     dbias[t]   =  sum_n dE[n][t]
 *     dcenter[t] =  sum_n dE[n][t] * 2 prec[t] (x_n - center[t])
 *     dprec[t]   = -sum_n dE[n][t] (x_n - center[t])^2
 * W is recomputed as exp(e - lse).  Each of the four outputs is optional (NULL), at least one must be
 * asked for, and each is the same bit for bit whichever others are asked for.  Each is written for
 * every t < tx and is exactly +0 at t >= Tx_b; rows of dy and y at n >= Ty_b are never read.  dbias
 * may be asked for with bias NULL.  A work group owns 32 phonemes and walks frames in ascending order;
 * an utterance of more than 128 frames is shared among up to 16 work groups per phoneme tile, whose
 * f32 partials go through `workspace` and are added in ascending order of their frames by a last
 * launch (the split is a function of n_out alone).  delta goes through `workspace` too: 16-B aligned,
 * tt2_gauss_upsample_bwd_workspace_size bytes: 0 when batch, tx or n_out is 0, else 4 batch n_out for
 * delta plus, with s > 1 work groups per phoneme tile, 4 s batch tx (dim + 3) for the partials (each
 * part rounded up to 16 bytes).
 *   Types and layout.  h, y, dy and dh share one dtype, TT2_DT_F32 or TT2_DT_BF16.  Element (b, r, c)
 * of each is at base + b * bs + r * ld + c in elements, so column slices of wider buffers go in as
 * they are; any dim and any element alignment work, rows moving into LDS in 16-byte chunks where the
 * base sits on 16 bytes and ld, bs and dim are whole numbers of chunks, element by element otherwise,
 * with the same result.  center, prec, bias and their gradients share the row stride p_ld; lse is
 * [batch, lse_ld].  Everything per phoneme or per frame is f32.
 *   Contract.  Inputs are finite.  NaN or +-inf inside one utterance may make that utterance's
 * outputs NaN; every other utterance's outputs stay bit-identical.
 *   Limits: tx <= TT2_REGULATE_MAX_PHONEMES, dim <= TT2_UPSAMPLE_MAX_DIM.
 *   Refused with TT2_E_INVALID before any launch, with a message that starts with the entry's name:
 * null args; batch, tx, n_out or dim negative; tx or dim over the limits; a dtype other than f32 /
 * bf16; h_ld < dim, y_ld < dim, p_ld < tx, lse_ld < n_out; dy_ld < dim, dh given with dh_ld < dim
 * (bwd); an offset that is negative or not finite; more than 2^31 - 1 work groups; a workspace that
 * is too small or misaligned (bwd); then, where the call has something to do, a null pointer it
 * would read or write: lse, y with dim > 0, and center, prec or (dim > 0) h with tx > 0 (fwd); all
 * four outputs null, and with n_out > 0 center, prec, lse or (dim > 0) h, dy, y (bwd).
 *   Zero sizes.  batch = 0 succeeds without a launch, in both.  fwd with n_out = 0 succeeds without a
 * launch and with tx = 0 writes +0 to every row of y and lse (h, center and prec may be NULL).  bwd
 * with tx = 0 succeeds without a launch and with n_out = 0 writes +0 to every output asked for (the
 * inputs may be NULL). */
#define TT2_UPSAMPLE_MAX_DIM 512
typedef struct tt2_gauss_upsample_args {
  const void* h;             /* [batch, tx, dim] */
  const float* center;       /* [batch, p_ld] */
  const float* prec;         /* [batch, p_ld] */
  const float* bias;         /* optional [batch, p_ld] */
  const int32_t* q_len; const int32_t* key_len;   /* [batch], device (NULL: n_out / tx) */
  void* y;                   /* [batch, n_out, dim]: fwd writes, bwd reads */
  float* lse;                /* [batch, lse_ld]: fwd writes, bwd reads */
  const void* dy;            /* [batch, n_out, dim]: bwd reads */
  void* dh;                  /* optional [batch, tx, dim]: bwd writes */
  float* dcenter;            /* optional [batch, p_ld]: bwd writes */
  float* dprec;              /* optional [batch, p_ld]: bwd writes */
  float* dbias;              /* optional [batch, p_ld]: bwd writes */
  void* workspace; size_t workspace_bytes;
  int64_t h_ld, h_bs, y_ld, y_bs, dy_ld, dy_bs, dh_ld, dh_bs, p_ld, lse_ld;   /* in elements */
  int32_t batch, tx, n_out, dim, dtype;
  float offset;
} tt2_gauss_upsample_args;
size_t tt2_gauss_upsample_bwd_workspace_size(int batch, int tx, int n_out, int dim);
int tt2_gauss_upsample_fwd(const tt2_gauss_upsample_args* a, hipStream_t stream);
int tt2_gauss_upsample_bwd(const tt2_gauss_upsample_args* a, hipStream_t stream);

/* ------------------------------------------------------------------ decode
 * One query row per batch element (the AR decode step):
 * out[b*o_ld + 64h ..] = softmax(scale q k^T) v over keys j < n_b of batch b,
 * key j of batch b at k + b*k_bstride + j*k_ld + 64h.  n_b = min(tk, *t_ptr + 1
 * if t_ptr, key_len[b] if key_len): t_ptr is the DEVICE step counter, so the
 * call is replayable from a captured graph. */
typedef struct tt2_attn_decode_args {
  const void* q; const void* k; const void* v; void* out;
  int64_t q_ld, k_bstride, k_ld, v_bstride, v_ld, o_ld;
  const int32_t* key_len;
  const int32_t* t_ptr;
  int32_t batch, heads, head_dim, tk, dtype;
  float scale;
  /* optional early exit: when stop_len != NULL, batch element b is finished once
   * *step >= stop_len[b] (step defaults to t_ptr); its output row is 0 and no key is read */
  const int32_t* stop_len;
  const int32_t* step;
  /* optional fused output projection (wo != NULL): the workgroup of (b, h) also writes
   * slab[(h * batch + b) * heads * head_dim + n] = sum_j o[b, h, j] * wo[n * wo_ld + h * head_dim + j]
   * (f32, n < heads * head_dim): one split-K slab per head for tt2_ln_combine (splits = heads),
   * which adds the bias; out may then be NULL */
  const void* wo;
  int64_t wo_ld;
  float* slab;
  /* optional fused query projection (wq != NULL): q is then the projection INPUT x [batch][q_ld]
   * (heads * head_dim wide) and the head's query is
   * q[b, h, j] = sum_k x[b, k] * wq[(h * head_dim + j) * wq_ld + k] + bq[h * head_dim + j]
   * (f32 accumulation, the query kept in f32): the decoder's cross-attention query GEMM
   * rides in the attention launch */
  const void* wq;
  int64_t wq_ld;
  const float* bq;
  /* optional fused residual combine + LayerNorm of the projection input (ln_part != NULL; needs
   * wq, 8 heads, q_ld == 512, bf16 / f16): the input row is x[b] = LN(q[b] + ln_bias +
   * sum_{s<8} ln_part[(s * batch + b) * 512 + :]) exactly as tt2_ln_combine(splits = 8) computes
   * it (the self-attention's output-projection slabs), and the workgroup of head 0 writes it to
   * ln_out[b] (the next sublayer's residual): the decoder's first post-LN rides in this launch */
  const float* ln_part;
  const float* ln_bias;
  const float* ln_gamma;
  const float* ln_beta;
  void* ln_out;
  float ln_eps;
} tt2_attn_decode_args;
/* Refused with TT2_E_INVALID before any launch (no output is touched): null q / k / v; batch <= 0,
 * heads <= 0 or tk < 0; a dtype other than TT2_DT_BF16 / TT2_DT_F16 / TT2_DT_F32; head_dim != 64;
 * q_ld, k_ld, v_ld, k_bstride or v_bstride that is not a multiple of 16 bytes; wq with a wq_ld that
 * is not, or with heads * head_dim != 512; wo without slab, with such a wo_ld or with heads *
 * head_dim > 512; ln_part without wq, 8 heads, ln_bias / ln_gamma / ln_beta / ln_out, q_ld == 512
 * and a 16-bit dtype; out == NULL without wo; stop_len with neither step nor t_ptr.
 * n_b == 0 (tk == 0, key_len[b] <= 0) gives a zero row, never NaN. */
int tt2_attn_decode(const tt2_attn_decode_args* a, hipStream_t stream);
/* cache[b*c_bstride + (*t_ptr)*c_ld + c] = src[b*src_ld + c], c < n, b < batch; dtype TT2_DT_BF16,
 * TT2_DT_F16 or TT2_DT_F32 (of src and cache).  A step past the cache ((*t_ptr) * c_ld >= c_bstride,
 * i.e. *t_ptr >= t_max of a [batch][t_max][c_ld] cache) writes nothing.  Refused with TT2_E_INVALID
 * before any launch: null src / cache / t_ptr, batch <= 0, n <= 0, any other dtype. */
int tt2_kv_append(const void* src, int64_t src_ld, void* cache, int64_t c_bstride, int64_t c_ld, int n, int batch,
                  const int32_t* t_ptr, int dtype, hipStream_t stream);
/* heads [batch, heads_ld] f32 -> mel_seq[b, t, :], stop_seq[b, t] (+ stop_bias[b, t] if given),
 * prev[b, :] (prev_dtype); stop_len[b] = t + 1 at the first stop logit >= stop_thr (if given);
 * then *t_ptr += 1 and *seed += 1 (seed may be NULL), with t = *t_ptr on entry.  The first stop
 * wins: stop_len[b] changes only while it is > t (the caller arms it with a value >= t_max, e.g.
 * INT32_MAX), and from the step after it the frames of b are stored as zeros (mel_seq and prev;
 * stop_seq keeps the logit).  t >= t_max: nothing is written and *t_ptr and *seed stay (the counter
 * saturates).  Refused with TT2_E_INVALID before any launch: null heads / mel_seq / stop_seq /
 * prev / t_ptr, batch <= 0, n_mels <= 0, t_max <= 0, heads_ld < n_mels + 1, a prev_dtype other
 * than TT2_DT_BF16 / TT2_DT_F16 / TT2_DT_F32. */
int tt2_decode_emit(const float* heads, int64_t heads_ld, int batch, int n_mels, int t_max, float* mel_seq,
                    float* stop_seq, void* prev, int prev_dtype, int32_t* t_ptr, uint32_t* seed,
                    const float* stop_bias, int32_t* stop_len, float stop_thr, hipStream_t stream);
/* The decode step's whole FFN sublayer in ONE launch (the decoder layer's
 * FFN + third post-LN, modeling_speecht5.py's SpeechT5FeedForward + final_layer_norm):
 *   hidden = relu(x W1^T + b1)            (m x d_ffn, stored in `hidden`, dtype)
 *   slab[s] = hidden[:, 256 s ..] W2[:, 256 s ..]^T   (s < 8, raw f32 partial sums)
 *   y = LN(x + b2 + sum_s slab[s]) * gamma + beta
 * with the arithmetic of the three launches it replaces (tt2_gemm act = relu, tt2_gemm splits = 8
 * main_only, tt2_ln_combine splits = 8): bit-identical results, but slower than those three
 * launches on MI355X (its two in-kernel hand-offs between work groups cost more than two launch
 * boundaries), so the decode step uses it only under schedule 4.  256 work groups that order the
 * three phases among themselves through the counters at `sync` (TT2_FFN_SYNC_INTS int32, zero
 * before the first call; every call leaves them zero again; sync[TT2_FFN_SYNC_ERR] != 0 afterwards
 * means a phase timed out and the outputs are invalid).  m <= 64, d_model 512, d_ffn 2048, dtype TT2_DT_BF16 or TT2_DT_F16,
 * 16-B aligned rows; anything else is TT2_E_INVALID.  Replayable from a captured graph. */
typedef struct tt2_ffn_decode_args {
  const void* x;                      /* [m][512] FFN input and residual */
  const void* w1; const float* b1;    /* [2048][512], [2048] */
  const void* w2; const float* b2;    /* [512][2048], [512] */
  const float* gamma; const float* beta;
  void* hidden;                       /* [m][2048] scratch */
  float* slab;                        /* [8][m][512] scratch */
  int32_t* sync;                      /* [TT2_FFN_SYNC_INTS] */
  void* y;                            /* [m][512] */
  int32_t m, d_model, d_ffn, dtype;
  float eps;
} tt2_ffn_decode_args;
#define TT2_FFN_SYNC_INTS 2048
#define TT2_FFN_SYNC_ERR 1088
int tt2_ffn_decode(const tt2_ffn_decode_args* a, hipStream_t stream);
/* measurement hook: also 8 device wall-clock stamps per work group into stamps[256][8] */
int tt2_ffn_decode_stamps(const tt2_ffn_decode_args* a, uint64_t* stamps, hipStream_t stream);

/* ------------------------------------------------------------ decode step / graph
 * The whole autoregressive decode step (the loop body of
 * modeling_speecht5.py:2215-2267 with a KV cache): pre-net on the previous frame (optional
 * always-on dropout, sites 128 / 129, seed = *seed, bumped every step) -> scaled PE at the
 * device step t -> n_layers x [self-attention with KV-cache append, cross-attention over the
 * encoder memory K/V, FFN, post-LNs] -> mel / stop heads -> frame emit, t += 1.  The library
 * composes the launches itself, so a non-Python host (C++, a JNI / cgo binding) can drive
 * inference; tt2_decode_graph_create captures one step as a hipGraph that the library owns,
 * and tt2_decode_graph_launch replays it n times.
 *
 * Early exit: an utterance finishes at the first frame whose stop logit (+ stop_bias) reaches
 * stop_logit (stop_len[b] = that frame + 1); afterwards its attention reads no keys.  The
 * caller polls stop_len between launches (stop_logit = +inf: forced length).  Frames emitted after
 * an utterance's stop are zero, so a batched post-net sees each utterance zero-padded at its length.
 *
 * Weights are in the step dtype (bf16 / f16 / f32, [out, in] row-major as in the checkpoint);
 * biases, LayerNorm parameters, alpha and the PE table are f32.  All buffers are caller-owned;
 * the workspace (tt2_decode_workspace_size bytes) holds the KV cache and step activations. */
#define TT2_MAX_DEC_LAYERS 16
typedef struct tt2_dec_layer {
  const void* qkv_w; const float* qkv_b;     /* self-attention in_proj [3d, d] */
  const void* o_w; const float* o_b;         /* self-attention out_proj [d, d] */
  const float* ln1_g; const float* ln1_b;
  const void* cq_w; const float* cq_b;       /* cross-attention query rows of in_proj [d, d] */
  const void* co_w; const float* co_b;       /* cross-attention out_proj [d, d] */
  const float* ln2_g; const float* ln2_b;
  const void* ffn1_w; const float* ffn1_b;   /* [F, d] */
  const void* ffn2_w; const float* ffn2_b;   /* [d, F] */
  const float* ln3_g; const float* ln3_b;
} tt2_dec_layer;

typedef struct tt2_decode_desc {
  int32_t batch, text_len, t_max, n_layers, d_model, n_heads, d_ffn, n_mels, prenet_dim;
  int32_t dtype;        /* step storage type: TT2_DT_BF16, TT2_DT_F16 (batch <= 64) or TT2_DT_F32 */
  int32_t schedule;     /* 0 auto, 1 plain (one launch per op), 2 split-K (16-bit, batch <= 64; output
                         * projections fused into the attention launches), 3 split-K without that
                         * fusion, 4 split-K with it and each FFN sublayer as one tt2_ffn_decode
                         * launch (bit-identical to 2, measured slower: opt-in) */
  float ln_eps;
  float prenet_dropout; /* 0 = off (Tacotron2 keeps it on at inference) */
  float stop_logit;     /* logit(stop_threshold); +inf never stops */
  const void* fc1_w; const float* fc1_b;     /* pre-net [P, n_mels], [P, P], proj [d, P] */
  const void* fc2_w; const float* fc2_b;
  const void* proj_w; const float* proj_b;
  const float* alpha;                        /* decoder PE scale (device scalar) */
  const float* pe_table;                     /* [>= t_max + 1][d] */
  tt2_dec_layer layers[TT2_MAX_DEC_LAYERS];
  const void* heads_w; const float* heads_b; /* [n_mels + 1, d]: mel rows, then the stop row */
  const void* mem_kv;        /* [batch * text_len, n_layers * 2d]: layer l's K at column 2dl, V at 2dl + d */
  const int32_t* text_lens;  /* [batch] phonemes per utterance */
  float* mel_seq;            /* out [batch][t_max][n_mels] (pre-post-net frames) */
  float* stop_seq;           /* out [batch][t_max] */
  int32_t* stop_len;         /* out [batch]; INT32_MAX while running */
  const float* stop_bias;    /* optional [batch][t_max] */
  int32_t* step;             /* device step counter */
  uint32_t* seed;            /* device dropout seed */
  void* workspace; size_t ws_bytes;
} tt2_decode_desc;
typedef struct tt2_decode_graph* tt2_decode_graph_t;

size_t tt2_decode_workspace_size(const tt2_decode_desc* d);
/* step = 0, seed = seed0, previous frame = 0 (the go frame), stop_len = INT32_MAX */
int tt2_decode_reset(const tt2_decode_desc* d, uint32_t seed0, hipStream_t stream);
/* one step as eager launches */
int tt2_decode_step(const tt2_decode_desc* d, hipStream_t stream);
int tt2_decode_graph_create(const tt2_decode_desc* d, hipStream_t stream, tt2_decode_graph_t* out);
/* also captures `steps` (1..64) consecutive steps as a second graph: a launch of n steps then
 * replays it n / steps times (one graph boundary per `steps` frames) and the one-step graph for
 * the rest.  tt2_decode_graph_create == steps 1. */
int tt2_decode_graph_create_n(const tt2_decode_desc* d, int32_t steps, hipStream_t stream, tt2_decode_graph_t* out);
/* n_steps replays.  The device step counter saturates at t_max: replays past it write no
 * KV-cache row, emit no frame and leave every output unchanged. */
int tt2_decode_graph_launch(tt2_decode_graph_t g, int32_t n_steps, hipStream_t stream);
int tt2_decode_graph_destroy(tt2_decode_graph_t g);

/* ------------------------------------------------------------- reductions */
#define TT2_COLSUM_ROWS 128
#define TT2_BN_ROWS_PER_CHUNK 64
#define TT2_PE_BWD_BLOCKS 1024
#define TT2_LOSS_BLOCKS 1024
#define TT2_ADAM_NORM_BLOCKS 1024

/* dst[c] = beta*dst[c] + sum_r src[r*ld + c] (fixed summation order) */
typedef struct tt2_reduce_args {
  const float* src; float* dst;
  int64_t ld; int32_t rows, cols;
  float beta;
} tt2_reduce_args;
int tt2_reduce_rows(const tt2_reduce_args* a, hipStream_t stream);

/* Bias gradient: dst[n] = beta*dst[n] + sum_m x[m*ld + n]. */
size_t tt2_colsum_workspace_size(int m, int n);
int tt2_colsum(const void* x, int dtype, int64_t ld, int m, int n, float* dst, float beta, void* ws,
               size_t ws_bytes, hipStream_t stream);

/* ------------------------------------------------------------- LayerNorm
 * fwd: y = LN(x + drop(branch)) (branch may be NULL), mean/rstd [m] f32 saved.
 * bwd: dx = dL/ds (residual stream), dbranch = drop'(dx); dgamma/dbeta (f32)
 *      = grad_beta*old + sum over rows.  C must be 512 (d_model).
 * Replaces the post-LN residual blocks of SURVEY 8(a) a3, a4, a6, a7. */
typedef struct tt2_ln_args {
  const void* x; const void* branch; const void* dy;
  void* y; void* dx; void* dbranch;
  const float* gamma; const float* beta;
  float* mean; float* rstd;
  float* dgamma; float* dbeta;
  void* workspace; size_t ws_bytes;
  const uint32_t* drop_seed;
  int32_t m, c, dtype;
  float eps, grad_beta;
  uint32_t drop_site, drop_thr;
  float drop_scale;
  float* dbias;   /* bwd, optional: grad_beta*dbias + column sums of the branch gradient
                     (= the bias gradient of the linear layer that produced `branch`) */
  int32_t defer_finalize;   /* bwd: leave the per-workgroup column partials in `workspace`
                               and do not write dgamma/dbeta/dbias yet: a later
                               tt2_layernorm_bwd (finalize_prev) or
                               tt2_layernorm_bwd_finalize completes them */
  const struct tt2_ln_args* finalize_prev;   /* bwd, optional: a deferred earlier call
                               (same c) whose dgamma/dbeta/dbias this launch completes in its
                               spare lanes; its workspace must not have been reused since */
} tt2_ln_args;
int tt2_layernorm_fwd(const tt2_ln_args* a, hipStream_t stream);
size_t tt2_layernorm_bwd_workspace_size(const tt2_ln_args* a);
/* tt2_gemm_grouped that also completes `fin`, a deferred LayerNorm backward (defer_finalize
 * = 1, partials still in its workspace), inside the group's split-K reduce launch: a layer's
 * last LayerNorm gradients need no launch of their own.  fin may be NULL; n may be 0. */
int tt2_gemm_grouped_fin(const tt2_gemm_args* probs, int32_t n, const tt2_ln_args* fin, hipStream_t stream);
/* tt2_gemm_grouped_fin with at most max_groups work groups at a time (rounded down to a multiple
 * of 8; 0: every 256 x 128 item at once): the items go out as consecutive launches of that many,
 * so a launch beside other work on a second stream leaves the remaining CUs to that work. */
int tt2_gemm_grouped_ex(const tt2_gemm_args* probs, int32_t n, const tt2_ln_args* fin, int32_t max_groups,
                        hipStream_t stream);
int tt2_layernorm_bwd(const tt2_ln_args* a, hipStream_t stream);
/* Completes a deferred tt2_layernorm_bwd (defer_finalize = 1): dgamma/dbeta/dbias from the
 * partials it left in a->workspace.  Same fixed summation order as a chained finalize. */
int tt2_layernorm_bwd_finalize(const tt2_ln_args* a, hipStream_t stream);
/* Decode-step residual combine + LayerNorm (x / y of dtype bf16 or f16, c = 512):
 *   y[m, :] = LN(x[m, :] + bias + sum_{s < splits} part[s][m][:]) * gamma + beta
 * part: the raw f32 partial slabs [splits][m][c] of a skinny split-K projection (tt2_gemm
 * with splits > 1 and main_only; splits 1, 2, 4, 8 or 16), summed in a fixed order.
 * Replaces the output-projection epilogue + residual + LayerNorm of a decoder sublayer
 *  where splitting K spreads the weight stream over more CUs. */
int tt2_ln_combine(const void* x, const float* part, int32_t splits, const float* bias, const float* gamma,
                   const float* beta, void* y, int32_t m, int32_t c, float eps, int32_t dtype, hipStream_t stream);

/* ------------------------------------------------------------- BatchNorm
 * fwd: out = drop(act((y - mean)*rstd*gamma + beta)) (+ res), statistics over
 *      all m rows (training: batch stats + running update; eval: running stats).
 * bwd: dy from dout (dtype dout_dtype), dgamma/dbeta written (f32).
 * Replaces the Conv1d+BatchNorm blocks of SURVEY 8(a) a1 (relu) and a9 (tanh). */
typedef struct tt2_bn_args {
  const void* y; const void* dout; const void* res;
  void* out; void* dy;
  const float* gamma; const float* beta;
  float* mean; float* rstd;
  float* run_mean; float* run_var;
  float* dgamma; float* dbeta;
  void* workspace; size_t ws_bytes;
  const uint32_t* drop_seed;
  int64_t res_ld;  /* row stride of res (elements) */
  int32_t m, c, act, dtype, out_dtype, res_dtype, dout_dtype, training;
  float eps, momentum;
  uint32_t drop_site, drop_thr;
  float drop_scale;
  /* SyncBatchNorm (the *_stats / *_apply phases below; ignored by tt2_batchnorm_fwd/bwd) */
  float* sync_buf;               /* tt2_batchnorm_sync_size bytes, 16-B aligned */
  int32_t sync_world, sync_rank;
  /* stats_rows > 0 says the workspace already holds this pass's per-chunk column statistics in
   * chunks of stats_rows rows, so the statistics pass over the rows is skipped: the training
   * forward's moments of y (tt2_gemm col_stats) or the backward's sums (tt2_gemm bn_bwd; both
   * with stats_rows = TT2_GEMM_STATS_ROWS); tt2_batchnorm_workspace_size then gives that layout's
   * size.  0: the pass runs (its own chunking). */
  int32_t stats_rows;
} tt2_bn_args;
size_t tt2_batchnorm_workspace_size(const tt2_bn_args* a);
/* The training forward with stats_rows = 0 keeps each chunk's mean relative to the chunk's first
 * row of y and reads those rows again while it applies, so `out` must either be y itself (in
 * place: same pointer, same dtype; the chunk means are then kept as absolute f32 values, which
 * costs accuracy only where |mean| is many times the column's spread) or not overlap y at all. */
int tt2_batchnorm_fwd(const tt2_bn_args* a, hipStream_t stream);
int tt2_batchnorm_bwd(const tt2_bn_args* a, hipStream_t stream);
/* SyncBatchNorm over sync_world data-parallel ranks, rank r holding its own m_r rows (ranks
 * may differ: torch.nn.SyncBatchNorm's semantics, training statistics and the backward's
 * column sums over all sum_r m_r rows, each rank weighted by its row count; the dgamma / dbeta
 * parameter gradients stay this rank's sums, for the gradient all-reduce).
 * Each pass is two phases around a caller-issued SUM all-reduce of the first
 * sync_world * 4 * c floats of sync_buf ([W][4][c]: this rank's slot holds its moments / sums,
 * its row count m and, forward, the low part of its mean, which travels as an f32 pair; the
 * other slots zeros, so the reduced slots are exact and rank-ordered on every rank):
 *   tt2_batchnorm_fwd_stats -> all-reduce -> tt2_batchnorm_fwd_apply   (training only)
 *   tt2_batchnorm_bwd_stats -> all-reduce -> tt2_batchnorm_bwd_apply
 * sync_world = 1 reproduces tt2_batchnorm_fwd / _bwd (no exchange needed).  The optional
 * SyncBN of SURVEY.md:219 (per-replica statistics stay the default). */
size_t tt2_batchnorm_sync_size(const tt2_bn_args* a);
int tt2_batchnorm_fwd_stats(const tt2_bn_args* a, hipStream_t stream);
int tt2_batchnorm_fwd_apply(const tt2_bn_args* a, hipStream_t stream);
int tt2_batchnorm_bwd_stats(const tt2_bn_args* a, hipStream_t stream);
int tt2_batchnorm_bwd_apply(const tt2_bn_args* a, hipStream_t stream);

/* -------------------------------------------------- embedding / pos. enc. */
int tt2_embedding_fwd(const int64_t* ids, const void* table, void* out, int m, int c, int vocab, int dtype,
                      hipStream_t stream);
/* dtable (f32) row v = sum of dout rows with ids == v, added in increasing row order (gathered per
 * table row: deterministic, no atomics); every row is written; rows == pad_idx get zero */
int tt2_embedding_bwd(const int64_t* ids, const void* dout, float* dtable, int m, int c, int vocab, int pad_idx,
                      int dtype, hipStream_t stream);

/* out = drop(x + alpha*pe[row % t + t_offset (+ *t_ptr if t_ptr)]); bwd: dx = drop'(dout),
 * *dalpha = sum dx*pe */
typedef struct tt2_pe_args {
  const void* x; const void* dout; void* out; void* dx;
  const float* alpha; const float* pe; float* dalpha;
  void* workspace; size_t ws_bytes;
  const uint32_t* drop_seed;
  const int32_t* t_ptr;
  int32_t m, c, t, t_offset, dtype;
  uint32_t drop_site, drop_thr;
  float drop_scale;
} tt2_pe_args;
int tt2_posenc_fwd(const tt2_pe_args* a, hipStream_t stream);
size_t tt2_posenc_bwd_workspace_size(void);
int tt2_posenc_bwd(const tt2_pe_args* a, hipStream_t stream);

/* teacher forcing: out[b*t + j] = j == 0 ? 0 : mel[b, j-1] (mel f32 [batch, t, c]) */
int tt2_shift_right(const float* mel, void* out, int batch, int t, int c, int dtype, hipStream_t stream);
int tt2_cast2d(const void* src, int src_dtype, int64_t src_ld, void* dst, int dst_dtype, int64_t dst_ld, int m,
               int n, hipStream_t stream);

/* ------------------------------------------------------------------- loss
 * heads [batch*t, heads_ld] f32 (cols 0..n_mels-1 mel_before, col n_mels stop logit),
 * mel_after [batch*t, n_mels] f32, target f32 [batch, t, n_mels].
 * loss_out[4] = (total, mse_before, mse_after, bce_stop); gradients: g_heads
 * (f32, heads_ld; mel cols carry before + after terms), g_after (grad_dtype).
 * Frame (b, j) is valid iff j < mel_len[b]; the terms are means over the N = sum_b
 * min(max(mel_len[b], 0), t) valid frames, the stop label is 1 at j == mel_len[b] - 1 (none within
 * a sequence cut off at t), padded frames get zero gradients, N == 0 gives zero losses and
 * gradients, and g_heads' columns above n_mels are written as zeros.
 * Replaces SURVEY 8(a) a10. */
typedef struct tt2_loss_args {
  const float* heads; const float* mel_after; const float* target;
  const int32_t* mel_len;
  float* loss_out; float* g_heads; void* g_after;
  void* workspace; size_t ws_bytes;
  int64_t heads_ld;
  int32_t batch, t, n_mels, grad_dtype;
  float pos_weight;
  float grad_scale;  /* multiplies every gradient (1/world_size under data parallelism) */
  int32_t separate_grads;  /* 1: g_heads' mel columns hold only d/d(mel_before) (no residual
                              d/d(mel_after) term folded in): the autograd boundary's layout */
} tt2_loss_args;
size_t tt2_loss_workspace_size(void);
int tt2_tts_loss(const tt2_loss_args* a, hipStream_t stream);

/* conv dgrad weight: wd[ci][tap][co] = w[co][k-1-tap][ci] */
int tt2_conv_weight_flip(const void* w, void* wd, int cout, int cin, int k, int dtype, hipStream_t stream);
/* The same flip for up to TT2_WFLIP_MAX conv layers in one launch (the backward flips every
 * encoder / post-net conv weight once per step). */
#define TT2_WFLIP_MAX 16
typedef struct tt2_wflip_job {
  const void* w; void* wd;
  int32_t cout, cin, k, pad_;
} tt2_wflip_job;
int tt2_conv_weight_flip_batch(const tt2_wflip_job* jobs, int32_t n, int32_t dtype, hipStream_t stream);

/* -------------------------------------------------------------- optimizer
 * Fused Adam(W) over the flat f32 parameter buffer with optional global-norm
 * clipping and Noam warmup (lr * d^-0.5 * min(s^-0.5, s*warmup^-1.5)); writes the
 * bf16 shadow used by the bf16 kernels.  step is a device counter (step+1 is used). */
typedef struct tt2_adam_args {
  float* params; const float* grads; float* exp_avg; float* exp_avg_sq;
  void* shadow_bf16;
  int32_t* step;
  void* workspace; size_t ws_bytes;
  int64_t n;
  float lr, beta1, beta2, eps, weight_decay, clip_norm, warmup;
  int32_t noam, d_model;
  /* clip: norm_parts != NULL gives the squared gradient norm as the sum of norm_nparts partial
   * sums the caller computed beforehand (tt2_sumsq_parts over ranges that cover grads[0, n)),
   * in place of the step's own pass over the gradients */
  const float* norm_parts;
  int32_t norm_nparts;
  /* gate != NULL: the update runs only while *gate != 0 (the pipelined optimizer's deferred
   * Adam: armed by tt2_adam_gate(op 1) when a step's gradients are final, consumed by
   * tt2_adam_gate(op 0) once the deferred update has run), so a captured step replays a
   * deferred update exactly once however often it was flushed eagerly in between */
  const int32_t* gate;
} tt2_adam_args;
size_t tt2_adam_workspace_size(void);
int tt2_adam_step(const tt2_adam_args* a, hipStream_t stream);
/* parts[0 .. nparts) = partial sums of g[i]^2 over g[0, n) (fixed split: reproducible); n == 0
 * writes zeros and g may then be NULL */
int tt2_sumsq_parts(const float* g, int64_t n, float* parts, int32_t nparts, hipStream_t stream);
/* step += 1; seed += 1 (either may be NULL: the pipelined optimizer bumps the dropout seed at the
 * end of a step and the step counter once the deferred Adam has run) */
int tt2_step_bump(int32_t* step, uint32_t* seed, hipStream_t stream);
/* op 1 (arm): *gate = 1.  op 0 (consume): if *gate != 0 { *step += 1 (when step != NULL); *gate = 0 } */
int tt2_adam_gate(int32_t* gate, int32_t* step, int32_t op, hipStream_t stream);

/* ---------------------------------------------------------- capture hygiene
 * For each of n streams, status[i] = 0: not part of the origin's capture, 1: part of it and
 * joined (the origin depends on all its captured work), 2: part of it with captured work the
 * origin does not depend on (ending the capture now would leave it unjoined), 3: its capture
 * was invalidated.  The origin stream must be capturing.  Host-only (reads the graph being
 * captured; enqueues nothing). */
int tt2_capture_joined(hipStream_t origin, const hipStream_t* streams, int32_t n, int32_t* status);

/* ---------------------------------------------------------- block-level entry points
 * One call per block of the path: each is a fixed sequence of the kernels
 * above on the caller's stream, with the block's shape and options in a tt2_desc.
 * Layout: activations channels-last [rows = batch * tq (or tk), channels] of desc.dtype
 * (TT2_DT_BF16 or TT2_DT_F32); weights of desc.dtype in nn.Linear layout [out][in]
 * (conv: [c_out][kernel][c_in], see tt2_conv_weight_pack); biases, LayerNorm / BatchNorm
 * parameters, statistics and every weight / bias gradient f32.  Weight and bias
 * gradients are written (not accumulated).
 *  - `saved`: activations a forward keeps for its backward, tt2_<block>_saved_size() bytes,
 *    written by _fwd and read by _bwd (the caller keeps it between them);
 *  - `workspace`: scratch of tt2_<block>_workspace_size() bytes (split-K slabs, partials),
 *    free again when the call's work has finished on the stream.
 * Dropout: p = desc.dropout at hash site desc.site (the FFN's second site is site + 1)
 * with seed *desc.seed, applied when desc.training is set. */
typedef struct tt2_desc {
  int32_t batch;          /* B */
  int32_t tq;             /* rows per utterance: query / sequence length */
  int32_t tk;             /* attention keys per utterance (cross: memory length; self: = tq) */
  int32_t d_model;        /* 512 (heads of width 64) */
  int32_t n_heads;
  int32_t d_ffn;
  int32_t c_in, c_out;    /* linear / conv1d_bn_act / heads channels (heads: c_out = n_mels + 1) */
  int32_t kernel;         /* conv taps (odd; "same" padding (kernel - 1) / 2) */
  int32_t dtype;          /* TT2_DT_BF16 or TT2_DT_F32 */
  int32_t causal;         /* attention: causal mask (self-attention) */
  int32_t cross;          /* attention: 1 = Q from x, K / V from mem (in_proj rows 0:d / d:3d) */
  int32_t act;            /* conv1d_bn_act: 0 none, 1 relu, 2 tanh */
  int32_t training;       /* dropout on; BatchNorm batch statistics + running-stat update */
  float eps;              /* LayerNorm / BatchNorm epsilon */
  float momentum;         /* BatchNorm running-stat momentum */
  float dropout;          /* p (0 = none) */
  const uint32_t* seed;   /* device dropout seed */
  uint32_t site;          /* dropout hash site */
  const int32_t* k_len;   /* [batch] valid keys per utterance (key padding mask) or NULL */
  const int32_t* mel_len; /* loss: [batch] valid frames */
  int32_t n_mels;         /* loss / heads: mel channels (80) */
  int32_t heads_ld;       /* heads / loss: row stride of the heads buffer (>= n_mels + 1) */
  float pos_weight;       /* loss: BCE positive weight */
  float grad_scale;       /* loss: multiplies every gradient (1 / world under data parallelism) */
} tt2_desc;

/* Attention sublayer (SURVEY 8(a) a3 / a6 / a7 + residual + post-LN):
 *   y = LN(x + drop(out_proj(SDPA(q = x Wq^T + bq, k|v = src Wkv^T + bkv))) ; src = cross ? mem : x
 * w_in [3d][d] (nn.MultiheadAttention in_proj), b_in [3d], w_out [d][d], b_out [d], ln_g / ln_b [d].
 * bwd: dy -> dx (residual + query path; + key/value path when not cross), dmem (cross: the
 * key/value path; NULL otherwise), and the parameter gradients. */
size_t tt2_attn_block_saved_size(const tt2_desc* d);
size_t tt2_attn_block_workspace_size(const tt2_desc* d);
int tt2_attn_block_fwd(const tt2_desc* d, const void* x, const void* mem, const void* w_in, const float* b_in,
                       const void* w_out, const float* b_out, const float* ln_g, const float* ln_b, void* y,
                       void* saved, void* workspace, size_t ws_bytes, hipStream_t stream);
int tt2_attn_block_bwd(const tt2_desc* d, const void* x, const void* mem, const void* w_in, const void* w_out,
                       const float* ln_g, const float* ln_b, const void* saved, const void* dy, void* dx, void* dmem,
                       float* dw_in, float* db_in, float* dw_out, float* db_out, float* dln_g, float* dln_b,
                       void* workspace, size_t ws_bytes, hipStream_t stream);

/* Position-wise FFN sublayer:
 *   y = LN(x + drop_{site+1}(drop_{site}(relu(x W1^T + b1)) W2^T + b2)),  w1 [d_ffn][d], w2 [d][d_ffn]. */
size_t tt2_ffn_saved_size(const tt2_desc* d);
size_t tt2_ffn_workspace_size(const tt2_desc* d);
int tt2_ffn_fwd(const tt2_desc* d, const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                const float* ln_g, const float* ln_b, void* y, void* saved, void* workspace, size_t ws_bytes,
                hipStream_t stream);
int tt2_ffn_bwd(const tt2_desc* d, const void* x, const void* w1, const void* w2, const float* ln_g,
                const float* ln_b, const void* saved, const void* dy, void* dx, float* dw1, float* db1, float* dw2,
                float* db2, float* dln_g, float* dln_b, void* workspace, size_t ws_bytes, hipStream_t stream);

/* Linear (pre-net / projections): y [rows][c_out] = x [rows][c_in] W^T + b (b may be NULL). */
size_t tt2_linear_workspace_size(const tt2_desc* d);
int tt2_linear_fwd(const tt2_desc* d, const void* x, const void* w, const float* b, void* y, void* workspace,
                   size_t ws_bytes, hipStream_t stream);
int tt2_linear_bwd(const tt2_desc* d, const void* x, const void* w, const void* dy, void* dx, float* dw, float* db,
                   void* workspace, size_t ws_bytes, hipStream_t stream);

/* Residual add + post-LayerNorm: y = LN(x + drop(branch)) over d_model channels; saved = mean / rstd.
 * bwd: dx = dL/d(x + drop(branch)), dbranch = drop'(dx), dln_g / dln_b. */
size_t tt2_add_ln_saved_size(const tt2_desc* d);
size_t tt2_add_ln_workspace_size(const tt2_desc* d);
int tt2_add_ln_fwd(const tt2_desc* d, const void* x, const void* branch, const float* ln_g, const float* ln_b,
                   void* y, void* saved, hipStream_t stream);
int tt2_add_ln_bwd(const tt2_desc* d, const void* x, const void* branch, const float* ln_g, const void* saved,
                   const void* dy, void* dx, void* dbranch, float* dln_g, float* dln_b, void* workspace,
                   size_t ws_bytes, hipStream_t stream);

/* Conv1d + BatchNorm + activation + dropout (SURVEY 8(a) a1 encoder pre-net, a9 post-net):
 *   out = drop(act(BN(conv(x) + b))) (+ res, [rows][c_out] of res_dtype, when res != NULL);
 * w [c_out][kernel][c_in]; BN over all rows (training: batch statistics, run_mean / run_var
 * updated; eval: the running statistics).  bwd: dout -> dx and dw / db / dbn_g / dbn_b. */
size_t tt2_conv1d_bn_act_saved_size(const tt2_desc* d);
size_t tt2_conv1d_bn_act_workspace_size(const tt2_desc* d);
int tt2_conv1d_bn_act_fwd(const tt2_desc* d, const void* x, const void* w, const float* b, const float* bn_g,
                          const float* bn_b, float* run_mean, float* run_var, const void* res, int32_t res_dtype,
                          void* out, void* saved, void* workspace, size_t ws_bytes, hipStream_t stream);
int tt2_conv1d_bn_act_bwd(const tt2_desc* d, const void* x, const void* w, const float* bn_g, const float* bn_b,
                          const void* saved, const void* dout, void* dx, float* dw, float* db, float* dbn_g,
                          float* dbn_b, void* workspace, size_t ws_bytes, hipStream_t stream);
/* nn.Conv1d weight [c_out][c_in][k] -> the blocks' tap-major [c_out][k][c_in] (same dtype) */
int tt2_conv_weight_pack(const void* w, void* wp, int32_t cout, int32_t cin, int32_t k, int32_t dtype,
                         hipStream_t stream);

/* Mel + stop heads: heads [rows][heads_ld] f32, cols 0..n_mels-1 = mel_before,
 * col n_mels = stop logit; w [n_mels + 1][d_model] (mel_linear rows, then stop_linear), b f32.
 * bwd: g_heads (f32, same layout) -> dx, dw, db. */
size_t tt2_heads_workspace_size(const tt2_desc* d);
int tt2_heads_fwd(const tt2_desc* d, const void* x, const void* w, const float* b, float* heads, void* workspace,
                  size_t ws_bytes, hipStream_t stream);
int tt2_heads_bwd(const tt2_desc* d, const void* x, const void* w, const float* g_heads, void* dx, float* dw,
                  float* db, void* workspace, size_t ws_bytes, hipStream_t stream);

/* Loss over rows = batch * tq: loss_out[4] = (total, mse_before, mse_after, bce);
 * bwd also writes g_heads (d/d mel_before in cols < n_mels, d/d stop logit in col n_mels) and
 * g_after (d/d mel_after, desc.dtype). */
size_t tt2_loss_block_workspace_size(const tt2_desc* d);
int tt2_loss_fwd(const tt2_desc* d, const float* heads, const float* mel_after, const float* target,
                 float* loss_out, void* workspace, size_t ws_bytes, hipStream_t stream);
int tt2_loss_bwd(const tt2_desc* d, const float* heads, const float* mel_after, const float* target,
                 float* loss_out, float* g_heads, void* g_after, void* workspace, size_t ws_bytes,
                 hipStream_t stream);

/* Data-parallel gradient bucket: in-place SUM all-reduce of n elements of
 * dtype over an RCCL communicator (ncclComm_t) on the caller's stream.  librccl is bound at
 * the first call (dlopen); the communicator helpers below wrap ncclGetUniqueId /
 * ncclCommInitRank / ncclCommDestroy for hosts without torch.distributed. */
int tt2_allreduce_bucket(void* buf, size_t n, int32_t dtype, void* comm, hipStream_t stream);
int tt2_comm_unique_id(void* id_out /* 128 bytes */);
int tt2_comm_init(void** comm_out, int32_t nranks, const void* id /* 128 bytes */, int32_t rank);
int tt2_comm_destroy(void* comm);
/* Measurement stand-in for one bucket's exchange at N ranks (tt2/dist.py StandinGradSync; the
 * DP schedule rehearsed on one GPU): `wgs` work groups copy `bytes` from src to scratch, then each
 * holds its CU until `seconds` have passed since it started.  No communicator; src is not modified.
 * rec (optional, 2 * wgs u64): each work group's {start, end} on the device wall clock. */
int tt2_comm_standin(const void* src, void* scratch, size_t bytes, double seconds, int32_t wgs, uint64_t* rec,
                     hipStream_t stream);

/* ------------------------------------------------------------ audio data path
 * Either side of the mel engine: log-mel extraction of the
 * training targets and Griffin-Lim inversion of synthesised mels.  The STFT, inverse DFT
 * and mel projections are tt2_gemm calls (f32) on window-folded bases; these are the
 * byte-moving steps around them (all f32, caller-owned buffers, caller's stream).
 * Frame layout: utterance b's padded signal is padded[b * Lp ...] with Lp a multiple of
 * hop, so the batch's frames are one strided matrix (row r at sample r * hop, ld = hop) and
 * utterance b owns rows [b * R, b * R + n_frames_b), R = Lp / hop.  Replaces the reference
 * pipeline's librosa / torch.stft feature extraction and its vocoder hand-off. */
/* Every entry below returns TT2_E_INVALID, with its own name in tt2_last_error(), before any launch
 * where a refusal is stated; nothing is written then.
 *
 * padded[b][j] = x[b][reflect(j - pad)] for j < len_b + 2 pad (np.pad "reflect"), else 0, for all
 * j < padded_len; x [batch][ldx], padded [batch][padded_len].  lens may be NULL (all len).  Ragged
 * rules: len_b = min(lens[b], len) (an entry above len counts as len); len_b <= 0 gives a row of
 * zeros and reads nothing; 0 < len_b <= pad is NOT np.pad's repeated reflection: s = j - pad is
 * reflected once about 0 (s < 0: -s), then once about len_b - 1 (s >= len_b: 2 (len_b - 1) - s),
 * then clamped into [0, len_b).  Samples at and beyond len_b are never read.
 * Refused: x or padded NULL; batch <= 0; len <= 0; pad < 0 or pad >= len;
 * padded_len < len + 2 pad; ldx < len when batch > 1. */
int tt2_reflect_pad(const float* x, int64_t ldx, const int32_t* lens, int32_t batch, int32_t len, float* padded,
                    int64_t padded_len, int32_t pad, hipStream_t stream);
/* mag[r][k] = |spec[r][k] + i spec[r][n_bins + k]| (k < n_bins), +0 in the padding columns
 * [n_bins, ld_mag), for r < m.  Columns of spec at and beyond 2 n_bins are never read.
 * Refused: spec or mag NULL; m <= 0; ld_spec < 2 n_bins; ld_mag < n_bins. */
int tt2_spec_magnitude(const float* spec, int64_t ld_spec, int32_t m, int32_t n_bins, float* mag, int64_t ld_mag,
                       hipStream_t stream);
/* out = mag * e / |e| as [re | im] rows, e = est[r][k] + i est[r][n_bins + k] (phase 0, that is
 * re = mag and im = +0 * mag, where est is NULL or e == 0): Griffin-Lim's projection onto the target
 * magnitude.  The padding columns [2 n_bins, ld_out) are set to +0; columns of mag at and beyond
 * n_bins and of est at and beyond 2 n_bins are never read.
 * Refused: mag or out NULL; m <= 0; ld_mag < n_bins; ld_out < 2 n_bins or ld_out > 3 n_bins;
 * ld_est < 2 n_bins when est is given. */
int tt2_spec_rephase(const float* mag, int64_t ld_mag, const float* est, int64_t ld_est, int32_t m, int32_t n_bins,
                     float* out, int64_t ld_out, hipStream_t stream);
/* y[b][t] = sum_f frames[b * R + f][t + n_fft/2 - f hop] / sum_f hann^2(t + n_fft/2 - f hop) for
 * t < len_b (least-squares iSTFT overlap-add, centre padding removed), over the frames
 * f < 1 + len_b / hop that cover the sample, hann the periodic Hann window of n_fft points; 0 where
 * the divisor is at most 1e-8, and 0 for len_b <= t < len.  R = rows_per_utt; y [batch][ld_y].
 * len_b = min(lens[b], len), lens NULL: all len; len_b <= 0 gives a row of zeros.  Frame rows at and
 * beyond 1 + len_b / hop of an utterance are never read.
 * Refused: frames or y NULL; batch <= 0; len <= 0; hop <= 0; n_fft < hop; ld_frames < n_fft;
 * rows_per_utt * hop < len + n_fft; ld_y < len when batch > 1. */
int tt2_overlap_add(const float* frames, int64_t ld_frames, const int32_t* lens, int32_t batch, int32_t len,
                    int32_t rows_per_utt, int32_t n_fft, int32_t hop, float* y, int64_t ld_y, hipStream_t stream);
/* scatter = 0: mel[b][t][c] = log(max(rows[b * R + t][c], clamp)) (t < frames_b, else log clamp),
 * for every row below the argument t; rows is only read;
 * scatter = 1: rows[b * R + t][c] = exp(mel[b][t][c]) (t < frames_b), +0 for every other row of the
 * utterance, frames_b <= t < R; mel is only read.  mel [batch][t][n_mels], R = rows_per_utt, c < n_mels
 * (columns [n_mels, ld_rows) of rows are neither read nor written).
 * frames_b = min(frames[b], t) (an entry above t counts as t; frames NULL: all t); frames[b] <= 0
 * makes the whole utterance silence (scatter = 0) or zero rows (scatter = 1).  Rows of the source at
 * and beyond frames_b are never read.
 * Refused: rows or mel NULL; batch <= 0; t <= 0; t > rows_per_utt; n_mels <= 0; ld_rows < n_mels;
 * clamp not > 0. */
int tt2_mel_rows(float* rows, int64_t ld_rows, float* mel, const int32_t* frames, int32_t batch, int32_t t,
                 int32_t n_mels, int32_t rows_per_utt, float clamp, int32_t scatter, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
