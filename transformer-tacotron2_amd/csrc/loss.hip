// loss.hip -- the fused TTS loss and its input gradients, HBM-bound (gfx950): masked MSE of
// mel_before and mel_after plus BCE(pos_weight) of the stop logit in one grid-stride pass,
// 16-B vectorised where the row width allows; deterministic (fixed-order partial sums, no
// float atomics).
#include <math.h>

#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {
constexpr int NT = 256;

// ------------------------------------------------------------------- loss
// heads [M, hld] f32: cols 0..79 mel_before, col 80 stop logit.  after [M, 80] f32.
// Writes: part[block][4] = (sum sq before, sum sq after, sum bce, 0);
//         g_heads[m, 0..79] = d/dbefore (direct + residual from after), g_heads[m, 80] = d/dstop,
//         g_heads[m, 81..hld) = 0; g_after[m, c] (T) = d/dafter.
template <typename T>
__global__ __launch_bounds__(NT) void loss_kernel(const float* heads, int64_t hld, const float* after,
                                                  const float* target, const int32_t* mel_len, int B, int Tlen,
                                                  int NM, float pos_weight, float gscale, float* g_heads, T* g_after, float* part,
                                                  int separate, int vec4) {
  __shared__ float red[3][NT / 64];
  int nvalid = 0;
  for (int b = 0; b < B; ++b) nvalid += min(max(mel_len[b], 0), Tlen);
  const float inv_n = nvalid > 0 ? gscale / nvalid : 0.f;
  const float inv_nm = inv_n / NM;
  const int M = B * Tlen;
  const int64_t total = vec4 ? 0 : (int64_t)M * hld;
  float sb = 0.f, sa = 0.f, ss = 0.f;
  if (vec4) {   // 4 columns per thread (hld, NM % 4 == 0, 16-B aligned rows): 32-bit indexing, vector loads
    const int cpr = (int)(hld >> 2), nchunk = M * cpr;
    for (int q = blockIdx.x * NT + threadIdx.x; q < nchunk; q += gridDim.x * NT) {
      const int m = q / cpr, c0 = (q - m * cpr) * 4;
      const int b = m / Tlen, t = m - b * Tlen;
      const int len = mel_len[b];
      const bool valid = t < len;
      const f32x4 hv = *reinterpret_cast<const f32x4*>(heads + (int64_t)m * hld + c0);
      f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c0 + 4 <= NM) {
        const int64_t j = (int64_t)m * NM + c0;
        const f32x4 tg = *reinterpret_cast<const f32x4*>(target + j), af = *reinterpret_cast<const f32x4*>(after + j);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float db = hv[k] - tg[k], da = af[k] - tg[k];
          float ga = 0.f;
          if (valid) {
            sb += db * db;
            sa += da * da;
            g[k] = 2.f * db * inv_nm;
            ga = 2.f * da * inv_nm;
          }
          g_after[j + k] = from_f32<T>(ga);
          if (!separate) g[k] += ga;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (c0 + k != NM || !valid) continue;
          const float x = hv[k];
          const float y = (t == len - 1) ? 1.f : 0.f;
          const float lsp = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
          const float lsn = fminf(-x, 0.f) - log1pf(expf(-fabsf(x)));
          ss += -(pos_weight * y * lsp + (1.f - y) * lsn);
          const float sg = 1.f / (1.f + expf(-x));
          g[k] = (pos_weight * y * (sg - 1.f) + (1.f - y) * sg) * inv_n;
        }
      }
      *reinterpret_cast<f32x4*>(g_heads + (int64_t)m * hld + c0) = g;
    }
  }
  for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int m = (int)(i / hld), c = (int)(i % hld);
    const int b = m / Tlen, t = m % Tlen;
    const int len = mel_len[b];
    const bool valid = t < len;
    float g = 0.f;
    if (c < NM) {
      const int64_t j = (int64_t)m * NM + c;
      const float db = heads[i] - target[j];
      const float da = after[j] - target[j];
      float ga = 0.f;
      if (valid) {
        sb += db * db;
        sa += da * da;
        g = 2.f * db * inv_nm;
        ga = 2.f * da * inv_nm;
      }
      g_after[j] = from_f32<T>(ga);
      if (!separate) g += ga;  // mel_after = mel_before + postnet(mel_before): residual path
    } else if (c == NM) {
      const float x = heads[i];
      const float y = (t == len - 1) ? 1.f : 0.f;
      if (valid) {
        // BCEWithLogits(pos_weight): l = -[pw*y*log s(x) + (1-y)*log(1-s(x))]
        const float lsp = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));   // log sigmoid(x)
        const float lsn = fminf(-x, 0.f) - log1pf(expf(-fabsf(x)));  // log sigmoid(-x)
        ss += -(pos_weight * y * lsp + (1.f - y) * lsn);
        const float sg = 1.f / (1.f + expf(-x));
        g = (pos_weight * y * (sg - 1.f) + (1.f - y) * sg) * inv_n;
      }
    }
    g_heads[i] = g;
  }
  sb = wave_sum(sb); sa = wave_sum(sa); ss = wave_sum(ss);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = sb; red[1][w] = sa; red[2][w] = ss; }
  __syncthreads();
  if (threadIdx.x < 3) {
    float t = 0.f;
    for (int k = 0; k < NT / 64; ++k) t += red[threadIdx.x][k];
    part[blockIdx.x * 4 + threadIdx.x] = t;
  }
}

// one wave: lane l sums partial rows l, l + 64, ... (loads issued together), then the 64 lane
// sums combine as a tree (wave_sum: a fixed order, reproducible, and 6 roundings where a serial
// sum in lane order had 64 -- that one put the BCE mean of 2048+ frames 2.5 ulp off)
__global__ void loss_finalize_kernel(const float* part, int nblocks, const int32_t* mel_len, int B, int Tlen, int NM,
                                     float* out) {
  const int l = threadIdx.x;
  float a[3] = {0.f, 0.f, 0.f};
  for (int i = l; i < nblocks; i += 64) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(part + i * 4);
    a[0] += v[0]; a[1] += v[1]; a[2] += v[2];
  }
  const float s[3] = {wave_sum(a[0]), wave_sum(a[1]), wave_sum(a[2])};
  if (l != 0) return;
  int nvalid = 0;
  for (int b = 0; b < B; ++b) nvalid += min(max(mel_len[b], 0), Tlen);
  const float n = nvalid > 0 ? (float)nvalid : 1.f;
  out[1] = s[0] / (n * NM);
  out[2] = s[1] / (n * NM);
  out[3] = s[2] / n;
  out[0] = out[1] + out[2] + out[3];
}

}  // namespace

extern "C" size_t tt2_loss_workspace_size(void) { return TT2_LOSS_BLOCKS * 4 * sizeof(float); }

extern "C" int tt2_tts_loss(const tt2_loss_args* p, hipStream_t s) {
  if (p->n_mels + 1 > p->heads_ld) return tt2_set_error(TT2_E_INVALID, "tt2_tts_loss: heads_ld too small");
  if (!p->workspace || p->ws_bytes < tt2_loss_workspace_size())
    return tt2_set_error(TT2_E_INVALID, "tt2_tts_loss: workspace");
  float* part = reinterpret_cast<float*>(p->workspace);
  auto al16 = [](const void* q) { return reinterpret_cast<uintptr_t>(q) % 16 == 0; };
  const int vec4 = p->heads_ld % 4 == 0 && p->n_mels % 4 == 0 && al16(p->heads) && al16(p->g_heads) &&
                   al16(p->mel_after) && al16(p->target);
  by_dtype(p->grad_dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(loss_kernel<T>, dim3(TT2_LOSS_BLOCKS), dim3(NT), 0, s, p->heads, p->heads_ld, p->mel_after,
                       p->target, p->mel_len, p->batch, p->t, p->n_mels, p->pos_weight, p->grad_scale, p->g_heads,
                       (T*)p->g_after, part, p->separate_grads, vec4);
  });
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, s, part, TT2_LOSS_BLOCKS, p->mel_len, p->batch,
                     p->t, p->n_mels, p->loss_out);
  return tt2_check_launch(hipGetLastError(), "tt2_tts_loss");
}
