// optim.hip -- the fused Adam/clip optimizer step, HBM-bound (gfx950): the gradient norm's
// partial sums of squares (ended by reduce.hip's kernel, a fixed order), clip + Adam(W) + Noam
// learning rate + bf16 shadow in one float4 grid-stride pass with nontemporal stores, and the
// one-thread step, seed and gate kernels of the captured step.
#include <math.h>

#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {
constexpr int NT = 256;

__global__ __launch_bounds__(NT) void sumsq_kernel(const float* g, int64_t n, float* part) {
  __shared__ float red[NT / 64];
  float s = 0.f;
  const int64_t n4 = n / 4;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
  for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * NT) {
    const f32x4 v = g4[i];
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) s += g[i] * g[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < NT / 64; ++w) t += red[w];
    part[blockIdx.x] = t;
  }
}

struct AdamArgs {
  float* p; const float* g; float* m; float* v; bf16* shadow;
  int64_t n;
  const float* sumsq;   // clip: global squared gradient norm (device scalar) or null
  int32_t* step;        // device step counter (read; bumped by tt2_step_bump)
  const int32_t* gate;  // null, or: update only while *gate != 0 (tt2_adam_gate)
  float lr, beta1, beta2, eps, wd, clip, warmup, d_model_rsqrt;
  int noam;
};

TT2_DEV void adam_one(const AdamArgs& a, int64_t i, float g, float lr, float step_size, float bc2_sqrt) {
  float p = a.p[i];
  if (a.wd != 0.f) p -= lr * a.wd * p;  // decoupled (AdamW) weight decay
  const float m = a.beta1 * a.m[i] + (1.f - a.beta1) * g;
  const float v = a.beta2 * a.v[i] + (1.f - a.beta2) * g * g;
  a.m[i] = m;
  a.v[i] = v;
  p -= step_size * m / (sqrtf(v) / bc2_sqrt + a.eps);
  a.p[i] = p;
  if (a.shadow) a.shadow[i] = (bf16)p;
}

// one thread updates 4 consecutive parameters (n is a multiple of 16: slots are 16-aligned)
__global__ __launch_bounds__(NT) void adam_kernel(AdamArgs a) {
  if (a.gate && *a.gate == 0) return;   // a deferred update that already ran (or none pending)
  const int step = *a.step + 1;
  float scale = 1.f;
  if (a.clip > 0.f && a.sumsq) {
    const float nrm = sqrtf(*a.sumsq);
    if (nrm > a.clip) scale = a.clip / (nrm + 1e-6f);
  }
  float lr = a.lr;
  if (a.noam) lr = a.lr * a.d_model_rsqrt * fminf(rsqrtf((float)step), step * powf(a.warmup, -1.5f));
  const float bc1 = 1.f - powf(a.beta1, (float)step);
  const float bc2 = 1.f - powf(a.beta2, (float)step);
  const float step_size = lr / bc1;
  const float bc2_sqrt = sqrtf(bc2);
  const int64_t n4 = a.n / 4;
  for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * NT) {
    const f32x4 g = reinterpret_cast<const f32x4*>(a.g)[i];
    const f32x4 p = reinterpret_cast<const f32x4*>(a.p)[i];
    const f32x4 m = reinterpret_cast<const f32x4*>(a.m)[i];
    const f32x4 v = reinterpret_cast<const f32x4*>(a.v)[i];
    f32x4 po, mo, vo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gj = g[j] * scale;
      float pj = p[j];
      if (a.wd != 0.f) pj -= lr * a.wd * pj;
      mo[j] = a.beta1 * m[j] + (1.f - a.beta1) * gj;
      vo[j] = a.beta2 * v[j] + (1.f - a.beta2) * gj * gj;
      po[j] = pj - step_size * mo[j] / (sqrtf(vo[j]) / bc2_sqrt + a.eps);
    }
    // nontemporal: every lane's 16 B (8 B for the shadow) continue its neighbours' into
    // whole lines, which stream to memory instead of being written back at the kernel's end
    __builtin_nontemporal_store(po, reinterpret_cast<f32x4*>(a.p) + i);
    __builtin_nontemporal_store(mo, reinterpret_cast<f32x4*>(a.m) + i);
    __builtin_nontemporal_store(vo, reinterpret_cast<f32x4*>(a.v) + i);
    if (a.shadow) {
      typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      bf16x4 sh;
#pragma unroll
      for (int j = 0; j < 4; ++j) sh[j] = (bf16)po[j];
      __builtin_nontemporal_store(*reinterpret_cast<const u32x2*>(&sh), reinterpret_cast<u32x2*>(a.shadow) + i);
    }
  }
  for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)NT + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * NT)
    adam_one(a, i, a.g[i] * scale, lr, step_size, bc2_sqrt);
}

__global__ void step_bump_kernel(int32_t* step, uint32_t* seed) {
  if (threadIdx.x == 0) {
    if (step) step[0] += 1;
    if (seed) seed[0] += 1u;
  }
}

__global__ void adam_gate_kernel(int32_t* gate, int32_t* step, int op) {
  if (threadIdx.x == 0) {
    if (op == 1) {
      gate[0] = 1;
    } else if (gate[0] != 0) {
      if (step) step[0] += 1;
      gate[0] = 0;
    }
  }
}

}  // namespace

extern "C" size_t tt2_adam_workspace_size(void) { return (TT2_ADAM_NORM_BLOCKS + 16) * sizeof(float); }

extern "C" int tt2_adam_step(const tt2_adam_args* p, hipStream_t s) {
  AdamArgs a{};
  a.p = p->params; a.g = p->grads; a.m = p->exp_avg; a.v = p->exp_avg_sq; a.shadow = (bf16*)p->shadow_bf16;
  a.n = p->n; a.step = p->step; a.gate = p->gate;
  a.lr = p->lr; a.beta1 = p->beta1; a.beta2 = p->beta2; a.eps = p->eps; a.wd = p->weight_decay;
  a.clip = p->clip_norm; a.warmup = p->warmup; a.noam = p->noam;
  a.d_model_rsqrt = p->d_model > 0 ? 1.f / sqrtf((float)p->d_model) : 1.f;
  if ((reinterpret_cast<uintptr_t>(p->params) | reinterpret_cast<uintptr_t>(p->grads) |
       reinterpret_cast<uintptr_t>(p->exp_avg) | reinterpret_cast<uintptr_t>(p->exp_avg_sq)) % 16 ||
      reinterpret_cast<uintptr_t>(p->shadow_bf16) % 8)
    return tt2_set_error(TT2_E_INVALID, "tt2_adam_step: buffers must be 16-B aligned");
  if (p->clip_norm > 0.f) {
    if (!p->workspace || p->ws_bytes < tt2_adam_workspace_size())
      return tt2_set_error(TT2_E_INVALID, "tt2_adam_step: workspace");
    if (p->norm_parts && p->norm_nparts <= 0) return tt2_set_error(TT2_E_INVALID, "tt2_adam_step: norm_nparts");
    float* part = reinterpret_cast<float*>(p->workspace);
    float* total = part + TT2_ADAM_NORM_BLOCKS;
    if (!p->norm_parts)
      hipLaunchKernelGGL(sumsq_kernel, dim3(TT2_ADAM_NORM_BLOCKS), dim3(NT), 0, s, p->grads, p->n, part);
    tt2_launch_reduce_rows(p->norm_parts ? p->norm_parts : part, p->norm_parts ? p->norm_nparts : TT2_ADAM_NORM_BLOCKS,
                           1, 1, total, 0.f, s, 1);
    a.sumsq = total;
  }
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(p->n / 4)), dim3(NT), 0, s, a);
  return tt2_check_launch(hipGetLastError(), "tt2_adam_step");
}

extern "C" int tt2_sumsq_parts(const float* g, int64_t n, float* parts, int32_t nparts, hipStream_t s) {
  if ((!g && n > 0) || !parts || nparts <= 0 || n < 0 || (reinterpret_cast<uintptr_t>(g) % 16))   // n == 0: g unread
    return tt2_set_error(TT2_E_INVALID, "tt2_sumsq_parts: g 16-B aligned, parts, nparts > 0");
  hipLaunchKernelGGL(sumsq_kernel, dim3(nparts), dim3(NT), 0, s, g, n, parts);
  return tt2_check_launch(hipGetLastError(), "tt2_sumsq_parts");
}

extern "C" int tt2_adam_gate(int32_t* gate, int32_t* step, int32_t op, hipStream_t s) {
  if (!gate || (op != 0 && op != 1)) return tt2_set_error(TT2_E_INVALID, "tt2_adam_gate: gate, op 0 or 1");
  hipLaunchKernelGGL(adam_gate_kernel, dim3(1), dim3(64), 0, s, gate, step, (int)op);
  return tt2_check_launch(hipGetLastError(), "tt2_adam_gate");
}

extern "C" int tt2_step_bump(int32_t* step, uint32_t* seed, hipStream_t s) {
  if (!step && !seed) return TT2_OK;
  hipLaunchKernelGGL(step_bump_kernel, dim3(1), dim3(64), 0, s, step, seed);
  return tt2_check_launch(hipGetLastError(), "tt2_step_bump");
}
