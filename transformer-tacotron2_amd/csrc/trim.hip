// trim.hip -- leading / trailing silence trimming of a batch of utterances (tt2_trim).  tt2_capi.h
// states the definition.  A translation unit of its own: no other kernel's code depends on it.
//
// Three launches on one stream, no host synchronisation:
//   trim_block_energy   one wave per block of `hop` samples: sum of x^2, to the workspace
//   trim_decide         one work group per utterance: frame energies from 2r block sums, emax,
//                       the lowest and highest loud frame, start / out to the workspace and outputs
//   trim_copy           y[b][i] = x[b][start_b + i], zeros past out_b
// The workspace is [batch][2] int32 (start, out), padded to 16 bytes, then the block sums
// [batch][nb] f32, nb = ceil(n_in / hop).  (Measured on an MI355X at B = 16 x 204 544, hop 512: these
// three launches 14.1 us; two launches, every work group of the copy redoing the decision from L2,
// 17.9 us.  DESIGN.md 5.11.)
#include <limits.h>

#include <algorithm>
#include <cmath>

#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_WAVES = TR_THREADS / 64;
constexpr int TR_ECHUNKS = 1024;   // energy pass: work groups per utterance at most (4 blocks each per trip)
constexpr int TR_CCOLS = 4 * TR_THREADS;   // copy: columns of a work group per trip
constexpr int TR_CCHUNKS = 256;    // copy: work groups per utterance at most

struct tr_plan {
  int nb, nf;          // block sums and frame energies (n_in / hop + 1) per utterance
  int ech, cch;        // work groups per utterance of the energy pass and of the copy
  int32_t* meta;       // [batch][2]: start, out
  float* bsum;         // [batch][nb]
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

TT2_DEV int tr_len(const tt2_trim_args& a, int b) {
  const int len = a.lens ? a.lens[b] : a.n_in;
  return min(max(len, 0), a.n_in);
}

// acc + x * x with the square rounded to f32 first: the definition's "sum of squares", not an fma
TT2_DEV float tr_sq_add(float acc, float x) { return __fadd_rn(acc, __fmul_rn(x, x)); }

// Block j of utterance b, samples [j * hop, j * hop + n), n = min(hop, len_b - j * hop), by one
// wave.  Sample i of the block belongs to lane (i / 4) % 64; a lane adds the squares of its samples
// to one accumulator from +0 with i ascending, and wave_sum's fixed tree adds the 64 accumulators:
// the order is a function of n alone.  Where the block starts on a 16-byte boundary a lane's four
// samples come as one load, otherwise as four; the arithmetic is the same.
__global__ __launch_bounds__(TR_THREADS) void trim_block_energy(tt2_trim_args a, tr_plan pl) {
  const int b = blockIdx.x / (unsigned)pl.ech;
  const int c = blockIdx.x % (unsigned)pl.ech;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int len = tr_len(a, b);
  const int nblk = (int)(((int64_t)len + a.hop - 1) / a.hop);
  const float* xrow = a.x + (int64_t)b * a.x_ld;
  float* out = pl.bsum + (int64_t)b * pl.nb;
  for (int64_t j = (int64_t)c * TR_WAVES + w; j < nblk; j += (int64_t)pl.ech * TR_WAVES) {
    const int64_t s0 = j * a.hop;
    const int n = (int)min((int64_t)a.hop, (int64_t)len - s0);
    const float* p = xrow + s0;
    const bool vec = (reinterpret_cast<uintptr_t>(p) & 15) == 0;   // wave-uniform
    float acc = 0.f;
    for (int i = 4 * lane; i < n; i += 256) {
      if (i + 4 <= n) {
        f32x4 v;
        if (vec) {
          v = *reinterpret_cast<const f32x4*>(p + i);
        } else {
          v.x = p[i], v.y = p[i + 1], v.z = p[i + 2], v.w = p[i + 3];
        }
        acc = tr_sq_add(tr_sq_add(tr_sq_add(tr_sq_add(acc, v.x), v.y), v.z), v.w);
      } else {
        for (int k = i; k < n; ++k) acc = tr_sq_add(acc, p[k]);
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) out[j] = acc;
  }
}

// Work-group reductions of trim_decide over LDS (the result in every thread)
TT2_DEV float tr_group_max(float v, float* s) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
}
TT2_DEV int tr_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
TT2_DEV int tr_group_min(int v, int* s) {
  v = tr_wave_min(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  return min(min(s[0], s[1]), min(s[2], s[3]));
}

// The decision for utterance b by one work group: frame energies from 2 r adjacent block sums, emax,
// the lowest and highest loud frame.  A frame energy is computed twice (for emax, then for the
// compare) from the same block sums in the same order, so both passes see the same bits.
__global__ __launch_bounds__(TR_THREADS) void trim_decide(tt2_trim_args a, tr_plan pl) {
  __shared__ float sf[TR_WAVES];
  __shared__ int si[TR_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = tr_len(a, b);
  const int nblk = (int)(((int64_t)len + a.hop - 1) / a.hop);
  const int F = len ? 1 + len / a.hop : 0;
  const float* bs = pl.bsum + (int64_t)b * pl.nb;
  float* erow = a.energy ? a.energy + (int64_t)b * a.energy_ld : nullptr;
  auto energy = [&](int f) {
    float e = 0.f;
    for (int j = f - a.r; j < f + a.r; ++j) e = __fadd_rn(e, (j >= 0 && j < nblk) ? bs[j] : 0.f);
    return e;
  };
  float emax = 0.f;                                     // energies are sums of squares: >= 0
  for (int f = tid; f < (erow ? pl.nf : F); f += TR_THREADS) {
    const float e = f < F ? energy(f) : 0.f;
    emax = fmaxf(emax, e);
    if (erow) erow[f] = e;
  }
  emax = tr_group_max(emax, sf);
  const float thr = __fmul_rn(a.ratio, emax);
  int f0 = INT_MAX, f1n = INT_MAX;                      // f1n = -f1: one kind of reduction
  for (int f = tid; f < F; f += TR_THREADS) {
    if (energy(f) > thr) f0 = min(f0, f), f1n = min(f1n, -f);
  }
  f0 = tr_group_min(f0, si);
  f1n = tr_group_min(f1n, si);
  if (tid == 0) {
    int64_t start = 0, end = 0;
    if (f0 != INT_MAX) {
      start = max((int64_t)0, (int64_t)f0 * a.hop - a.keep);
      end = min((int64_t)len, ((int64_t)(-f1n) + 1) * a.hop + a.keep);
    }
    const int outb = (int)min(end - start, (int64_t)a.n_out);
    pl.meta[2 * (int64_t)b] = (int)start;
    pl.meta[2 * (int64_t)b + 1] = outb;
    if (a.start) a.start[b] = (int)start;
    if (a.out_lens) a.out_lens[b] = outb;
  }
}

// Columns are handled in groups of four that sit on 16-byte boundaries of y's row (group g holds
// columns 4 g - m .. 4 g - m + 3, m the row's misalignment in floats): a whole group inside
// [0, n_out) is one 16-byte store.  The source x + start_b is wherever the decision put it: one
// 16-byte load where it happens to be aligned too, four dword loads otherwise.
__global__ __launch_bounds__(TR_THREADS) void trim_copy(tt2_trim_args a, tr_plan pl) {
  const int b = blockIdx.x / (unsigned)pl.cch;
  const int c = blockIdx.x % (unsigned)pl.cch;
  const int start = pl.meta[2 * (int64_t)b], outb = pl.meta[2 * (int64_t)b + 1];
  const float* src = a.x + (int64_t)b * a.x_ld + start;
  float* yrow = a.y + (int64_t)b * a.y_ld;
  const int m = (int)((reinterpret_cast<uintptr_t>(yrow) >> 2) & 3);
  const bool vec = ((reinterpret_cast<uintptr_t>(src) >> 2) & 3) == (unsigned)m;   // src - m is aligned with y - m
  const int64_t ngroups = ((int64_t)a.n_out + m + 3) / 4;
  for (int64_t g = (int64_t)c * TR_THREADS + threadIdx.x; g < ngroups; g += (int64_t)pl.cch * TR_THREADS) {
    const int64_t i0 = 4 * g - m;
    if (i0 >= 0 && i0 + 4 <= a.n_out) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (i0 + 4 <= outb) {
        if (vec) {
          v = *reinterpret_cast<const f32x4*>(src + i0);
        } else {
          v.x = src[i0], v.y = src[i0 + 1], v.z = src[i0 + 2], v.w = src[i0 + 3];
        }
      } else if (i0 < outb) {
        v.x = src[i0];
        if (i0 + 1 < outb) v.y = src[i0 + 1];
        if (i0 + 2 < outb) v.z = src[i0 + 2];
      }
      *reinterpret_cast<f32x4*>(yrow + i0) = v;
    } else {
      for (int64_t i = max(i0, (int64_t)0); i < min(i0 + 4, (int64_t)a.n_out); ++i) yrow[i] = i < outb ? src[i] : 0.f;
    }
  }
}

int tr_err(const char* msg) { return tt2_invalid("tt2_trim", msg); }

size_t tr_meta_bytes(int64_t batch) { return ((size_t)batch * 2 * sizeof(int32_t) + 15) & ~(size_t)15; }
}  // namespace

extern "C" size_t tt2_trim_workspace_size(int batch, int n_in, int hop) {
  if (batch <= 0 || n_in < 0 || hop < 1) return 0;
  const size_t nb = ((size_t)n_in + hop - 1) / hop;
  return tr_meta_bytes(batch) + (size_t)batch * nb * sizeof(float);
}

extern "C" int tt2_trim(const tt2_trim_args* p, hipStream_t s) {
  if (!p) return tr_err("args required");
  if (p->hop < 1) return tr_err("hop < 1");
  if (p->r < 1 || p->r > TT2_TRIM_MAX_R) return tr_err("r outside 1 .. TT2_TRIM_MAX_R");
  if (2 * (int64_t)p->r * p->hop > INT_MAX) return tr_err("the frame length 2 * r * hop overflows int32");
  if (p->keep < 0) return tr_err("keep < 0");
  if (!std::isfinite(p->ratio) || p->ratio < 0.f || p->ratio > 1.f) return tr_err("ratio must be finite and in [0, 1]");
  if (p->batch < 0 || p->n_in < 0 || p->n_out < 0) return tr_err("negative batch / n_in / n_out");
  if (p->x_ld < p->n_in || p->y_ld < p->n_out) return tr_err("x_ld < n_in or y_ld < n_out");
  tr_plan pl;
  pl.nb = (int)(((int64_t)p->n_in + p->hop - 1) / p->hop);
  pl.nf = p->n_in / p->hop + 1;
  if (p->energy && p->energy_ld < pl.nf) return tr_err("energy_ld < n_in / hop + 1");
  if (!p->y) return tr_err("y required");
  const size_t need = tt2_trim_workspace_size(p->batch, p->n_in, p->hop);
  if (need && (!p->workspace || p->workspace_bytes < need)) return tr_err("workspace below tt2_trim_workspace_size");
  pl.ech = std::max(1, std::min(TR_ECHUNKS, (pl.nb + TR_WAVES - 1) / TR_WAVES));
  pl.cch = std::max(1, (int)std::min<int64_t>(TR_CCHUNKS, ((int64_t)p->n_out + 3 + TR_CCOLS - 1) / TR_CCOLS));
  if ((int64_t)p->batch * std::max(pl.ech, pl.cch) > INT_MAX) return tr_err("more than 2^31 - 1 work groups");
  if (p->batch == 0 || p->n_out == 0) return TT2_OK;
  if (!p->x && p->n_in > 0) return tr_err("x required");
  char* ws = static_cast<char*>(p->workspace);
  pl.meta = reinterpret_cast<int32_t*>(ws);
  pl.bsum = reinterpret_cast<float*>(ws + tr_meta_bytes(p->batch));
  if (pl.nb > 0) {
    hipLaunchKernelGGL(trim_block_energy, dim3((unsigned)(p->batch * pl.ech)), dim3(TR_THREADS), 0, s, *p, pl);
    const int rc = tt2_check_launch(hipGetLastError(), "tt2_trim (block energies)");
    if (rc != TT2_OK) return rc;
  }
  hipLaunchKernelGGL(trim_decide, dim3((unsigned)p->batch), dim3(TR_THREADS), 0, s, *p, pl);
  const int rc = tt2_check_launch(hipGetLastError(), "tt2_trim (decision)");
  if (rc != TT2_OK) return rc;
  hipLaunchKernelGGL(trim_copy, dim3((unsigned)(p->batch * pl.cch)), dim3(TR_THREADS), 0, s, *p, pl);
  return tt2_check_launch(hipGetLastError(), "tt2_trim (copy)");
}
