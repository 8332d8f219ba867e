// embed.hip -- the model's input side, HBM-bound (gfx950): embedding forward and backward,
// scaled positional encoding with dropout, forward and backward, and the teacher-forcing
// shift of the decoder input.  Grid-stride, 16-B vectorised where the row width allows,
// deterministic: the embedding backward is a gather in row order (no float atomics), dalpha a
// fixed-order sum of per-work-group partials (reduce.hip's kernel).
#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {
constexpr int NT = 256;

// ------------------------------------------------------------ embedding
template <typename T>
__global__ void embed_fwd_kernel(const int64_t* ids, const T* table, T* out, int M, int C, int V) {
  const int64_t total = (int64_t)M * C;
  for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int m = (int)(i / C), c = (int)(i % C);
    const int64_t id = ids[m];
    out[i] = (id >= 0 && id < V) ? table[id * C + c] : from_f32<T>(0.f);
  }
}

// Gather form, deterministic (no atomics): workgroup (v, column block of 512) writes table row
// v's gradient = sum over the rows m with ids[m] == v of dout[m], added in increasing m (the same
// bits every run, whatever the collisions).  The ids are taken in chunks of EB_CHUNK rows: each
// of the 8 waves ballots its slice of the chunk, the matching rows are compacted into an LDS
// list in row order (wave offsets from the per-wave counts), then every thread adds its column of
// those rows with EB_UNROLL loads in flight.  Rows == pad_idx (and out-of-range ids) get no
// gradient; every table row is written, not accumulated.
constexpr int EB_NT = 512, EB_CHUNK = 4096, EB_UNROLL = 8;
template <typename T>
__global__ __launch_bounds__(EB_NT) void embed_bwd_kernel(const int64_t* ids, const T* dout, float* dtable, int M,
                                                          int C, int V, int pad_idx) {
  __shared__ int list[EB_CHUNK];
  __shared__ int wcnt[EB_NT / 64];
  const int v = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.y * EB_NT + threadIdx.x;
  constexpr int PERW = EB_CHUNK / (EB_NT / 64);   // rows per wave per chunk
  float acc = 0.f;
  if (v != pad_idx) {
    for (int base = 0; base < M; base += EB_CHUNK) {
      const int r0 = base + w * PERW;
      uint64_t masks[PERW / 64];
      int n = 0;
#pragma unroll
      for (int i = 0; i < PERW / 64; ++i) {
        const int m = r0 + 64 * i + lane;
        masks[i] = __ballot(m < M && ids[m] == (int64_t)v);
        n += __builtin_popcountll(masks[i]);
      }
      if (lane == 0) wcnt[w] = n;
      __syncthreads();
      int off = 0, total = 0;
#pragma unroll
      for (int k = 0; k < EB_NT / 64; ++k) {
        off += k < w ? wcnt[k] : 0;
        total += wcnt[k];
      }
#pragma unroll
      for (int i = 0; i < PERW / 64; ++i) {
        const uint64_t below = lane ? (masks[i] & (~0ull >> (64 - lane))) : 0ull;
        if ((masks[i] >> lane) & 1ull) list[off + __builtin_popcountll(below)] = r0 + 64 * i + lane;
        off += __builtin_popcountll(masks[i]);
      }
      __syncthreads();
      if (c < C) {
        int i = 0;
        for (; i + EB_UNROLL <= total; i += EB_UNROLL) {
          float x[EB_UNROLL];
#pragma unroll
          for (int u = 0; u < EB_UNROLL; ++u) x[u] = to_f32(dout[(int64_t)list[i + u] * C + c]);
#pragma unroll
          for (int u = 0; u < EB_UNROLL; ++u) acc += x[u];
        }
        for (; i < total; ++i) acc += to_f32(dout[(int64_t)list[i] * C + c]);
      }
      __syncthreads();   // the list is rebuilt for the next chunk
    }
  }
  if (c < C) dtable[(int64_t)v * C + c] = acc;
}

// ------------------------------------------------------ positional encoding
// out = drop(x + alpha * pe[t]),  t = row % T
template <typename T>
__global__ void pe_fwd_kernel(const T* x, const float* alpha, const float* pe, T* out, int M, int C, int Tlen,
                              int t_off, const int32_t* t_ptr, DropDesc drop) {
  const int64_t total = (int64_t)M * C;
  const float al = *alpha;
  if (t_ptr) t_off += *t_ptr;
  const uint32_t seed = drop.thr ? *drop.seed : 0u;
  for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int m = (int)(i / C), c = (int)(i % C);
    const int t = m % Tlen + t_off;
    float v = to_f32(x[i]) + al * pe[(int64_t)t * C + c];
    if (drop.thr) v = drop_apply(drop, seed, (uint32_t)i, v);
    out[i] = from_f32<T>(v);
  }
}
// 8 elements per thread (C % 8 == 0, bf16 / f32): 16-B loads, 32-bit chunk indexing, the
// dropout bits of the chunk from drop_bits8, nontemporal stores
template <typename T>
__global__ __launch_bounds__(NT) void pe_fwd8_kernel(const T* x, const float* alpha, const float* pe, T* out, int M,
                                                     int C, int Tlen, int t_off, const int32_t* t_ptr, DropDesc drop) {
  const int cpr = C >> 3, nchunk = M * cpr;
  const float al = *alpha;
  if (t_ptr) t_off += *t_ptr;
  const uint32_t seed = drop.thr ? *drop.seed : 0u;
  for (int q = blockIdx.x * NT + threadIdx.x; q < nchunk; q += gridDim.x * NT) {
    const int m = q / cpr, c0 = (q - m * cpr) * 8, t = m % Tlen + t_off;
    const uint32_t i0 = (uint32_t)m * C + c0;
    float v[8];
    if constexpr (sizeof(T) == 2) {
      const bf16x8 xv = *reinterpret_cast<const bf16x8*>(x + i0);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (float)xv[j];
    } else {
      const f32x4 a = *reinterpret_cast<const f32x4*>(x + i0), b = *reinterpret_cast<const f32x4*>(x + i0 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
    }
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(pe + (int64_t)t * C + c0);
    const f32x4 p1 = *reinterpret_cast<const f32x4*>(pe + (int64_t)t * C + c0 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] += al * p0[j]; v[4 + j] += al * p1[j]; }
    if (drop.thr) drop_apply8(drop, seed, i0, v);
    if constexpr (sizeof(T) == 2) {
      bf16 o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (bf16)v[j];
      __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(o), reinterpret_cast<u32x4*>(out + i0));
    } else {
      __builtin_nontemporal_store(f32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4*>(out + i0));
      __builtin_nontemporal_store(f32x4{v[4], v[5], v[6], v[7]}, reinterpret_cast<f32x4*>(out + i0) + 1);
    }
  }
}

// dx = drop'(dout); part[block] = sum dx * pe
// dx = drop(dout) and a per-block partial of dalpha = sum(dx * pe[t]).  8-element
// chunks (C % 8 == 0): 16-B loads, 32-bit chunk indexing.
template <typename T>
__global__ __launch_bounds__(NT) void pe_bwd_kernel(const T* dout, const float* pe, T* dx, float* part, int M, int C,
                                                    int Tlen, DropDesc drop) {
  __shared__ float red[NT / 64];
  const int cpr = C >> 3, nchunk = M * cpr;
  const uint32_t seed = drop.thr ? *drop.seed : 0u;
  float s = 0.f;
  for (int q = blockIdx.x * NT + threadIdx.x; q < nchunk; q += gridDim.x * NT) {
    const int m = q / cpr, c0 = (q - m * cpr) * 8;
    const int t = m % Tlen;
    const int64_t i0 = (int64_t)m * C + c0;
    float g[8];
    if constexpr (sizeof(T) == 2) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(dout + i0);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = (float)v[j];
    } else {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(dout + i0), hi = *reinterpret_cast<const f32x4*>(dout + i0 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { g[j] = lo[j]; g[4 + j] = hi[j]; }
    }
    if (drop.thr) drop_apply8(drop, seed, (uint32_t)i0, g);
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(pe + (int64_t)t * C + c0);
    const f32x4 p1 = *reinterpret_cast<const f32x4*>(pe + (int64_t)t * C + c0 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) s += g[j] * p0[j] + g[4 + j] * p1[j];
    if constexpr (sizeof(T) == 2) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (bf16)g[j];
      *reinterpret_cast<bf16x8*>(dx + i0) = o;
    } else {
      *reinterpret_cast<f32x4*>(dx + i0) = f32x4{g[0], g[1], g[2], g[3]};
      *reinterpret_cast<f32x4*>(dx + i0 + 4) = f32x4{g[4], g[5], g[6], g[7]};
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < NT / 64; ++w) t += red[w];
    part[blockIdx.x] = t;
  }
}

// ------------------------------------------------------ teacher forcing input
// out[b*T + t, c] = t == 0 ? 0 : mel[b, t-1, c]
template <typename T>
__global__ void shift_right_kernel(const float* mel, T* out, int B, int Tlen, int C) {
  const int64_t total = (int64_t)B * Tlen * C;
  for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t m = i / C;
    const int t = (int)(m % Tlen);
    out[i] = from_f32<T>(t == 0 ? 0.f : mel[i - C]);
  }
}

}  // namespace

extern "C" int tt2_embedding_fwd(const int64_t* ids, const void* table, void* out, int m, int c, int vocab,
                                 int dtype, hipStream_t s) {
  const int g = grid_for((int64_t)m * c);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(embed_fwd_kernel<T>, dim3(g), dim3(NT), 0, s, ids, (const T*)table, (T*)out, m, c, vocab);
  });
  return tt2_check_launch(hipGetLastError(), "tt2_embedding_fwd");
}

extern "C" int tt2_embedding_bwd(const int64_t* ids, const void* dout, float* dtable, int m, int c, int vocab,
                                 int pad_idx, int dtype, hipStream_t s) {
  if (vocab <= 0 || c <= 0) return TT2_OK;
  const dim3 g(vocab, (c + EB_NT - 1) / EB_NT);   // every table row written: no memset
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(embed_bwd_kernel<T>, g, dim3(EB_NT), 0, s, ids, (const T*)dout, dtable, m, c, vocab, pad_idx);
  });
  return tt2_check_launch(hipGetLastError(), "tt2_embedding_bwd");
}

extern "C" int tt2_posenc_fwd(const tt2_pe_args* p, hipStream_t s) {
  const DropDesc d = drop_of(p);
  const bool v8 = p->c % 8 == 0 && (int64_t)p->m * p->c < (1ll << 31) &&
                  reinterpret_cast<uintptr_t>(p->x) % 16 == 0 && reinterpret_cast<uintptr_t>(p->out) % 16 == 0;
  const int g = grid_for(v8 ? (int64_t)p->m * p->c / 8 : (int64_t)p->m * p->c);
  by_dtype(p->dtype, [&](auto t) {
    using T = decltype(t);
    if (v8)
      hipLaunchKernelGGL(pe_fwd8_kernel<T>, dim3(g), dim3(NT), 0, s, (const T*)p->x, p->alpha, p->pe, (T*)p->out, p->m,
                         p->c, p->t, p->t_offset, p->t_ptr, d);
    else
      hipLaunchKernelGGL(pe_fwd_kernel<T>, dim3(g), dim3(NT), 0, s, (const T*)p->x, p->alpha, p->pe, (T*)p->out, p->m,
                         p->c, p->t, p->t_offset, p->t_ptr, d);
  });
  return tt2_check_launch(hipGetLastError(), "tt2_posenc_fwd");
}

extern "C" size_t tt2_posenc_bwd_workspace_size(void) { return TT2_PE_BWD_BLOCKS * sizeof(float); }

extern "C" int tt2_posenc_bwd(const tt2_pe_args* p, hipStream_t s) {
  if (!p->workspace || p->ws_bytes < tt2_posenc_bwd_workspace_size())
    return tt2_set_error(TT2_E_INVALID, "tt2_posenc_bwd: workspace");
  if (p->c % 8 || (int64_t)p->m * p->c >= (1ll << 31))
    return tt2_set_error(TT2_E_INVALID, "tt2_posenc_bwd: C must be a multiple of 8 and M*C < 2^31");
  const DropDesc d = drop_of(p);
  float* part = reinterpret_cast<float*>(p->workspace);
  by_dtype(p->dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(pe_bwd_kernel<T>, dim3(TT2_PE_BWD_BLOCKS), dim3(NT), 0, s, (const T*)p->dout, p->pe, (T*)p->dx,
                       part, p->m, p->c, p->t, d);
  });
  tt2_launch_reduce_rows(part, TT2_PE_BWD_BLOCKS, 1, 1, p->dalpha, 0.f, s, 1);
  return tt2_check_launch(hipGetLastError(), "tt2_posenc_bwd");
}

extern "C" int tt2_shift_right(const float* mel, void* out, int batch, int t, int c, int dtype, hipStream_t s) {
  const int g = grid_for((int64_t)batch * t * c);
  by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(shift_right_kernel<T>, dim3(g), dim3(NT), 0, s, mel, (T*)out, batch, t, c);
  });
  return tt2_check_launch(hipGetLastError(), "tt2_shift_right");
}

