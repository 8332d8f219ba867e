// reduce.hip -- row reductions and bias gradients (column sums), HBM-bound (gfx950).
// Deterministic: fixed-order partial sums, no float atomics; 16-B vectorised where the row
// width allows.  reduce_rows_kernel also ends the positional encoding's dalpha (embed.hip) and
// the Adam gradient norm (optim.hip): they launch it through tt2_launch_reduce_rows.
#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {
constexpr int NT = 256;

// dst[c] = beta * dst[c] + sum_r src[r * ld + c]   (fixed order)
// block = 16 columns x 16 row groups (short dependent chains); LDS combine in a fixed order.
constexpr int RR_COLS = 16;
// block = CW columns x (NT / CW) row groups, CW = min(16, cols rounded up to a power of
// two): narrow reductions (the Adam norm's 1024 x 1 partials) use every lane.  Each lane
// sums its rows two at a time; the group sums combine in a fixed order (two levels).
__global__ __launch_bounds__(NT) void reduce_rows_kernel(const float* src, int rows, int cols, int64_t ld, float* dst,
                                                         float beta, int cw) {
  __shared__ float red[NT];
  const int G = NT / cw;
  const int cl = threadIdx.x % cw, g = threadIdx.x / cw;
  const int c = blockIdx.x * cw + cl;
  float s0 = 0.f, s1 = 0.f;
  if (c < cols) {
    int r = g;
    for (; r + G < rows; r += 2 * G) {
      s0 += src[(int64_t)r * ld + c];
      s1 += src[(int64_t)(r + G) * ld + c];
    }
    if (r < rows) s0 += src[(int64_t)r * ld + c];
  }
  red[threadIdx.x] = s0 + s1;
  __syncthreads();
  // level 1: 16 partial sums per column over strided groups; level 2: lane g == 0
  const int P = G < 16 ? G : 16;
  float t1 = 0.f;
  if (g < P)
    for (int k = g; k < G; k += P) t1 += red[k * cw + cl];
  __syncthreads();
  if (g < P) red[g * cw + cl] = t1;
  __syncthreads();
  if (g == 0 && c < cols) {
    float t = 0.f;
    for (int k = 0; k < P; ++k) t += red[k * cw + cl];
    dst[c] = beta != 0.f ? beta * dst[c] + t : t;
  }
}

// partial column sums of a [M, N] matrix: part[blockIdx.y][n] over rows [y*rows_per, ...).
// block = 64 columns (8 lanes x 8 columns, 16-B loads) x 32 row lanes; LDS combine.
template <typename T>
__global__ __launch_bounds__(NT) void colsum_partial_kernel(const T* x, int64_t ld, int M, int N, int rows_per,
                                                            int vec, float* part) {
  __shared__ float red[32][65];
  const int cg = threadIdx.x & 7, rg = threadIdx.x >> 3;
  const int n0 = blockIdx.x * 64 + cg * 8;
  const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (vec && n0 + 8 <= N) {
    for (int r = r0 + rg; r < r1; r += 32) {
      const T* p = x + (int64_t)r * ld + n0;
      ChunkV<T> c0 = ld_chunk<T>(p);
      if (Chunk<T>::N == 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += to_f32(c0.e[j % Chunk<T>::N]);
      } else {
        ChunkV<T> c1 = ld_chunk<T>(p + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[j] += to_f32(c0.e[j]); acc[4 + j] += to_f32(c1.e[j]); }
      }
    }
  } else {
    for (int r = r0 + rg; r < r1; r += 32)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (n0 + j < N) acc[j] += to_f32(x[(int64_t)r * ld + n0 + j]);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[rg][cg * 8 + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < 64) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    float s = 0.f;
    for (int r = 0; r < 32; ++r) s += red[r][threadIdx.x];
    if (n < N) part[(int64_t)blockIdx.y * N + n] = s;
  }
}

// number of row chunks for a colsum over [m, n]: ~1024 blocks total, >= 32 rows each
int colsum_chunks(int m, int n) {
  const int cb = (n + 63) / 64;
  int r = 1024 / cb;
  if (r < 1) r = 1;
  const int max_r = (m + 31) / 32;
  if (r > max_r) r = max_r;
  return r < 1 ? 1 : r;
}

}  // namespace

void tt2_launch_reduce_rows(const float* src, int rows, int cols, int64_t ld, float* dst, float beta, hipStream_t s,
                            int cw) {
  if (cw <= 0)
    for (cw = 1; cw < cols && cw < RR_COLS;) cw <<= 1;
  hipLaunchKernelGGL(reduce_rows_kernel, dim3((cols + cw - 1) / cw), dim3(NT), 0, s, src, rows, cols, ld, dst, beta,
                     cw);
}

extern "C" int tt2_reduce_rows(const tt2_reduce_args* p, hipStream_t s) {
  if (p->cols <= 0) return TT2_OK;
  tt2_launch_reduce_rows(p->src, p->rows, p->cols, p->ld, p->dst, p->beta, s);
  return tt2_check_launch(hipGetLastError(), "tt2_reduce_rows");
}

extern "C" size_t tt2_colsum_workspace_size(int m, int n) {
  return (size_t)colsum_chunks(m, n) * n * sizeof(float);
}

extern "C" int tt2_colsum(const void* x, int dtype, int64_t ld, int m, int n, float* dst, float beta, void* ws,
                          size_t ws_bytes, hipStream_t s) {
  if (n <= 0) return TT2_OK;
  if (ws_bytes < tt2_colsum_workspace_size(m, n)) return tt2_set_error(TT2_E_INVALID, "tt2_colsum: workspace");
  const int R = colsum_chunks(m, n);
  const int rows_per = (m + R - 1) / R;
  float* part = reinterpret_cast<float*>(ws);
  const int esz = dtype == TT2_DT_BF16 ? 2 : 4;
  const int vec = (reinterpret_cast<uintptr_t>(x) % 16 == 0) && ((ld * esz) % 16 == 0);
  dim3 g((n + 63) / 64, R);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(colsum_partial_kernel<T>, g, dim3(NT), 0, s, (const T*)x, ld, m, n, rows_per, vec, part);
  });
  tt2_launch_reduce_rows(part, R, n, n, dst, beta, s, RR_COLS);
  return tt2_check_launch(hipGetLastError(), "tt2_colsum");
}
