// repack.hip -- casts and weight repacks, HBM-bound byte movers (gfx950): the strided 2-D cast
// between f32, bf16 and f16, and the three conv-weight layouts (the dgrad flip of one layer, of
// every layer in one launch, and nn.Conv1d -> tap-major).
#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {
constexpr int NT = 256;

TT2_DEV float ldf(const void* p, int64_t i, int dt) {
  if (dt == TT2_F16) return (float)reinterpret_cast<const f16*>(p)[i];
  return dt == TT2_BF16 ? (float)reinterpret_cast<const bf16*>(p)[i] : reinterpret_cast<const float*>(p)[i];
}
TT2_DEV void stf(void* p, int64_t i, int dt, float v) {
  if (dt == TT2_F16) reinterpret_cast<f16*>(p)[i] = (f16)v;
  else if (dt == TT2_BF16) reinterpret_cast<bf16*>(p)[i] = (bf16)v;
  else reinterpret_cast<float*>(p)[i] = v;
}

__global__ void cast2d_kernel(const void* src, int sdt, int64_t sld, void* dst, int ddt, int64_t dld, int M, int N) {
  const int64_t total = (int64_t)M * N;
  for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int m = (int)(i / N), n = (int)(i % N);
    stf(dst, (int64_t)m * dld + n, ddt, ldf(src, (int64_t)m * sld + n, sdt));
  }
}

// ------------------------------------------------------------ weight repack
// conv dgrad weight: wd[ci][tap'][co] = w[co][K-1-tap'][ci] -- per tap a [Cout x Cin] ->
// [Cin x Cout] transpose through a 64 x 64 LDS tile: reads coalesced along ci, writes along co.
template <typename T>
TT2_DEV void conv_wflip_tile(const T* w, T* wd, int Cout, int Cin, int K, int bx, int by, int tap) {
  __shared__ T tile[64][65];
  const int ci0 = bx * 64, co0 = by * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll 4
  for (int r = ty; r < 64; r += NT / 64) {
    const int co = co0 + r, ci = ci0 + tx;
    if (co < Cout && ci < Cin) tile[r][tx] = w[((int64_t)co * K + tap) * Cin + ci];
  }
  __syncthreads();
  const int tp = K - 1 - tap;
#pragma unroll 4
  for (int r = ty; r < 64; r += NT / 64) {
    const int ci = ci0 + r, co = co0 + tx;
    if (co < Cout && ci < Cin) wd[((int64_t)ci * K + tp) * Cout + co] = tile[tx][r];
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void conv_wflip_kernel(const T* w, T* wd, int Cout, int Cin, int K) {
  conv_wflip_tile<T>(w, wd, Cout, Cin, K, blockIdx.x, blockIdx.y, blockIdx.z);
}

// every conv layer's flip in one launch: workgroup b belongs to the job whose item range
// [first[j], first[j + 1]) holds it; items are (tap, co block, ci block) in that order
struct WflipBatch {
  tt2_wflip_job job[TT2_WFLIP_MAX];
  int first[TT2_WFLIP_MAX + 1];
  int n;
};
template <typename T>
__global__ __launch_bounds__(NT) void conv_wflip_batch_kernel(WflipBatch B) {
  int j = 0;
  while (j + 1 < B.n && (int)blockIdx.x >= B.first[j + 1]) ++j;
  const tt2_wflip_job& J = B.job[j];
  const int it = blockIdx.x - B.first[j], nbx = (J.cin + 63) / 64, nby = (J.cout + 63) / 64;
  conv_wflip_tile<T>(reinterpret_cast<const T*>(J.w), reinterpret_cast<T*>(J.wd), J.cout, J.cin, J.k, it % nbx,
                     (it / nbx) % nby, it / (nbx * nby));
}

// nn.Conv1d weight [Cout][Cin][K] -> tap-major [Cout][K][Cin]: per output channel a
// [Cin x K] -> [K x Cin] transpose (weights are small; one thread per element, writes coalesced)
template <typename T>
__global__ __launch_bounds__(NT) void conv_wpack_kernel(const T* w, T* wp, int Cout, int Cin, int K) {
  const int64_t total = (int64_t)Cout * Cin * K;
  for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int ci = (int)(i % Cin);
    const int64_t r = i / Cin;
    const int tap = (int)(r % K), co = (int)(r / K);
    wp[i] = w[((int64_t)co * Cin + ci) * K + tap];
  }
}

}  // namespace

extern "C" int tt2_cast2d(const void* src, int src_dtype, int64_t src_ld, void* dst, int dst_dtype, int64_t dst_ld,
                          int m, int n, hipStream_t s) {
  if ((int64_t)m * n == 0) return TT2_OK;
  hipLaunchKernelGGL(cast2d_kernel, dim3(grid_for((int64_t)m * n)), dim3(NT), 0, s, src, src_dtype, src_ld, dst,
                     dst_dtype, dst_ld, m, n);
  return tt2_check_launch(hipGetLastError(), "tt2_cast2d");
}

extern "C" int tt2_conv_weight_flip(const void* w, void* wd, int cout, int cin, int k, int dtype, hipStream_t s) {
  if (cout <= 0 || cin <= 0 || k <= 0) return TT2_OK;
  const dim3 g((cin + 63) / 64, (cout + 63) / 64, k);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(conv_wflip_kernel<T>, g, dim3(NT), 0, s, (const T*)w, (T*)wd, cout, cin, k);
  });
  return tt2_check_launch(hipGetLastError(), "tt2_conv_weight_flip");
}

extern "C" int tt2_conv_weight_flip_batch(const tt2_wflip_job* jobs, int32_t n, int32_t dtype, hipStream_t s) {
  if (n <= 0) return TT2_OK;
  if (n > TT2_WFLIP_MAX || !jobs) return tt2_set_error(TT2_E_INVALID, "tt2_conv_weight_flip_batch: 1..16 jobs");
  WflipBatch B{};
  B.n = n;
  for (int j = 0; j < n; ++j) {
    const tt2_wflip_job& J = jobs[j];
    if (J.cout <= 0 || J.cin <= 0 || J.k <= 0 || !J.w || !J.wd || J.w == J.wd)
      return tt2_set_error(TT2_E_INVALID, "tt2_conv_weight_flip_batch: bad job");
    B.job[j] = J;
    B.first[j + 1] = B.first[j] + ((J.cin + 63) / 64) * ((J.cout + 63) / 64) * J.k;
  }
  by_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(conv_wflip_batch_kernel<decltype(t)>, dim3(B.first[n]), dim3(NT), 0, s, B);
  });
  return tt2_check_launch(hipGetLastError(), "tt2_conv_weight_flip_batch");
}

extern "C" int tt2_conv_weight_pack(const void* w, void* wp, int32_t cout, int32_t cin, int32_t k, int32_t dtype,
                                    hipStream_t s) {
  if (cout <= 0 || cin <= 0 || k <= 0) return TT2_OK;
  if (!w || !wp || w == wp) return tt2_set_error(TT2_E_INVALID, "tt2_conv_weight_pack: null or in-place");
  if (dtype != TT2_DT_BF16 && dtype != TT2_DT_F32) return tt2_set_error(TT2_E_INVALID, "tt2_conv_weight_pack: dtype");
  const int g = grid_for((int64_t)cout * cin * k, NT, 4096);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(conv_wpack_kernel<T>, dim3(g), dim3(NT), 0, s, (const T*)w, (T*)wp, cout, cin, k);
  });
  return tt2_check_launch(hipGetLastError(), "tt2_conv_weight_pack");
}
