// tt2_internal.h -- library-internal helpers (not part of the public C ABI).
#pragma once
#include <hip/hip_runtime_api.h>

extern "C" {
int tt2_set_error(int code, const char* msg);
int tt2_check_launch(hipError_t err, const char* what);
}
// compute units of the current device (cached per device; 256 on an MI355X)
int tt2_cu_count();
// reduce.hip: launches the one reduce_rows_kernel, dst[c] = beta * dst[c] + sum_r src[r * ld + c],
// cw columns to a work group (0: tt2_reduce_rows' choice, min(16, cols rounded up to a power of
// two)).  Sets no error and reads no launch status: the calling entry point checks its own launches.
void tt2_launch_reduce_rows(const float* src, int rows, int cols, int64_t ld, float* dst, float beta,
                            hipStream_t stream, int cw = 0);
