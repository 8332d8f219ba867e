// tt2_internal.h -- library-internal helpers (not part of the public C ABI).
#pragma once
#include <hip/hip_runtime_api.h>

extern "C" {
int tt2_set_error(int code, const char* msg);
int tt2_check_launch(hipError_t err, const char* what);
}
// What every entry point refuses with (runtime.cpp; hidden: not part of the library's exports).
// tt2_invalid: sets "who: msg" and returns TT2_E_INVALID.  tt2_need_workspace: TT2_OK when need
// is 0 or `ws` holds `have` >= need bytes at a multiple of `align` (a power of two), else
// tt2_invalid(who, "workspace too small or misaligned: <need> bytes needed").
__attribute__((visibility("hidden"))) int tt2_invalid(const char* who, const char* msg);
__attribute__((visibility("hidden"))) int tt2_need_workspace(const char* who, const void* ws, size_t have, size_t need,
                                                             size_t align);
// compute units of the current device (cached per device; 256 on an MI355X)
int tt2_cu_count();
// reduce.hip: launches the one reduce_rows_kernel, dst[c] = beta * dst[c] + sum_r src[r * ld + c],
// cw columns to a work group (0: tt2_reduce_rows' choice, min(16, cols rounded up to a power of
// two)).  Sets no error and reads no launch status: the calling entry point checks its own launches.
void tt2_launch_reduce_rows(const float* src, int rows, int cols, int64_t ld, float* dst, float beta,
                            hipStream_t stream, int cw = 0);
