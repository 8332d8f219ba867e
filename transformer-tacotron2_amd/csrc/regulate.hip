// regulate.hip -- the length regulator of a non-autoregressive student: durations -> segment ends and
// the frame -> phoneme index (tt2_regulate_plan), phoneme rows -> frame rows (tt2_regulate_fwd) and
// the segment sum of frame rows per phoneme (tt2_regulate_bwd), the gradient of the expansion.
// tt2_capi.h states the definition.  A translation unit of its own: no other kernel's code depends
// on it.  One launch per entry, no workspace, no host synchronisation, no atomics.
//
//   regulate_plan_kernel   a work group per utterance (x up to 64 slices of the index): durations
//                          to LDS, a 64-bit scan over 256 per-thread runs, ends in LDS (16 KB at
//                          tx = 4096), the index by binary search over them
//   regulate_fwd_kernel    lanes across a row's 16-byte chunks (or its elements, where base, strides
//                          or dim rule the chunks out), FW_ROWS rows per thread in flight: a copy of bits
//   regulate_bwd_kernel    the same lanes, one phoneme per lane group: f32 accumulators in registers,
//                          the frames of the phoneme added in ascending order, 16 or 4 loads in flight
// A phoneme's sum is serial in its duration by definition, so the longest phoneme of a launch is its
// tail (DESIGN.md 5.13 has the measurement).
#include <limits.h>

#include <algorithm>

#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_PLAN_SLICES = 64;     // plan: work groups per utterance at most (each redoes the scan)
constexpr int RG_PLAN_SLICE_ROWS = 1024;
constexpr int FW_ROWS = 4;             // fwd: rows per thread, their loads issued together
constexpr int BW_ROWS = 4;             // bwd: frame rows loaded together, added in order
constexpr int BW_ROWS_LONG = 16;       // ... while a phoneme has that many left: the long ones are the launch's tail

TT2_DEV int rg_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(RG_THREADS) void regulate_plan_kernel(tt2_regulate_plan_args a, int slices) {
  __shared__ int32_t s_ends[TT2_REGULATE_MAX_PHONEMES];
  __shared__ unsigned long long s_run[RG_THREADS];
  const int b = blockIdx.x / (unsigned)slices;
  const int c = blockIdx.x % (unsigned)slices;
  const int tid = threadIdx.x;
  const int tx = a.tx;
  const int txb = a.key_len ? rg_clamp(a.key_len[b], 0, tx) : tx;
  const int32_t* dur = a.durations + (int64_t)b * a.dur_ld;
  // d' to LDS with coalesced reads; entries at and past Tx_b are not read
  for (int t = tid; t < tx; t += RG_THREADS) s_ends[t] = t < txb ? max(dur[t], 0) : 0;
  __syncthreads();
  // thread i owns the `per` consecutive phonemes from i * per: its run's sum, then an inclusive
  // scan of the 256 sums in 64-bit integers (4096 * (2^31 - 1) < 2^43: nothing wraps)
  const int per = (tx + RG_THREADS - 1) / RG_THREADS;
  const int t0 = tid * per, t1 = min(t0 + per, tx);
  unsigned long long run = 0;
  for (int t = t0; t < t1; ++t) run += (unsigned long long)s_ends[t];
  s_run[tid] = run;
  __syncthreads();
  for (int o = 1; o < RG_THREADS; o <<= 1) {
    const unsigned long long v = tid >= o ? s_run[tid - o] : 0ull;
    __syncthreads();
    s_run[tid] += v;
    __syncthreads();
  }
  const unsigned long long n_out = (unsigned long long)a.n_out;
  unsigned long long acc = tid ? s_run[tid - 1] : 0ull;
  for (int t = t0; t < t1; ++t) {
    acc += (unsigned long long)s_ends[t];
    s_ends[t] = (int32_t)min(acc, n_out);
  }
  const unsigned long long sum = s_run[RG_THREADS - 1];
  const int frames = (int)min(sum, n_out);
  __syncthreads();
  if (c == 0) {
    int32_t* erow = a.ends + (int64_t)b * a.ends_ld;
    for (int t = tid; t < tx; t += RG_THREADS) erow[t] = s_ends[t];
    if (tid == 0) {
      if (a.frames) a.frames[b] = frames;
      if (a.total) a.total[b] = (int32_t)min(sum, (unsigned long long)INT_MAX);
    }
  }
  if (!a.index) return;
  int32_t* irow = a.index + (int64_t)b * a.index_ld;
  for (int64_t n = (int64_t)c * RG_THREADS + tid; n < a.n_out; n += (int64_t)slices * RG_THREADS) {
    int idx = -1;
    if (n < frames) {      // the lowest t with ends[t] > n: ends[tx - 1] = frames > n, so it exists
      int lo = 0, hi = tx - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_ends[mid] > (int32_t)n) hi = mid; else lo = mid + 1;
      }
      idx = lo;
    }
    irow[n] = idx;
  }
}

// The geometry fwd and bwd share: `lanes` threads (a power of two, 1 .. 256) stride over the `units`
// of a row (16-byte chunks or single elements), RG_THREADS / lanes rows side by side.
struct rg_geom {
  int units;      // per row
  int lanes;      // threads per row
  int rows;       // rows per work group (fwd: x FW_ROWS)
  int blocks;     // work groups per utterance
};

rg_geom rg_geometry(int dim, int unit, int64_t nrows, int rows_per_thread) {
  rg_geom g;
  g.units = dim / unit;
  g.lanes = 1;
  while (g.lanes < g.units && g.lanes < RG_THREADS) g.lanes <<= 1;
  g.rows = RG_THREADS / g.lanes * rows_per_thread;
  g.blocks = (int)std::min<int64_t>((nrows + g.rows - 1) / g.rows, INT_MAX);
  return g;
}

// U is the unit of the copy: u32x4 (16 bytes), uint32_t (an f32) or uint16_t (a bf16).  Bits only.
template <typename U>
__global__ __launch_bounds__(RG_THREADS) void regulate_fwd_kernel(tt2_regulate_args a, rg_geom g) {
  const int b = blockIdx.x / (unsigned)g.blocks;
  const int blk = blockIdx.x % (unsigned)g.blocks;
  const int lane = threadIdx.x & (g.lanes - 1), sub = threadIdx.x / (unsigned)g.lanes;
  const int per = RG_THREADS / g.lanes;
  constexpr int64_t E = sizeof(U);     // a.*_ld and a.*_bs count elements of a.dtype, not units
  const int64_t es = a.dtype == TT2_DT_F32 ? 4 : 2;
  const char* src = static_cast<const char*>(a.src) + (int64_t)b * a.src_bs * es;
  char* dst = static_cast<char*>(a.dst) + (int64_t)b * a.dst_bs * es;
  const int32_t* map = a.map ? a.map + (int64_t)b * a.map_ld : nullptr;
  int64_t n[FW_ROWS];
  int idx[FW_ROWS];
#pragma unroll
  for (int r = 0; r < FW_ROWS; ++r) {
    n[r] = (int64_t)blk * g.rows + r * per + sub;
    idx[r] = (n[r] < a.n_out && map) ? map[n[r]] : -1;
    if (idx[r] >= a.tx) idx[r] = -1;
  }
  for (int u = lane; u < g.units; u += g.lanes) {
    U v[FW_ROWS];
#pragma unroll
    for (int r = 0; r < FW_ROWS; ++r) {
      v[r] = U{};
      if (idx[r] >= 0) v[r] = *reinterpret_cast<const U*>(src + (int64_t)idx[r] * a.src_ld * es + u * E);
    }
#pragma unroll
    for (int r = 0; r < FW_ROWS; ++r) {
      if (n[r] < a.n_out) *reinterpret_cast<U*>(dst + n[r] * a.dst_ld * es + u * E) = v[r];
    }
  }
}

// T the element type, N the elements of a unit (16 bytes' worth, or 1)
template <typename T, int N> struct alignas(sizeof(T) * N) rg_unit { T e[N]; };

// acc += R consecutive frame rows from p, in row order; the R loads are issued before the first add
template <typename T, int N, int R>
TT2_DEV void rg_add_rows(float (&acc)[N], const T* p, int64_t ld) {
  rg_unit<T, N> v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) v[r] = *reinterpret_cast<const rg_unit<T, N>*>(p + r * ld);
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = __fadd_rn(acc[k], to_f32(v[r].e[k]));
  }
}

// One lane group per phoneme.
template <typename T, int N>
__global__ __launch_bounds__(RG_THREADS) void regulate_bwd_kernel(tt2_regulate_args a, rg_geom g) {
  using unit = rg_unit<T, N>;
  const int b = blockIdx.x / (unsigned)g.blocks;
  const int blk = blockIdx.x % (unsigned)g.blocks;
  const int lane = threadIdx.x & (g.lanes - 1), sub = threadIdx.x / (unsigned)g.lanes;
  const int t = blk * g.rows + sub;
  if (t >= a.tx) return;
  const T* src = static_cast<const T*>(a.src) + (int64_t)b * a.src_bs;
  T* drow = static_cast<T*>(a.dst) + (int64_t)b * a.dst_bs + (int64_t)t * a.dst_ld;
  int s = 0, e = 0;
  if (a.n_out > 0) {
    const int32_t* ends = a.map + (int64_t)b * a.map_ld;
    s = t ? rg_clamp(ends[t - 1], 0, a.n_out) : 0;
    e = rg_clamp(ends[t], 0, a.n_out);
  }
  for (int u = lane; u < g.units; u += g.lanes) {
    float acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.f;
    const T* col = src + (int64_t)u * N;
    int n = s;
    for (; n + BW_ROWS_LONG <= e; n += BW_ROWS_LONG) rg_add_rows<T, N, BW_ROWS_LONG>(acc, col + (int64_t)n * a.src_ld, a.src_ld);
    for (; n + BW_ROWS <= e; n += BW_ROWS) rg_add_rows<T, N, BW_ROWS>(acc, col + (int64_t)n * a.src_ld, a.src_ld);
    for (; n < e; ++n) rg_add_rows<T, N, 1>(acc, col + (int64_t)n * a.src_ld, a.src_ld);
    unit o;
#pragma unroll
    for (int k = 0; k < N; ++k) o.e[k] = from_f32<T>(acc[k]);
    *reinterpret_cast<unit*>(drow + (int64_t)u * N) = o;
  }
}

// 16-byte units need both bases on 16 bytes and every stride and dim a whole number of units
bool rg_chunks_ok(const tt2_regulate_args& p, int n) {
  const uintptr_t bases = reinterpret_cast<uintptr_t>(p.src) | reinterpret_cast<uintptr_t>(p.dst);
  const int64_t strides = p.src_ld | p.src_bs | p.dst_ld | p.dst_bs | (int64_t)p.dim;
  return (bases & 15) == 0 && (strides & (n - 1)) == 0;
}

// What fwd and bwd refuse alike; map_cols is the extent of a row of `map`
int rg_check(const char* who, const tt2_regulate_args* p, int64_t map_cols) {
  if (!p) return tt2_invalid(who, "args required");
  if (p->batch < 0 || p->tx < 0 || p->n_out < 0 || p->dim < 0) return tt2_invalid(who, "negative batch / tx / n_out / dim");
  if (p->tx > TT2_REGULATE_MAX_PHONEMES) return tt2_invalid(who, "tx above TT2_REGULATE_MAX_PHONEMES");
  if (p->dtype != TT2_DT_F32 && p->dtype != TT2_DT_BF16) return tt2_invalid(who, "dtype must be TT2_DT_F32 or TT2_DT_BF16");
  if (p->src_ld < p->dim || p->dst_ld < p->dim) return tt2_invalid(who, "src_ld or dst_ld < dim");
  if (p->map_ld < map_cols) return tt2_invalid(who, "map_ld below the extent of a row of map");
  return TT2_OK;
}

}  // namespace

extern "C" int tt2_regulate_plan(const tt2_regulate_plan_args* p, hipStream_t s) {
  const char* who = "tt2_regulate_plan";
  if (!p) return tt2_invalid(who, "args required");
  if (p->batch < 0 || p->tx < 0 || p->n_out < 0) return tt2_invalid(who, "negative batch / tx / n_out");
  if (p->tx > TT2_REGULATE_MAX_PHONEMES) return tt2_invalid(who, "tx above TT2_REGULATE_MAX_PHONEMES");
  if (p->dur_ld < p->tx || p->ends_ld < p->tx) return tt2_invalid(who, "dur_ld or ends_ld < tx");
  if (p->index && p->index_ld < p->n_out) return tt2_invalid(who, "index_ld < n_out");
  const int slices = p->index ? (int)std::max<int64_t>(1, std::min<int64_t>(RG_PLAN_SLICES, ((int64_t)p->n_out + RG_PLAN_SLICE_ROWS - 1) / RG_PLAN_SLICE_ROWS)) : 1;
  if ((int64_t)p->batch * slices > INT_MAX) return tt2_invalid(who, "more than 2^31 - 1 work groups");
  if (p->batch == 0) return TT2_OK;
  if (p->tx > 0 && (!p->durations || !p->ends)) return tt2_invalid(who, "durations and ends required");
  if (p->tx == 0 && !p->frames && !p->total && !(p->index && p->n_out > 0)) return TT2_OK;   // nothing to write
  hipLaunchKernelGGL(regulate_plan_kernel, dim3((unsigned)(p->batch * slices)), dim3(RG_THREADS), 0, s, *p, slices);
  return tt2_check_launch(hipGetLastError(), who);
}

extern "C" int tt2_regulate_fwd(const tt2_regulate_args* p, hipStream_t s) {
  const char* who = "tt2_regulate_fwd";
  const int rc = rg_check(who, p, p ? p->n_out : 0);
  if (rc != TT2_OK) return rc;
  const int n = p->dtype == TT2_DT_F32 ? 4 : 8;
  const bool chunks = rg_chunks_ok(*p, n);
  const rg_geom g = rg_geometry(p->dim, chunks ? n : 1, p->n_out, FW_ROWS);
  if ((int64_t)p->batch * g.blocks > INT_MAX) return tt2_invalid(who, "more than 2^31 - 1 work groups");
  if (p->batch == 0 || p->n_out == 0 || p->dim == 0) return TT2_OK;
  if (!p->dst) return tt2_invalid(who, "dst required");
  if (p->tx > 0 && (!p->src || !p->map)) return tt2_invalid(who, "src and map required");
  const dim3 grid((unsigned)(p->batch * g.blocks)), block(RG_THREADS);
  if (chunks) {
    hipLaunchKernelGGL(regulate_fwd_kernel<u32x4>, grid, block, 0, s, *p, g);
  } else if (p->dtype == TT2_DT_F32) {
    hipLaunchKernelGGL(regulate_fwd_kernel<uint32_t>, grid, block, 0, s, *p, g);
  } else {
    hipLaunchKernelGGL(regulate_fwd_kernel<uint16_t>, grid, block, 0, s, *p, g);
  }
  return tt2_check_launch(hipGetLastError(), who);
}

extern "C" int tt2_regulate_bwd(const tt2_regulate_args* p, hipStream_t s) {
  const char* who = "tt2_regulate_bwd";
  const int rc = rg_check(who, p, p ? p->tx : 0);
  if (rc != TT2_OK) return rc;
  const int n = p->dtype == TT2_DT_F32 ? 4 : 8;
  const bool chunks = rg_chunks_ok(*p, n);
  const rg_geom g = rg_geometry(p->dim, chunks ? n : 1, p->tx, 1);
  if ((int64_t)p->batch * g.blocks > INT_MAX) return tt2_invalid(who, "more than 2^31 - 1 work groups");
  if (p->batch == 0 || p->tx == 0 || p->dim == 0) return TT2_OK;
  if (!p->dst) return tt2_invalid(who, "dst required");
  if (p->n_out > 0 && (!p->src || !p->map)) return tt2_invalid(who, "src and map required");
  const dim3 grid((unsigned)(p->batch * g.blocks)), block(RG_THREADS);
  if (p->dtype == TT2_DT_F32) {
    if (chunks) hipLaunchKernelGGL((regulate_bwd_kernel<float, 4>), grid, block, 0, s, *p, g);
    else hipLaunchKernelGGL((regulate_bwd_kernel<float, 1>), grid, block, 0, s, *p, g);
  } else {
    if (chunks) hipLaunchKernelGGL((regulate_bwd_kernel<bf16, 8>), grid, block, 0, s, *p, g);
    else hipLaunchKernelGGL((regulate_bwd_kernel<bf16, 1>), grid, block, 0, s, *p, g);
  }
  return tt2_check_launch(hipGetLastError(), who);
}
