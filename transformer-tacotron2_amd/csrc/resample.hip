// resample.hip -- polyphase windowed-sinc sample-rate conversion (tt2_resample).  tt2_capi.h states
// the definition.  A translation unit of its own: no other kernel's code depends on it.
#include <limits.h>

#include <algorithm>

#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {

// Output n = q * up + r reads bank row r, and so do n + up, n + 2 up, ...: a thread owns one residue
// r over RS_P periods q, reads each tap of its row once and uses it RS_P times, one accumulator
// per period.  A work group is a tile of `rt` residues by `pg * RS_P` periods of one
// utterance: thread t has residue t % rt and, with g = t / rt, the periods g, g + pg, g + 2 pg, ...
// of the tile, so that neighbouring threads read neighbouring samples and write neighbouring
// outputs also when up is small.  It stages in LDS
//   sB  the tile's bank rows, [rt][K]: K is odd, so the threads of a wave, one row apart, read
//       different banks;
//   sX  the samples the tile reads.  Period j of the tile reads the window of `wmax` samples from
//       start + j * down, start = q0 * down + floor(r0 * down / up) - half, and sits at j * ps,
//       ps = min(down, wmax rounded up to even): with ps = down the windows of consecutive periods
//       overlap in LDS as they do in the utterance (one contiguous span), otherwise they are
//       disjoint.  A sample outside [0, len) is stored as 0 and not read.  A thread's RS_P windows
//       start at one parity (pg * ps is even unless an odd `down` meets an odd pg), so after at most
//       one single tap it reads its samples as aligned pairs.
// The host picks rt, pg and ps so that both fit the budgets below.  A tile wholly at or past the
// utterance's output length stages nothing and writes zeros.  y[n] is one accumulator from +0 over
// k ascending, one fma per tap: the tiling decides where a sum is computed, never its order.
constexpr int RS_THREADS = 256;
constexpr int RS_P = 8;            // periods per thread
constexpr int RS_RCAP = 64;        // residues per tile at most
constexpr int RS_SB = 8192;        // floats of sB at most (32 KiB)
constexpr int RS_SX = 8192;        // floats of sX at most (32 KiB)
constexpr int RS_WCAP = 1022;      // wmax at most: RS_P windows, one pad float each, always fit RS_SX
static_assert(RS_P * (RS_WCAP + 1) <= RS_SX && TT2_RESAMPLE_MAX_TAPS <= RS_WCAP, "one period group always fits");
static_assert(TT2_RESAMPLE_MAX_TAPS <= RS_SB, "one bank row always fits");

struct rs_plan {
  int rt, nrt;       // residues per tile, residue tiles
  int pg;            // period groups per tile: pg * rt <= RS_THREADS
  int ps, wmax;      // LDS stride of a period's window, window length
  int nx;            // floats of sX: (pg * RS_P - 1) * ps + wmax
  int nqt;           // period tiles per utterance
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

// dst[e] = src(e) for e < n, by the whole work group: batches of four independent loads
template <class F>
TT2_DEV void rs_stage(float* dst, int n, int tid, F src) {
  int e = tid;
  for (; e + 3 * RS_THREADS < n; e += 4 * RS_THREADS) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = src(e + u * RS_THREADS);
#pragma unroll
    for (int u = 0; u < 4; ++u) dst[e + u * RS_THREADS] = v[u];
  }
  for (; e < n; e += RS_THREADS) dst[e] = src(e);
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(tt2_resample_args a, rs_plan pl) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  float* sB = rs_lds;
  const int K = 2 * a.half + 1;
  float* sX = rs_lds + ((pl.rt * K + 1) & ~1);          // 8-byte aligned: the sample reads go in pairs
  const int tid = threadIdx.x;
  // blockIdx.x = (b * nrt + rtile) * nqt + qtile
  const int qt = blockIdx.x % (unsigned)pl.nqt;
  const int br = blockIdx.x / (unsigned)pl.nqt;
  const int rtile = br % pl.nrt;
  const int b = br / pl.nrt;
  const int r0 = rtile * pl.rt;
  const int nr = min(pl.rt, a.up - r0);                 // residues of this tile
  const int Q = pl.pg * RS_P;                           // periods of a tile
  const int64_t q0 = (int64_t)qt * Q;

  int len = a.lens ? a.lens[b] : a.n_in;
  len = min(max(len, 0), a.n_in);
  const int64_t full = ((int64_t)len * a.up + a.down - 1) / a.down;
  const int outb = (int)min(full, (int64_t)a.n_out);
  if (a.out_lens && rtile == 0 && qt == 0 && tid == 0) a.out_lens[b] = outb;

  const int rl = tid % pl.rt;
  const int g = tid / pl.rt;
  const bool active = g < pl.pg && rl < nr;
  const int r = r0 + rl;
  float* yrow = a.y + (int64_t)b * a.y_ld;
  const int64_t nfirst = q0 * a.up + r0;                // the lowest output index of the tile

  if (nfirst >= outb) {                                 // work-group uniform: nothing to compute
    if (active) {
#pragma unroll
      for (int p = 0; p < RS_P; ++p) {
        const int64_t n = (q0 + p * pl.pg + g) * a.up + r;
        if (n < a.n_out) yrow[n] = 0.f;
      }
    }
    return;
  }

  const int64_t base0 = (int64_t)r0 * a.down / a.up;    // floor(r0 * down / up)
  const int64_t start = q0 * a.down + base0 - a.half;
  const float* xrow = a.x + (int64_t)b * a.x_ld;
  // every load is unconditional (the index clamped into the utterance, the value dropped when it
  // was outside: len >= 1 here) and four are in flight per thread before the first LDS store
  rs_stage(sB, nr * K, tid, [&](int e) {
    const int row = e / K;
    return a.bank[(int64_t)(r0 + row) * a.bank_ld + (e - row * K)];
  });
  const int64_t last = len - 1;
  if (pl.ps == a.down) {                                // one contiguous span
    rs_stage(sX, pl.nx, tid, [&](int e) {
      const int64_t i = start + e, ic = min(max(i, (int64_t)0), last);
      const float v = xrow[ic];
      return i == ic ? v : 0.f;
    });
  } else {                                              // disjoint windows, `down` apart in the utterance
    rs_stage(sX, pl.nx, tid, [&](int e) {
      const int j = min(e / pl.ps, Q - 1);
      const int64_t i = start + (int64_t)j * a.down + (e - j * pl.ps), ic = min(max(i, (int64_t)0), last);
      const float v = xrow[ic];
      return i == ic ? v : 0.f;
    });
  }
  __syncthreads();
  if (!active) return;

  const int dr = (int)((int64_t)r * a.down / a.up - base0);   // < wmax - K + 1
  const float* taps = sB + rl * K;
  const int o0 = g * pl.ps + dr;
  const float* xs = sX + o0;
  const int pstep = pl.pg * pl.ps;                      // LDS distance of the thread's consecutive periods
  float acc[RS_P];
#pragma unroll
  for (int p = 0; p < RS_P; ++p) acc[p] = 0.f;
  auto one = [&](int k) {
    const float h = taps[k];
#pragma unroll
    for (int p = 0; p < RS_P; ++p) acc[p] = fmaf(h, xs[p * pstep + k], acc[p]);
  };
  if (pstep & 1) {                                      // (an odd `down` in one span with an odd pg)
#pragma unroll 4
    for (int k = 0; k < K; ++k) one(k);
  } else {
    // all of the thread's windows start at the parity of o0: after at most one single tap the
    // samples come as aligned pairs (ds_read_b64: twice the bytes per LDS cycle), k still ascending
    int k = 0;
    if (o0 & 1) one(0), k = 1;
#pragma unroll 2
    for (; k + 1 < K; k += 2) {
      const float h0 = taps[k], h1 = taps[k + 1];
#pragma unroll
      for (int p = 0; p < RS_P; ++p) {
        const f32x2 v = *reinterpret_cast<const f32x2*>(xs + p * pstep + k);
        acc[p] = fmaf(h0, v.x, acc[p]);
        acc[p] = fmaf(h1, v.y, acc[p]);
      }
    }
    if (k < K) one(k);
  }
#pragma unroll
  for (int p = 0; p < RS_P; ++p) {
    const int64_t n = (q0 + p * pl.pg + g) * a.up + r;
    if (n < a.n_out) yrow[n] = n < outb ? acc[p] : 0.f;
  }
}

int rs_err(const char* msg) { return tt2_invalid("tt2_resample", msg); }

// The tiling of one call; false when it needs more than INT_MAX work groups.
bool rs_make_plan(const tt2_resample_args* p, rs_plan* pl, int64_t* groups) {
  const int K = 2 * p->half + 1;
  const int64_t up = p->up, down = p->down;
  // residues per tile: the bank rows fit sB and the window fits RS_WCAP
  int64_t cap = std::min<int64_t>(RS_RCAP, RS_SB / K);
  cap = std::min<int64_t>(cap, 1 + (int64_t)(RS_WCAP - K) * up / down);
  cap = std::max<int64_t>(cap, 1);
  pl->nrt = (int)((up + cap - 1) / cap);
  pl->rt = (int)((up + pl->nrt - 1) / pl->nrt);
  // floor(x + d) - floor(x) <= ceil(d): the window of rt residues
  pl->wmax = (int)(((int64_t)(pl->rt - 1) * down + up - 1) / up) + K;
  pl->ps = (int)std::min<int64_t>(down, pl->wmax);
  if (pl->ps < down) pl->ps += pl->ps & 1;              // disjoint windows: an even stride, so that pairs stay aligned
  const int by_lds = ((RS_SX - pl->wmax) / pl->ps + 1) / RS_P;   // >= 1 as wmax, ps <= RS_WCAP
  pl->pg = std::max(1, std::min(RS_THREADS / pl->rt, by_lds));
  const int Q = pl->pg * RS_P;
  pl->nx = (Q - 1) * pl->ps + pl->wmax;
  const int64_t periods = ((int64_t)p->n_out + up - 1) / up;
  const int64_t nqt = (periods + Q - 1) / Q;
  *groups = nqt * pl->nrt * (int64_t)p->batch;
  if (nqt > INT_MAX || *groups > INT_MAX) return false;
  pl->nqt = (int)nqt;
  return true;
}
}  // namespace

extern "C" int tt2_resample(const tt2_resample_args* p, hipStream_t s) {
  if (!p) return rs_err("args required");
  if (p->up < 1 || p->down < 1 || p->up > TT2_RESAMPLE_MAX_PHASES)
    return rs_err("1 <= up <= TT2_RESAMPLE_MAX_PHASES and down >= 1");
  if (p->half < 0 || 2 * (int64_t)p->half + 1 > TT2_RESAMPLE_MAX_TAPS)
    return rs_err("half < 0 or 2 * half + 1 above TT2_RESAMPLE_MAX_TAPS");
  if (p->batch < 0 || p->n_in < 0 || p->n_out < 0) return rs_err("negative batch / n_in / n_out");
  if (p->x_ld < p->n_in || p->y_ld < p->n_out || p->bank_ld < 2 * p->half + 1)
    return rs_err("x_ld < n_in, y_ld < n_out or bank_ld < 2 * half + 1");
  if (!p->bank || !p->y) return rs_err("bank and y required");
  rs_plan pl;
  int64_t groups = 0;
  if (!rs_make_plan(p, &pl, &groups)) return rs_err("more than 2^31 - 1 work groups");
  if (p->batch == 0 || p->n_out == 0) return TT2_OK;
  if (!p->x && p->n_in > 0) return rs_err("x required");
  const size_t lds = sizeof(float) * ((((size_t)pl.rt * (2 * p->half + 1) + 1) & ~(size_t)1) + pl.nx);
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)groups), dim3(RS_THREADS), lds, s, *p, pl);
  return tt2_check_launch(hipGetLastError(), "tt2_resample");
}
