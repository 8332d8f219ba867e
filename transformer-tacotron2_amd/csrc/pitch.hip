// pitch.hip -- YIN pitch and frame energy on the mel frame grid (tt2_yin).  tt2_capi.h states the
// definition.  A translation unit of its own: no other kernel's code depends on it.
#include <limits.h>
#include <math.h>


#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {

// One wave per frame, YIN_NW consecutive frames of an utterance per work group; the waves share
// nothing and never meet at a work-group barrier.  A wave stages its 1024 samples in its own LDS
// row and sums their squares on the way (the energy).  Lane l owns the 8 lags 8l .. 8l + 7.  The
// samples j < 512 go by in blocks of 8: the block's y[j] come as two broadcast b128 reads, and the
// lane keeps y[j0 + 8l .. j0 + 8l + 15] in registers, a window that slides by 8 per block with two
// aligned b128 reads.  Sample j0 + jj against lag 8l + k needs window entry jj + k: one subtract
// and one fma, 64 of each per block and lane, with both LDS reads issued one block ahead.  The
// loop is plain f32: packed (v_pk_add_f32 / v_pk_fma_f32 over even-aligned lag pairs) it measured
// 5 % slower, so build_lib.py compiles this file without SLP vectorisation, which would pack it
// again.  Every sum has a fixed order: d(tau) runs over j ascending in one accumulator.
//
// LDS image: sample e sits at e ^ 4 when bit 6 of e is set.  Lanes l and l + 8 (and l + 24), whose
// 32-byte windows would meet in the same banks inside one 16-lane group of a b128 read, differ in
// that bit, so one reads the upper half of the banks while the other reads the lower.
constexpr int YIN_NW = 4;
constexpr int YIN_ROW = TT2_YIN_FRAME + 8;   // the last block's look-ahead read lands in the padding
constexpr int YIN_LPL = 8;                   // lags per lane
static_assert(64 * YIN_LPL == TT2_YIN_WINDOW && TT2_YIN_MAX_LAG == TT2_YIN_WINDOW - 1, "64 lanes cover the lags");
static_assert(TT2_YIN_WINDOW - 1 + TT2_YIN_MAX_LAG < TT2_YIN_FRAME, "W + tau stays inside the frame");

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

TT2_DEV int yin_swz(int e) { return e ^ ((e & 64) >> 4); }

TT2_DEV void yin_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// samples e0 .. e0 + 7 of the row (e0 a multiple of 8) as four pairs
TT2_DEV void yin_ld8(const float* Y, int e0, f32x2 (&d)[4]) {
  const int p = e0 | ((e0 & 64) >> 4);
  const f32x4 lo = *reinterpret_cast<const f32x4*>(Y + p);
  const f32x4 hi = *reinterpret_cast<const f32x4*>(Y + (p ^ 4));
  d[0] = f32x2{lo.x, lo.y}, d[1] = f32x2{lo.z, lo.w}, d[2] = f32x2{hi.x, hi.y}, d[3] = f32x2{hi.z, hi.w};
}

__global__ __launch_bounds__(64 * YIN_NW) void yin_kernel(tt2_yin_args a, int groups) {
  __shared__ __attribute__((aligned(16))) float sY[YIN_NW][YIN_ROW];
  __shared__ __attribute__((aligned(16))) float sD[YIN_NW][TT2_YIN_WINDOW];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x / groups;
  const int f = (blockIdx.x - b * groups) * YIN_NW + w;
  if (f >= a.t) return;   // wave-uniform, as every branch below
  int nv = a.frames ? a.frames[b] : a.t;
  nv = min(max(nv, 0), a.t);
  const int64_t o = (int64_t)b * a.t + f;
  if (f >= nv) {
    if (lane == 0) a.f0[o] = 0.f, a.lag[o] = -1, a.aper[o] = 1.f, a.energy[o] = 0.f;
    return;
  }
  const float* src = a.x + (int64_t)b * a.utt_stride + (int64_t)f * a.hop;
  float* Y = sY[w];
  float* Dp = sD[w];

  // ---- stage the frame (any hop: dword loads), sum of squares on the way
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < TT2_YIN_FRAME / 64; ++i) {
    const int e = lane + 64 * i;
    const float v = src[e];
    Y[yin_swz(e)] = v;
    ss = fmaf(v, v, ss);
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) ss += __shfl_xor(ss, s);
  yin_wave_sync();

  // ---- the difference function of the lane's 8 lags
  const int lb = YIN_LPL * lane;
  f32x2 win[8];
  float d[YIN_LPL];
#pragma unroll
  for (int k = 0; k < YIN_LPL; ++k) d[k] = 0.f;
  {
    f32x2 t[4];
    yin_ld8(Y, lb, t);
#pragma unroll
    for (int m = 0; m < 4; ++m) win[m] = t[m];
    yin_ld8(Y, lb + 8, t);
#pragma unroll
    for (int m = 0; m < 4; ++m) win[4 + m] = t[m];
  }
  f32x2 yb[4];
  yin_ld8(Y, 0, yb);                // the block's own samples, the same address in every lane
#pragma unroll 4
  for (int j0 = 0; j0 < TT2_YIN_WINDOW; j0 += 8) {
    f32x2 nx[4], ybn[4];
    yin_ld8(Y, j0 + lb + 16, nx);   // both reads are for the next block: a block never waits for its own
    yin_ld8(Y, j0 + 8, ybn);
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const float yj = (jj & 1) ? yb[jj / 2].y : yb[jj / 2].x;
#pragma unroll
      for (int k = 0; k < YIN_LPL; ++k) {
        const int i = jj + k;
        const float df = yj - ((i & 1) ? win[i / 2].y : win[i / 2].x);
        d[k] = fmaf(df, df, d[k]);
      }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) win[m] = win[4 + m], win[4 + m] = nx[m], yb[m] = ybn[m];
  }

  // ---- S(tau): the lane's running sum plus the sum of the lanes below (d(0) is an exact 0)
  float run[YIN_LPL];
  run[0] = d[0];
#pragma unroll
  for (int k = 1; k < YIN_LPL; ++k) run[k] = run[k - 1] + d[k];
  float inc = run[YIN_LPL - 1];
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const float t = __shfl_up(inc, s);
    if (lane >= s) inc += t;
  }
  float below = __shfl_up(inc, 1);
  if (lane == 0) below = 0.f;
  float cm[YIN_LPL];
#pragma unroll
  for (int k = 0; k < YIN_LPL; ++k) {
    const float S = below + run[k];
    cm[k] = S > 0.f ? (d[k] * (float)(lb + k)) / S : 1.f;
  }
  if (lane == 0) cm[0] = 1.f;
  *reinterpret_cast<f32x4*>(Dp + lb) = f32x4{cm[0], cm[1], cm[2], cm[3]};
  *reinterpret_cast<f32x4*>(Dp + lb + 4) = f32x4{cm[4], cm[5], cm[6], cm[7]};
  yin_wave_sync();
  if (a.cmnd) {
    float* c = a.cmnd + o * a.cmnd_ld;
    for (int tau = lane; tau <= a.tau_max; tau += 64) c[tau] = Dp[tau];
  }

  // ---- the first lag under the threshold, then downhill while the next lag is strictly lower
  int lag = -1;
  for (int base = a.tau_min & ~63; base <= a.tau_max && lag < 0; base += 64) {
    const int tau = base + lane;
    const bool in = tau >= a.tau_min && tau <= a.tau_max;
    const float v = Dp[min(tau, TT2_YIN_MAX_LAG)];
    const uint64_t m = __ballot(in && v < a.threshold);
    if (m) lag = base + __builtin_ctzll(m);
  }
  bool voiced = lag >= 0;
  if (voiced) {
    for (int base = lag;; base += 64) {
      const int tau = base + lane, q = min(tau, TT2_YIN_MAX_LAG - 1);
      const bool stop = tau >= a.tau_max || !(Dp[q + 1] < Dp[q]);
      const uint64_t m = __ballot(stop);
      if (m) {
        lag = base + __builtin_ctzll(m);
        break;
      }
    }
  } else {   // the lowest lag that attains the minimum
    float bv = INFINITY;
    int bi = INT_MAX;
    for (int tau = a.tau_min + lane; tau <= a.tau_max; tau += 64) {
      const float v = Dp[tau];
      if (v < bv) bv = v, bi = tau;
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const float ov = __shfl_xor(bv, s);
      const int oi = __shfl_xor(bi, s);
      if (ov < bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    lag = bi == INT_MAX ? a.tau_min : bi;   // (no finite value anywhere: unspecified, but in range)
  }
  lag = __builtin_amdgcn_readfirstlane(lag);
  const float bq = Dp[lag];
  float f0 = 0.f;
  if (voiced && isfinite(ss)) {
    float off = 0.f;
    if (lag > a.tau_min && lag < a.tau_max) {
      const float aq = Dp[lag - 1], cq = Dp[lag + 1];
      off = 0.5f * (aq - cq) / ((aq - bq) + (cq - bq));
    }
    f0 = a.sr / ((float)lag + off);
  }
  if (lane == 0) {
    a.f0[o] = f0;
    a.lag[o] = lag;
    a.aper[o] = bq;
    a.energy[o] = sqrtf(ss * (1.f / TT2_YIN_FRAME));   // the correctly rounded root (__fsqrt_rn is the native one)
  }
}

int yin_err(const char* msg) { return tt2_invalid("tt2_yin", msg); }
}  // namespace

extern "C" int tt2_yin(const tt2_yin_args* p, hipStream_t s) {
  if (!p) return yin_err("args required");
  if (!(1 <= p->tau_min && p->tau_min <= p->tau_max && p->tau_max <= TT2_YIN_MAX_LAG))
    return yin_err("lags: 1 <= tau_min <= tau_max <= TT2_YIN_MAX_LAG");
  if (p->hop < 1 || p->utt_stride < 0 || p->batch < 0 || p->t < 0) return yin_err("hop < 1 or negative utt_stride / batch / t");
  if (!(isfinite(p->sr) && p->sr > 0.f && isfinite(p->threshold) && p->threshold > 0.f))
    return yin_err("sr and threshold must be finite and positive");
  if (!p->f0 || !p->lag || !p->aper || !p->energy) return yin_err("f0 / lag / aper / energy required");
  if (p->cmnd && p->cmnd_ld < (int64_t)p->tau_max + 1) return yin_err("cmnd_ld below tau_max + 1");
  if (p->batch == 0 || p->t == 0) return TT2_OK;
  if (!p->x) return yin_err("x required");
  const int groups = (p->t + YIN_NW - 1) / YIN_NW;
  if ((int64_t)groups * p->batch > INT_MAX) return yin_err("batch * t too large for one launch");
  hipLaunchKernelGGL(yin_kernel, dim3((unsigned)(groups * p->batch)), dim3(64 * YIN_NW), 0, s, *p, groups);
  return tt2_check_launch(hipGetLastError(), "tt2_yin");
}
