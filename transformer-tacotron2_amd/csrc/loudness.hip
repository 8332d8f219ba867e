// loudness.hip -- integrated loudness (ITU-R BS.1770 gating over a two-biquad weighting filter) and
// gain to a target level under a peak ceiling, for a batch of utterances (tt2_loudness).  tt2_capi.h
// states the definition.  A translation unit of its own: no other kernel's code depends on it.
//
// The filter is a linear recurrence along the utterance, evaluated in float64 as a two-level scan.
// A lane owns a chunk of LK_C samples, a wave a segment of 64 chunks.  The state is that of the two
// sections in transposed direct form II, s = (z1, z2, w1, w2), which one sample advances by
// s' = A s + B x; a run of n samples from state s ends in A^n s + (its end state from zero).
//
// Five launches on one stream, no host synchronisation, no work group waiting on another:
//   loud_local    one wave per segment: every lane runs its chunk from zero state, the lanes combine
//                 with A^(C 2^k) (Kogge-Stone over the wave); the segment's zero-state end state and
//                 its max |x| go to the workspace
//   loud_carry    one wave per utterance: the same scan over the segments' end states with
//                 A^(SEG 2^k), 64 segments a round; every segment's true entry state to the workspace
//   loud_energy   one wave per segment: the scan again with lane 0 entering from the true state, every
//                 chunk run again from its true entry state, y^2 to LDS, and one partial sum ("piece")
//                 per sub-block of `step` samples that the segment touches to the workspace
//   loud_final    one work group per utterance: sub-block sums from the pieces in ascending order,
//                 the block sums a tile at a time into LDS, from where one thread adds the gated ones
//                 in ascending order; loudness, peak, gain and the flag
//   loud_apply    y = gain * x, 16-byte stores where y's row allows, zeros past the utterance
// The carry matrices come from the ten coefficients alone, by repeated squaring in float64 on the
// host (lk_powers), and travel as kernel arguments.
#include <limits.h>

#include <algorithm>
#include <cmath>

#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {

constexpr int LK_THREADS = 256;
constexpr int LK_WAVES = LK_THREADS / 64;
constexpr int LK_C = 16;              // samples of a chunk (one lane)
constexpr int LK_SEG = 64 * LK_C;     // samples of a segment (one wave)
constexpr int LK_LD = LK_C + 1;       // doubles per chunk in LDS: 34 dwords apart, so a wave's ds_read_b64
                                      // of one sample per chunk meets no bank twice in a half wave
constexpr int LK_NPOW = 12;           // A^(C 2^k), k = 0 .. 11: 0 .. 5 the chunk scan, 6 .. 11 the segment scan
constexpr int LK_TILE = 1024;          // block sums that the last launch holds in LDS at a time
constexpr int LK_ACOLS = 4 * LK_THREADS;   // apply: columns of a work group per trip
constexpr int LK_ACHUNKS = 256;       // apply: work groups per utterance at most

struct lk_plan {
  double m[LK_NPOW][16];   // m[k] = A^(LK_C * 2^k), row-major
  int nseg;                // segments per utterance, ceil(n_in / LK_SEG)
  int npiece;              // pieces per segment, min(LK_SEG, (LK_SEG - 1) / step + 2)
  int nsub;                // sub-block sums per utterance, n_in / step
  int ach;                 // work groups per utterance of the apply
  float* gain;             // [batch]
  float* speak;            // [batch][nseg]     max |x| of a segment
  double* state;           // [batch][nseg][4]  zero-state end state, then the true entry state
  double* piece;           // [batch][nseg][npiece]
  double* sub;             // [batch][nsub]
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

TT2_DEV int lk_len(const tt2_loudness_args& a, int b) {
  const int len = a.lens ? a.lens[b] : a.n_in;
  return min(max(len, 0), a.n_in);
}

// o = add + m[.][0] v0 + m[.][1] v1 + m[.][2] v2 + m[.][3] v3, one fma per term in that order
TT2_DEV void lk_mv(const double (&m)[16], const double (&v)[4], const double (&add)[4], double (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    o[r] = fma(m[4 * r + 3], v[3], fma(m[4 * r + 2], v[2], fma(m[4 * r + 1], v[1], fma(m[4 * r], v[0], add[r]))));
}

// Both sections over nc samples at p (LDS), from state s to the end state in s.  k = b0 b1 b2 a1 a2 of
// section 1, then of section 2.  WRITE: the squared output replaces the sample.
template <bool WRITE>
TT2_DEV void lk_run(double* p, int nc, const double (&k)[10], double (&s)[4]) {
  double z1 = s[0], z2 = s[1], w1 = s[2], w2 = s[3];
  auto sample = [&](double x) {
    const double y1 = fma(k[0], x, z1);
    z1 = fma(k[1], x, fma(-k[3], y1, z2));
    z2 = fma(-k[4], y1, k[2] * x);
    const double y2 = fma(k[5], y1, w1);
    w1 = fma(k[6], y1, fma(-k[8], y2, w2));
    w2 = fma(-k[9], y2, k[7] * y1);
    return y2 * y2;
  };
  if (nc == LK_C) {                   // a whole chunk: the LDS reads go out together, the arithmetic is the same
    double x[LK_C];
#pragma unroll
    for (int i = 0; i < LK_C; ++i) x[i] = p[i];
#pragma unroll
    for (int i = 0; i < LK_C; ++i) {
      const double q = sample(x[i]);
      if (WRITE) p[i] = q;
    }
  } else {
    for (int i = 0; i < nc; ++i) {
      const double q = sample(p[i]);
      if (WRITE) p[i] = q;
    }
  }
  s[0] = z1, s[1] = z2, s[2] = w1, s[3] = w2;
}

// Inclusive scan over the wave: lane l ends with the end state of the run of lanes 0 .. l, each lane's
// own part given in e, a lane's part spanning as many samples as m[K0] advances.
template <int K0>
TT2_DEV void lk_scan(const lk_plan& pl, int lane, double (&e)[4]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double t[4], o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) t[r] = __shfl_up(e[r], 1 << k, 64);
    lk_mv(pl.m[K0 + k], t, e, o);
    if (lane >= (1 << k)) {
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = o[r];
    }
  }
}

TT2_DEV double lk_wave_sum(double v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Samples p[0 .. n) of a segment into LDS as doubles, chunk c at s + c * LK_LD; returns the lane's
// max |x| over what it loaded.  16-byte loads where p allows; the values are the same either way.
TT2_DEV float lk_fill(double* s, const float* p, int n, int lane) {
  float pk = 0.f;
  const bool vec = (reinterpret_cast<uintptr_t>(p) & 15) == 0;   // wave-uniform
  auto slot = [&](int i) { return s + (i / LK_C) * LK_LD + i % LK_C; };
  if (n == LK_SEG && vec) {           // a whole segment: the four loads of a lane go out together
    f32x4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const f32x4*>(p + 4 * lane + 256 * q);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double* d = slot(4 * lane + 256 * q);
      d[0] = v[q].x, d[1] = v[q].y, d[2] = v[q].z, d[3] = v[q].w;
      pk = fmaxf(fmaxf(pk, fmaxf(fabsf(v[q].x), fabsf(v[q].y))), fmaxf(fabsf(v[q].z), fabsf(v[q].w)));
    }
  } else if (n == LK_SEG) {
    float v[LK_C];
#pragma unroll
    for (int q = 0; q < LK_C; ++q) v[q] = p[lane + 64 * q];
#pragma unroll
    for (int q = 0; q < LK_C; ++q) *slot(lane + 64 * q) = v[q], pk = fmaxf(pk, fabsf(v[q]));
  } else if (vec) {
    for (int i = 4 * lane; i < n; i += 256) {
      double* d = slot(i);                               // i % 4 == 0: the four stay in one chunk
      if (i + 4 <= n) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + i);
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        pk = fmaxf(fmaxf(pk, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
      } else {
        for (int q = 0; i + q < n; ++q) d[q] = p[i + q], pk = fmaxf(pk, fabsf(p[i + q]));
      }
    }
  } else {
    for (int i = lane; i < n; i += 64) {
      const float v = p[i];
      *slot(i) = v;
      pk = fmaxf(pk, fabsf(v));
    }
  }
  return pk;
}

// Which segment this wave has, and how many valid samples n of it (0: none, or no such segment)
struct lk_where { int b, seg, n; int64_t s0; };
TT2_DEV lk_where lk_locate(const tt2_loudness_args& a, const lk_plan& pl) {
  lk_where w;
  const int64_t gw = (int64_t)blockIdx.x * LK_WAVES + (threadIdx.x >> 6);
  const bool valid = gw < (int64_t)a.batch * pl.nseg;
  w.b = valid ? (int)(gw / pl.nseg) : 0;
  w.seg = valid ? (int)(gw % pl.nseg) : 0;
  w.s0 = (int64_t)w.seg * LK_SEG;
  w.n = valid ? (int)min((int64_t)LK_SEG, max((int64_t)0, (int64_t)lk_len(a, w.b) - w.s0)) : 0;
  return w;
}

__global__ __launch_bounds__(LK_THREADS) void loud_local(tt2_loudness_args a, lk_plan pl) {
  __shared__ double sd[LK_WAVES][64 * LK_LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const lk_where at = lk_locate(a, pl);
  float pk = 0.f;
  if (at.n > 0) pk = lk_fill(sd[w], a.x + (int64_t)at.b * a.x_ld + at.s0, at.n, lane);
  __syncthreads();
  if (at.n > 0) {
    double e[4] = {0., 0., 0., 0.};
    lk_run<false>(sd[w] + lane * LK_LD, min(max(at.n - lane * LK_C, 0), LK_C), a.coef, e);
    lk_scan<0>(pl, lane, e);
    const int64_t sg = (int64_t)at.b * pl.nseg + at.seg;
    if (lane == 63) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pl.state[4 * sg + r] = e[r];
    }
    pk = wave_max(pk);
    if (lane == 0) pl.speak[sg] = pk;
  }
}

// One wave per utterance.  state[b][seg] holds the zero-state end state of segment seg on entry and
// the state at its first sample on exit.  Only an end state of a full segment is ever used.
__global__ __launch_bounds__(64) void loud_carry(tt2_loudness_args a, lk_plan pl) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int len = lk_len(a, b);
  const int nsegb = (int)(((int64_t)len + LK_SEG - 1) / LK_SEG);
  double* st = pl.state + (int64_t)b * pl.nseg * 4;
  double in[4] = {0., 0., 0., 0.};                     // the state entering this round's first segment
  for (int base = 0; base < nsegb; base += 64) {
    const int seg = base + lane;
    double e[4] = {0., 0., 0., 0.};
    if (seg < nsegb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = st[4 * (int64_t)seg + r];
    }
    if (lane == 0) {
      double o[4];
      lk_mv(pl.m[6], in, e, o);
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = o[r];
    }
    lk_scan<6>(pl, lane, e);
    double entry[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double up = __shfl_up(e[r], 1, 64);
      entry[r] = lane == 0 ? in[r] : up;
      in[r] = __shfl(e[r], 63, 64);
    }
    if (seg < nsegb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) st[4 * (int64_t)seg + r] = entry[r];
    }
  }
}

__global__ __launch_bounds__(LK_THREADS) void loud_energy(tt2_loudness_args a, lk_plan pl) {
  __shared__ double sd[LK_WAVES][64 * LK_LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const lk_where at = lk_locate(a, pl);
  const int64_t sg = (int64_t)at.b * pl.nseg + at.seg;
  if (at.n > 0) lk_fill(sd[w], a.x + (int64_t)at.b * a.x_ld + at.s0, at.n, lane);
  __syncthreads();
  if (at.n > 0) {
    const int nc = min(max(at.n - lane * LK_C, 0), LK_C);
    double in[4], e[4], entry[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) in[r] = pl.state[4 * sg + r], e[r] = lane == 0 ? in[r] : 0.;
    lk_run<false>(sd[w] + lane * LK_LD, nc, a.coef, e);
    lk_scan<0>(pl, lane, e);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double up = __shfl_up(e[r], 1, 64);
      entry[r] = lane == 0 ? in[r] : up;
    }
    lk_run<true>(sd[w] + lane * LK_LD, nc, a.coef, entry);
  }
  __syncthreads();
  if (at.n > 0) {
    // piece (seg, j): y^2 over the samples of sub-block j inside this segment; sample i of them belongs
    // to lane (i - first) mod 64, a lane adds its own from +0 ascending, then the xor tree
    const int64_t j0 = at.s0 / a.step, j1 = (at.s0 + at.n - 1) / a.step;
    double* out = pl.piece + sg * pl.npiece;
    for (int64_t j = j0; j <= j1; ++j) {
      const int lo = (int)(max(j * a.step, at.s0) - at.s0);
      const int hi = (int)(min((j + 1) * a.step, at.s0 + at.n) - at.s0);
      double acc = 0.;
      for (int i = lo + lane; i < hi; i += 64) acc += sd[w][(i / LK_C) * LK_LD + i % LK_C];
      acc = lk_wave_sum(acc);
      if (lane == 0) out[j - j0] = acc;
    }
  }
}

__global__ __launch_bounds__(LK_THREADS) void loud_final(tt2_loudness_args a, lk_plan pl) {
  __shared__ float sf[LK_WAVES];
  __shared__ double se[LK_TILE];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = lk_len(a, b);
  const int S = len / a.step;
  const int nsegb = (int)(((int64_t)len + LK_SEG - 1) / LK_SEG);
  double* sub = pl.sub + (int64_t)b * pl.nsub;
  const double* pc = pl.piece + (int64_t)b * pl.nseg * pl.npiece;
  float* erow = a.energy ? a.energy + (int64_t)b * a.energy_ld : nullptr;
  for (int j = tid; j < S; j += LK_THREADS) {
    const int64_t lo = (int64_t)j * a.step, hi = lo + a.step;
    double acc = 0.;
    for (int64_t seg = lo / LK_SEG; seg <= (hi - 1) / LK_SEG; ++seg)
      acc += pc[seg * pl.npiece + (j - seg * LK_SEG / a.step)];
    sub[j] = acc;
    if (erow) erow[j] = (float)acc;
  }
  if (erow) {
    for (int j = S + tid; j <= pl.nsub; j += LK_THREADS) erow[j] = 0.f;
  }
  float pk = 0.f;
  for (int seg = tid; seg < nsegb; seg += LK_THREADS) pk = fmaxf(pk, pl.speak[(int64_t)b * pl.nseg + seg]);
  pk = wave_max(pk);
  if ((tid & 63) == 0) sf[tid >> 6] = pk;
  __syncthreads();                                      // also: sub[] of every thread is visible
  pk = fmaxf(fmaxf(sf[0], sf[1]), fmaxf(sf[2], sf[3]));
  // The gates add in ascending order, so one thread adds; the others put the block sums of a tile
  // into LDS for it (from global memory the 2 N dependent trips cost 29 us of this launch's 30 at
  // N = 89).  Pass 0 is the absolute gate, pass 1 both; a block sum is formed the same
  // way both times, so both passes see the same bits.
  const int N = max(0, S - 3);
  double sum = 0., thr = 0., ms = 0.;
  int64_t cnt = 0;
  bool measured = false;
  for (int pass = 0; pass < 2; ++pass) {
    for (int base = 0; base < N; base += LK_TILE) {
      const int m = min(LK_TILE, N - base);
      if (pass == 0 || N > LK_TILE) {                   // a single tile is still there in pass 1
        __syncthreads();
        for (int i = tid; i < m; i += LK_THREADS) {
          const double* q = sub + base + i;
          se[i] = ((q[0] + q[1]) + q[2]) + q[3];
        }
        __syncthreads();
      }
      if (tid == 0) {
        for (int i = 0; i < m; ++i) {
          const double E = se[i];
          if (E > a.abs_sum && (pass == 0 || E > thr)) sum += E, ++cnt;
        }
      }
    }
    if (pass == 0) {
      // (no early exit: only thread 0 counts, and every thread has to reach pass 1's barriers)
      thr = cnt > 0 ? a.rel_ratio * (sum / (double)cnt) : (double)INFINITY;
      sum = 0., cnt = 0;
    } else if (cnt > 0) {
      measured = true, ms = (sum / (double)cnt) / (4.0 * (double)a.step);
    }
  }
  if (tid != 0) return;
  float g = 1.f, loud = -INFINITY;
  int limited = 0;
  if (measured) {
    loud = (float)(-0.691 + 10.0 * log10(ms));
    double gd = sqrt(a.target_ms / ms);
    if (pk > 0.f) {
      const double c = (double)a.ceiling / (double)pk;
      if (c < gd) gd = c, limited = 1;
    }
    g = (float)gd;
  }
  pl.gain[b] = g;
  if (a.loud) a.loud[b] = loud;
  if (a.gain) a.gain[b] = g;
  if (a.peak) a.peak[b] = pk;
  if (a.limited) a.limited[b] = limited;
}

// Columns in groups of four on 16-byte boundaries of y's row, as trim_copy has them: a whole group
// inside [0, n_out) is one 16-byte store, and one 16-byte load where x's row is aligned like y's.
__global__ __launch_bounds__(LK_THREADS) void loud_apply(tt2_loudness_args a, lk_plan pl) {
  const int b = blockIdx.x / (unsigned)pl.ach;
  const int c = blockIdx.x % (unsigned)pl.ach;
  const float g = pl.gain[b];
  const int outb = min(lk_len(a, b), a.n_out);
  const float* src = a.x + (int64_t)b * a.x_ld;
  float* yrow = a.y + (int64_t)b * a.y_ld;
  const int m = (int)((reinterpret_cast<uintptr_t>(yrow) >> 2) & 3);
  const bool vec = ((reinterpret_cast<uintptr_t>(src) >> 2) & 3) == (unsigned)m;
  const int64_t ngroups = ((int64_t)a.n_out + m + 3) / 4;
  for (int64_t q = (int64_t)c * LK_THREADS + threadIdx.x; q < ngroups; q += (int64_t)pl.ach * LK_THREADS) {
    const int64_t i0 = 4 * q - m;
    if (i0 >= 0 && i0 + 4 <= a.n_out) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (i0 + 4 <= outb) {
        if (vec) {
          v = *reinterpret_cast<const f32x4*>(src + i0);
        } else {
          v.x = src[i0], v.y = src[i0 + 1], v.z = src[i0 + 2], v.w = src[i0 + 3];
        }
        v.x = __fmul_rn(g, v.x), v.y = __fmul_rn(g, v.y), v.z = __fmul_rn(g, v.z), v.w = __fmul_rn(g, v.w);
      } else if (i0 < outb) {
        v.x = __fmul_rn(g, src[i0]);
        if (i0 + 1 < outb) v.y = __fmul_rn(g, src[i0 + 1]);
        if (i0 + 2 < outb) v.z = __fmul_rn(g, src[i0 + 2]);
      }
      *reinterpret_cast<f32x4*>(yrow + i0) = v;
    } else {
      for (int64_t i = max(i0, (int64_t)0); i < min(i0 + 4, (int64_t)a.n_out); ++i)
        yrow[i] = i < outb ? __fmul_rn(g, src[i]) : 0.f;
    }
  }
}

int lk_err(const char* msg) { return tt2_invalid("tt2_loudness", msg); }

size_t lk_up16(size_t n) { return (n + 15) & ~(size_t)15; }

struct lk_sizes { size_t nseg, npiece, nsub, gain, speak, state, piece, sub; };
lk_sizes lk_layout(int batch, int n_in, int step) {
  lk_sizes z;
  z.nseg = ((size_t)n_in + LK_SEG - 1) / LK_SEG;
  z.npiece = std::min<size_t>(LK_SEG, (size_t)(LK_SEG - 1) / step + 2);
  z.nsub = (size_t)n_in / step;
  z.gain = lk_up16((size_t)batch * sizeof(float));
  z.speak = lk_up16((size_t)batch * z.nseg * sizeof(float));
  z.state = (size_t)batch * z.nseg * 4 * sizeof(double);
  z.piece = lk_up16((size_t)batch * z.nseg * z.npiece * sizeof(double));
  z.sub = lk_up16((size_t)batch * z.nsub * sizeof(double));
  return z;
}

// The one-sample matrix of the two sections in transposed direct form II (state z1 z2 w1 w2; section
// 2 reads y1 = b0 x + z1), and m[k] = A^(LK_C 2^k) by repeated squaring, each product a plain
// row-by-column sum in ascending index order.
void lk_powers(const double (&k)[10], double (*m)[16]) {
  double p[16] = {-k[3], 1., 0., 0.,
                  -k[4], 0., 0., 0.,
                  k[6] - k[8] * k[5], 0., -k[8], 1.,
                  k[7] - k[9] * k[5], 0., -k[9], 0.};
  auto square = [](double (&q)[16]) {
    double o[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) {
        double s = 0.;
        for (int i = 0; i < 4; ++i) s += q[4 * r + i] * q[4 * i + c];
        o[4 * r + c] = s;
      }
    std::copy(o, o + 16, q);
  };
  for (int c = 1; c < LK_C; c <<= 1) square(p);
  for (int i = 0; i < LK_NPOW; ++i) {
    std::copy(p, p + 16, m[i]);
    square(p);
  }
}
}  // namespace

extern "C" size_t tt2_loudness_workspace_size(int batch, int n_in, int step) {
  if (batch <= 0 || n_in < 0 || step < 1) return 0;
  const lk_sizes z = lk_layout(batch, n_in, step);
  return z.gain + z.speak + z.state + z.piece + z.sub;
}

extern "C" int tt2_loudness(const tt2_loudness_args* p, hipStream_t s) {
  if (!p) return lk_err("args required");
  if (p->step < 1) return lk_err("step < 1");
  if (4 * (int64_t)p->step > INT_MAX) return lk_err("the block length 4 * step overflows int32");
  if (p->batch < 0 || p->n_in < 0 || p->n_out < 0) return lk_err("negative batch / n_in / n_out");
  if (p->x_ld < p->n_in) return lk_err("x_ld < n_in");
  if (p->y && p->y_ld < p->n_out) return lk_err("y_ld < n_out");
  if (p->energy && p->energy_ld < (int64_t)p->n_in / p->step + 1) return lk_err("energy_ld < n_in / step + 1");
  for (double c : p->coef)
    if (!std::isfinite(c)) return lk_err("a coefficient is not finite");
  if (!std::isfinite(p->abs_sum) || p->abs_sum < 0.) return lk_err("abs_sum must be finite and not negative");
  if (!(p->rel_ratio >= 0. && p->rel_ratio <= 1.)) return lk_err("rel_ratio must be in [0, 1]");
  if (!std::isfinite(p->target_ms) || p->target_ms <= 0.) return lk_err("target_ms must be finite and positive");
  if (!std::isfinite(p->ceiling) || p->ceiling <= 0.f) return lk_err("ceiling must be finite and positive");
  if (!p->y && !p->loud && !p->gain && !p->peak && !p->limited && !p->energy) return lk_err("every output is null");
  if (!p->x && p->batch > 0 && p->n_in > 0) return lk_err("x required");
  const size_t need = tt2_loudness_workspace_size(p->batch, p->n_in, p->step);
  if (need && (!p->workspace || p->workspace_bytes < need)) return lk_err("workspace below tt2_loudness_workspace_size");
  lk_plan pl;
  const lk_sizes z = lk_layout(std::max(p->batch, 1), p->n_in, p->step);
  pl.nseg = (int)z.nseg, pl.npiece = (int)z.npiece, pl.nsub = (int)z.nsub;
  pl.ach = std::max(1, (int)std::min<int64_t>(LK_ACHUNKS, ((int64_t)p->n_out + 3 + LK_ACOLS - 1) / LK_ACOLS));
  const int64_t segwg = ((int64_t)p->batch * pl.nseg + LK_WAVES - 1) / LK_WAVES;
  if (std::max(segwg, (int64_t)p->batch * pl.ach) > INT_MAX) return lk_err("more than 2^31 - 1 work groups");
  if (p->batch == 0) return TT2_OK;
  char* ws = static_cast<char*>(p->workspace);
  pl.gain = reinterpret_cast<float*>(ws);
  pl.speak = reinterpret_cast<float*>(ws + z.gain);
  pl.state = reinterpret_cast<double*>(ws + z.gain + z.speak);
  pl.piece = reinterpret_cast<double*>(ws + z.gain + z.speak + z.state);
  pl.sub = reinterpret_cast<double*>(ws + z.gain + z.speak + z.state + z.piece);
  lk_powers(p->coef, pl.m);
  int rc;
  if (pl.nseg > 0) {
    hipLaunchKernelGGL(loud_local, dim3((unsigned)segwg), dim3(LK_THREADS), 0, s, *p, pl);
    if ((rc = tt2_check_launch(hipGetLastError(), "tt2_loudness (chunk scan)")) != TT2_OK) return rc;
    hipLaunchKernelGGL(loud_carry, dim3((unsigned)p->batch), dim3(64), 0, s, *p, pl);
    if ((rc = tt2_check_launch(hipGetLastError(), "tt2_loudness (segment scan)")) != TT2_OK) return rc;
    hipLaunchKernelGGL(loud_energy, dim3((unsigned)segwg), dim3(LK_THREADS), 0, s, *p, pl);
    if ((rc = tt2_check_launch(hipGetLastError(), "tt2_loudness (energies)")) != TT2_OK) return rc;
  }
  hipLaunchKernelGGL(loud_final, dim3((unsigned)p->batch), dim3(LK_THREADS), 0, s, *p, pl);
  if ((rc = tt2_check_launch(hipGetLastError(), "tt2_loudness (gates)")) != TT2_OK) return rc;
  if (p->y && p->n_out > 0) {
    hipLaunchKernelGGL(loud_apply, dim3((unsigned)(p->batch * pl.ach)), dim3(LK_THREADS), 0, s, *p, pl);
    return tt2_check_launch(hipGetLastError(), "tt2_loudness (gain)");
  }
  return TT2_OK;
}
