// pitch_track.hip -- Viterbi pitch tracking over YIN's d' (tt2_pitch_track).  tt2_capi.h states the
// definition.  A translation unit of its own: no other kernel's code depends on it.
#include <math.h>


#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {

// One work group of PT_NW waves per utterance; S = tau_max - tau_min + 1 lag states, state i = lag
// tau_min + i.  V of the previous frame, the pos table of the range and the partial minima live in
// LDS; U is a register that every thread carries (all compute the same value).  A frame is two
// phases with one work-group barrier after each:
//   sweep    every wave holds all the targets (lane l: states l, l + 64, .. l + 64 (K - 1), their
//            pos in registers) and takes its own slice of the sources: PT_NW slices of `chunk`
//            sources (a multiple of 4; the slots past S hold V = +inf, which never wins).  A
//            source's V and pos come as broadcast b128 reads, four sources each; a (source,
//            target) pair costs one subtract, one fma (|.| is an operand modifier) and one min,
//            and the source's V enters the slice's plain minimum (for m[f]) once per wave.  The K
//            partial minima go to the wave's LDS row.
//   combine  thread i < S takes the minimum of the PT_NW partials of state i, forms V[f][i] with
//            the frame's d' (loaded from global before the sweep, so the sweep hides the
//            latency), and writes it to LDS and to the value history; every thread updates U.
// A minimum of f32 values does not depend on the order, so the split changes no bit.  No decision
// is recorded in the sweep: the workspace keeps the values, [t][S + 1] f32 per utterance (V of
// the S states, then U), and the backtrack (wave 0 alone, no barrier) forms the one row of sums
// it needs per frame again, with the same operations, and takes the lowest index of the minimum:
// lane l owns states l K .. l K + K - 1 there, so the lowest lane that holds the minimum holds
// its lowest index.  The lags collect in LDS; all threads then write lag and f0.
constexpr int PT_NW = 16;
constexpr int PT_NT = 64 * PT_NW;
constexpr int PT_SLOTS = 512 + 64;   // PT_NW * chunk <= S + 4 * PT_NW - 1 rounded: see chunk below
static_assert(TT2_YIN_MAX_LAG + 1 <= 512, "K = 8 covers every range");
static_assert(TT2_PITCH_TRACK_MAX_FRAMES <= 4096, "the lags of one utterance fit sLag");

typedef float f32x4_t __attribute__((ext_vector_type(4)));

TT2_DEV float wave_min(float v) {   // every lane ends with the minimum (NaN operands are passed over)
  v = fminf(v, dpp_f32<0xB1>(v));    // quad_perm [1,0,3,2]
  v = fminf(v, dpp_f32<0x4E>(v));    // quad_perm [2,3,0,1]
  v = fminf(v, dpp_f32<0x141>(v));   // row_half_mirror
  v = fminf(v, dpp_f32<0x140>(v));   // row_mirror
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fminf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fminf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

__host__ __device__ constexpr int pt_chunk(int S) { return ((S + PT_NW - 1) / PT_NW + 3) & ~3; }

template <int K>   // targets per lane: 64 K >= S
__global__ __launch_bounds__(PT_NT) void pitch_track_kernel(tt2_pitch_track_args a) {
  __shared__ __attribute__((aligned(16))) float sV[PT_SLOTS];
  __shared__ __attribute__((aligned(16))) float sP[PT_SLOTS];
  __shared__ float sPart[PT_NW][64 * K];
  __shared__ float sMin[PT_NW];
  __shared__ int sLag[TT2_PITCH_TRACK_MAX_FRAMES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  const int S = a.tau_max - a.tau_min + 1;
  int N = a.frames ? a.frames[b] : a.t;
  N = min(max(N, 0), a.t);
  float* f0o = a.f0 + (int64_t)b * a.t;
  int32_t* lago = a.lag + (int64_t)b * a.t;
  if (N == 0) {   // block-uniform
    for (int f = tid; f < a.t; f += PT_NT) f0o[f] = 0.f, lago[f] = -1;
    if (tid == 0) a.cost[b] = 0.f;
    return;
  }
  const float* cm = a.cmnd + (int64_t)b * a.t * a.cmnd_ld + a.tau_min;   // c(f, state i) = cm[f * cmnd_ld + i]
  const int SP = S + 1;
  float* hist = reinterpret_cast<float*>(a.workspace) + (int64_t)b * a.t * SP;
  const float J = a.jump, W = a.switch_cost, C = a.unvoiced;
  const bool own = tid < S;   // the thread combines state tid

  for (int i = tid; i < PT_SLOTS; i += PT_NT) {
    sV[i] = INFINITY;
    sP[i] = i < S ? a.pos[a.tau_min + i] : 0.f;
  }
  __syncthreads();
  float U = C;
  if (own) {
    const float v = cm[tid];
    sV[tid] = v;
    hist[tid] = v;
  }
  if (tid == 0) hist[S] = U;
  float pt[K];
#pragma unroll
  for (int k = 0; k < K; ++k) pt[k] = sP[min(lane + 64 * k, PT_SLOTS - 1)];
  const int chunk = pt_chunk(S);
  const int s0 = w * chunk;
  __syncthreads();

  for (int f = 1; f < N; ++f) {
    const float c = own ? cm[(int64_t)f * a.cmnd_ld + tid] : 0.f;
    // ---- sweep: the wave's slice of sources against every target
    float acc[K], mloc = INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = INFINITY;
    for (int s = s0; s < s0 + chunk; s += 4) {
      const f32x4_t v4 = *reinterpret_cast<const f32x4_t*>(sV + s);
      const f32x4_t p4 = *reinterpret_cast<const f32x4_t*>(sP + s);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        mloc = fminf(mloc, v4[j]);
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = fminf(acc[k], fmaf(J, fabsf(pt[k] - p4[j]), v4[j]));
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) sPart[w][lane + 64 * k] = acc[k];
    if (lane == 0) sMin[w] = mloc;
    __syncthreads();
    // ---- combine
    float m = sMin[0];
#pragma unroll
    for (int q = 1; q < PT_NW; ++q) m = fminf(m, sMin[q]);
    const float uw = U + W, mw = m + W;
    if (own) {
      float A = sPart[0][tid];
#pragma unroll
      for (int q = 1; q < PT_NW; ++q) A = fminf(A, sPart[q][tid]);
      const float v = c + (uw < A ? uw : A);
      sV[tid] = v;
      hist[(int64_t)f * SP + tid] = v;
    }
    U = C + (mw < U ? mw : U);
    if (tid == 0) hist[(int64_t)f * SP + S] = U;
    __syncthreads();
  }

  // ---- the end state and the backtrack: wave 0, lane l on states l K .. l K + K - 1
  if (w == 0) {
    const int i0 = lane * K;
    float pk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) pk[k] = sP[i0 + k];
    // the lowest index of the minimum of x over the states (x of a state >= S is +inf); a NaN
    // never wins, and with no finite value anywhere the answer is state 0: always inside
    auto argmin = [&](const float (&x)[K], float& best) {
      float bv = INFINITY;
      int bi = i0;
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (x[k] < bv) bv = x[k], bi = i0 + k;
      best = wave_min(bv);
      const uint64_t hit = __ballot(bv == best);
      const int src = hit ? __builtin_ctzll(hit) : 0;
      return min(__builtin_amdgcn_readlane(bi, src), S - 1);
    };
    float x[K], best;
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = sV[i0 + k];   // V[N-1]; the slots past S hold +inf
    int st = argmin(x, best);                         // state, -1 = unvoiced
    const bool uv = U < best;
    if (lane == 0) a.cost[b] = uv ? U : best;
    if (uv) st = -1;
    float nx[K], nU;   // row f - 1 of the history, loaded one step ahead
    auto load = [&](int f) {
      const float* h = hist + (int64_t)f * SP;
#pragma unroll
      for (int k = 0; k < K; ++k) nx[k] = i0 + k < S ? h[i0 + k] : INFINITY;
      nU = h[S];
    };
    if (N > 1) load(N - 2);
    for (int f = N - 1; f >= 1; --f) {
      if (lane == 0) sLag[f] = st < 0 ? 0 : a.tau_min + st;
      float Up = nU;
#pragma unroll
      for (int k = 0; k < K; ++k) x[k] = nx[k];
      if (f > 1) load(f - 2);
      if (st >= 0) {   // wave-uniform
        const float ps = sP[st];
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = fmaf(J, fabsf(ps - pk[k]), x[k]);
        const int am = argmin(x, best);
        st = (Up + W < best) ? -1 : am;
      } else {
        const int am = argmin(x, best);
        st = (best + W < Up) ? am : -1;
      }
    }
    if (lane == 0) sLag[0] = st < 0 ? 0 : a.tau_min + st;
  }
  __syncthreads();

  // ---- lag and f0 of every frame
  for (int f = tid; f < a.t; f += PT_NT) {
    int lag = -1;
    float f0 = 0.f;
    if (f < N) {
      lag = sLag[f];
      if (lag > 0) {
        const float* r = a.cmnd + ((int64_t)b * a.t + f) * a.cmnd_ld;
        f0 = a.sr / (float)lag;
        if (lag > a.tau_min && lag < a.tau_max) {
          const float aq = r[lag - 1], bq = r[lag], cq = r[lag + 1];
          if (aq > bq && cq >= bq) {
            const float off = 0.5f * (aq - cq) / ((aq - bq) + (cq - bq));
            f0 = a.sr / ((float)lag + off);
          }
        }
      }
    }
    f0o[f] = f0;
    lago[f] = lag;
  }
}

int pt_err(const char* msg) { return tt2_invalid("tt2_pitch_track", msg); }
bool pt_cost_ok(float x) { return isfinite(x) && x >= 0.f; }
}  // namespace

extern "C" size_t tt2_pitch_track_workspace_size(int batch, int t, int tau_min, int tau_max) {
  if (batch <= 0 || t <= 0 || tau_min < 1 || tau_max < tau_min) return 0;
  return (size_t)batch * t * ((size_t)(tau_max - tau_min) + 2) * sizeof(float);
}

extern "C" int tt2_pitch_track(const tt2_pitch_track_args* p, hipStream_t s) {
  if (!p) return pt_err("args required");
  if (!(1 <= p->tau_min && p->tau_min <= p->tau_max && p->tau_max <= TT2_YIN_MAX_LAG))
    return pt_err("lags: 1 <= tau_min <= tau_max <= TT2_YIN_MAX_LAG");
  if (p->batch < 0 || p->t < 0) return pt_err("negative batch / t");
  if (p->t > TT2_PITCH_TRACK_MAX_FRAMES) return pt_err("t exceeds TT2_PITCH_TRACK_MAX_FRAMES");
  if (p->cmnd_ld < (int64_t)p->tau_max + 1) return pt_err("cmnd_ld below tau_max + 1");
  if (!(isfinite(p->sr) && p->sr > 0.f)) return pt_err("sr must be finite and positive");
  if (!pt_cost_ok(p->jump) || !pt_cost_ok(p->switch_cost) || !pt_cost_ok(p->unvoiced))
    return pt_err("jump / switch_cost / unvoiced must be finite and not negative");
  if (!p->f0 || !p->lag || !p->cost || !p->pos) return pt_err("f0 / lag / cost / pos required");
  if (p->batch == 0) return TT2_OK;
  if (p->t == 0) {
    hipError_t e = hipMemsetAsync(p->cost, 0, sizeof(float) * (size_t)p->batch, s);
    return tt2_check_launch(e, "tt2_pitch_track");
  }
  if (!p->cmnd) return pt_err("cmnd required");
  // (batch, t >= 1 and the lags hold here: the size is never 0)
  const int rc = tt2_need_workspace("tt2_pitch_track", p->workspace, p->workspace_bytes,
                                    tt2_pitch_track_workspace_size(p->batch, p->t, p->tau_min, p->tau_max), 4);
  if (rc != TT2_OK) return rc;
  const int S = p->tau_max - p->tau_min + 1;
  const dim3 grid((unsigned)p->batch), block(PT_NT);
  if (S <= 128) hipLaunchKernelGGL(pitch_track_kernel<2>, grid, block, 0, s, *p);
  else if (S <= 320) hipLaunchKernelGGL(pitch_track_kernel<5>, grid, block, 0, s, *p);
  else hipLaunchKernelGGL(pitch_track_kernel<8>, grid, block, 0, s, *p);
  return tt2_check_launch(hipGetLastError(), "tt2_pitch_track");
}
