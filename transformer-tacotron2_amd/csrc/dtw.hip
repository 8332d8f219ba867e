// dtw.hip -- dynamic time warping between two f32 feature sequences per utterance (tt2_dtw; the
// alignment under mel-cepstral distortion).  tt2_capi.h states the definition.  A translation
// unit of its own: no other kernel's code depends on it.
#include <math.h>


#include "tt2_capi.h"
#include "tt2_internal.h"
#include "tt2_common.h"

namespace {

// One work group per utterance pair, a wavefront of tiles.  Wave w owns the band of 64 * CPL
// columns of b that starts at w * 64 * CPL (lane l: columns l * CPL .. l * CPL + CPL - 1, their
// features in registers); a tile is RB rows of a by one band.  At stage st wave w works on row
// block st - w, so the tile to its left was finished one stage earlier by wave w - 1, which left
// its right-edge column (D and path length) in the edge array of that stage's parity; one
// work-group barrier per stage.  A tile has two phases:
//   costs   every lane forms the RB costs of its columns with the row of a broadcast from lane
//           registers (v_readlane), so the expensive part runs with all lanes busy, and writes
//           them to the wave's own LDS tile;
//   DP      the lanes run skewed, lane l on row s - l at tick s.  Left's D comes over one DPP wave
//           shift per tick (lane 0 takes the edge array's value), the diagonal is the value received
//           the tick before and up is the lane's own previous value: every cell is the sequential
//           f32 recurrence of the definition.
// Move codes (0 diagonal, 1 up, 2 left; 2 bits) collect in lane registers over a tile's rows and
// go to the workspace after the tile, 16 rows of one column per word, [row / 16][column].  The backtrack copies as many
// 16-row bands of words (columns 0 .. j) into LDS as fit, walks them with one thread until the
// path leaves them, and repeats.
constexpr int DTW_NW = 16;             // waves: 16 * 64 * 2 = TT2_DTW_MAX_FRAMES columns
constexpr int DTW_NT = 64 * DTW_NW;
constexpr int DTW_TILE = 2048;         // floats per wave's cost tile: RB * 64 * CPL
constexpr int DTW_MR = 16;             // rows per move word
static_assert(DTW_NW * 128 >= TT2_DTW_MAX_FRAMES, "bands cover the columns");
static_assert(DTW_NW * DTW_TILE >= TT2_DTW_MAX_FRAMES, "one band of move words fits the tiles");

__host__ __device__ constexpr int dtw_cpl(int tb) { return tb > 64 * DTW_NW ? 2 : 1; }

typedef float f32x2 __attribute__((ext_vector_type(2)));

TT2_DEV float shr1(float x, float first) {   // lane l <- lane l - 1 (wave_shr:1); lane 0 <- first
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(first), __float_as_int(x), 0x138, 0xF, 0xF, false));
}
TT2_DEV int shr1(int x, int first) { return __builtin_amdgcn_update_dpp(first, x, 0x138, 0xF, 0xF, false); }
TT2_DEV float lane_f(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }

template <int CPL, int NF>   // columns per lane, feature capacity (c1 - c0 rounded up; the rest are zeros)
__global__ __launch_bounds__(DTW_NT) void dtw_kernel(tt2_dtw_args a) {
  constexpr int RB = 32 / CPL;           // rows per tile
  constexpr int W = 64 * CPL;            // columns per band
  constexpr int NREG = RB * NF / 64;     // a tile's rows of a, spread over the lanes
  constexpr int RPR = 64 / NF;           // rows of a per such register
  constexpr bool PK = CPL * NF <= 32;    // packed-f32 costs (they hold b's features twice: not at 2 x 32)
  static_assert(RB * W == DTW_TILE && RB % DTW_MR == 0 && RB <= 32, "tile shape");
  __shared__ __attribute__((aligned(16))) float sC[DTW_NW * DTW_TILE];
  __shared__ float sED[2][DTW_NW][32];
  __shared__ int sEL[2][DTW_NW][32];
  __shared__ int sWalk[4];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  int Na = a.ta, Nb = a.tb;
  if (a.a_len) Na = min(Na, a.a_len[b]);
  if (a.b_len) Nb = min(Nb, a.b_len[b]);
  Na = Na < 0 ? 0 : Na;
  Nb = Nb < 0 ? 0 : Nb;
  const int np = a.ta + a.tb - 1;
  const bool want = a.path_a != nullptr;
  int32_t* pa = want ? a.path_a + (int64_t)b * np : nullptr;
  int32_t* pb = want ? a.path_b + (int64_t)b * np : nullptr;
  if (Na == 0 || Nb == 0) {   // block-uniform
    if (tid == 0) {
      a.total[b] = 0.f;
      a.length[b] = 0;
    }
    if (want)
      for (int k = tid; k < np; k += blockDim.x) pa[k] = pb[k] = -1;
    return;
  }
  const int nf = a.c1 - a.c0;
  const float* A = a.a + (int64_t)b * a.ta * a.a_ld + a.c0;
  const float* Bp = a.b + (int64_t)b * a.tb * a.b_ld + a.c0;
  uint32_t* mv = reinterpret_cast<uint32_t*>(a.workspace) + (int64_t)b * ((a.ta + DTW_MR - 1) / DTW_MR) * a.tb;
  const int nI = (Na + RB - 1) / RB, nJ = (Nb + W - 1) / W;
  const int col0 = w * W + lane * CPL;

  float fb[CPL][NF];
#pragma unroll
  for (int q = 0; q < CPL; ++q)
#pragma unroll
    for (int k = 0; k < NF; ++k) fb[q][k] = (col0 + q < Nb && k < nf) ? Bp[(int64_t)(col0 + q) * a.b_ld + k] : 0.f;

  float D[CPL];   // the lane's columns at the last row it finished (up for the next)
  int Ln[CPL];    // and the path lengths there
#pragma unroll
  for (int q = 0; q < CPL; ++q) D[q] = INFINITY, Ln[q] = 0;
  // left's value one tick ago (the diagonal), and lane 0's across tiles.  Cell (0, 0) takes a
  // virtual diagonal of D = 0, L = 0 (up and left are +inf there), so it needs no special case.
  float pD = INFINITY, carryD = w == 0 ? 0.f : INFINITY;
  int pL = 0, carryL = 0;
  float* T = sC + w * DTW_TILE;

  for (int st = 0; st < nI + nJ - 1; ++st) {
    const int I = st - w;
    if (w < nJ && I >= 0 && I < nI) {   // wave-uniform
      const int r0 = I * RB;
      // ---- costs of the tile
      float av[NREG];
#pragma unroll
      for (int m = 0; m < NREG; ++m) {
        const int e = lane + 64 * m, row = r0 + e / NF, k = e % NF;
        av[m] = (row < Na && k < nf) ? A[(int64_t)row * a.a_ld + k] : 0.f;
      }
#pragma unroll
      for (int m = 0; m < NREG; ++m) {
        if constexpr (!PK) {
#pragma nounroll
          for (int rr = 0; rr < RPR; ++rr) {
            float acc[CPL];
#pragma unroll
            for (int q = 0; q < CPL; ++q) acc[q] = 0.f;
#pragma unroll
            for (int k = 0; k < NF; ++k) {
              const float ak = lane_f(av[m], rr * NF + k);
#pragma unroll
              for (int q = 0; q < CPL; ++q) {
                const float d = ak - fb[q][k];
                acc[q] = fmaf(d, d, acc[q]);
              }
            }
#pragma unroll
            for (int q = 0; q < CPL; ++q) T[(m * RPR + rr) * W + lane * CPL + q] = __fsqrt_rn(acc[q]);
          }
          continue;
        }
#pragma nounroll
        for (int rr = 0; rr < RPR; rr += 2) {   // two rows at a time: packed f32 subtract and fma
          f32x2 acc[CPL];
#pragma unroll
          for (int q = 0; q < CPL; ++q) acc[q] = f32x2{0.f, 0.f};
#pragma unroll
          for (int k = 0; k < NF; ++k) {
            const f32x2 ak = {lane_f(av[m], rr * NF + k), lane_f(av[m], (rr + 1) * NF + k)};
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
              const f32x2 d = ak - f32x2{fb[q][k], fb[q][k]};
              acc[q] = __builtin_elementwise_fma(d, d, acc[q]);
            }
          }
#pragma unroll
          for (int q = 0; q < CPL; ++q) {
            T[(m * RPR + rr) * W + lane * CPL + q] = __fsqrt_rn(acc[q].x);
            T[(m * RPR + rr + 1) * W + lane * CPL + q] = __fsqrt_rn(acc[q].y);
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

      // ---- the recurrence, skewed over the lanes
      float eD = INFINITY;   // lane r: the left band's edge at row r0 + r
      int eL = 0;
      if (w > 0 && lane < RB) {
        eD = sED[(st - 1) & 1][w - 1][lane];
        eL = sEL[(st - 1) & 1][w - 1][lane];
      }
      if (lane == 0) pD = carryD, pL = carryL;
      uint64_t bits[CPL];   // the tile's move codes of the lane's columns, shifted in from the top
#pragma unroll
      for (int q = 0; q < CPL; ++q) bits[q] = 0;
      auto costs = [&](float (&c)[CPL], int s) {   // of the lane's cells at tick s (row clamped into the tile)
        const float* p = T + min(max(s - lane, 0), RB - 1) * W + lane * CPL;
        if constexpr (CPL == 2) {
          const float2 x = *reinterpret_cast<const float2*>(p);
          c[0] = x.x, c[1] = x.y;
        } else {
          c[0] = p[0];
        }
      };
      float cc[CPL], cn[CPL];
      costs(cc, 0);
      for (int s = 0; s < RB + 63; ++s) {
        costs(cn, s + 1);   // read one tick ahead of the chain
        const int se = min(s, RB - 1);
        const float lD = shr1(D[CPL - 1], lane_f(eD, se));
        const int lL = shr1(Ln[CPL - 1], __builtin_amdgcn_readlane(eL, se));
        const int r = s - lane, row = r0 + r;
        if (r >= 0 && r < RB && row < Na) {
          float dD = pD, xD = lD;   // diagonal and left of the lane's first column
          int dL = pL, xL = lL;
#pragma unroll
          for (int q = 0; q < CPL; ++q) {
            const float c = cc[q];
            const float uD = D[q];
            const int uL = Ln[q];
            const bool dg = dD <= uD && dD <= xD;
            const bool up = uD <= xD;
            float best = dg ? dD : up ? uD : xD;
            int len = dg ? dL : up ? uL : xL;
            const uint64_t code = dg ? 0u : up ? 1u : 2u;
            D[q] = c + best;
            Ln[q] = len + 1;
            bits[q] = (bits[q] >> 2) | (code << 62);
            dD = uD, dL = uL;       // the next column's diagonal and left
            xD = D[q], xL = Ln[q];
          }
          if (lane == 63) {
            sED[st & 1][w][r] = D[CPL - 1];
            sEL[st & 1][w][r] = Ln[CPL - 1];
          }
        }
        pD = lD, pL = lL;
#pragma unroll
        for (int q = 0; q < CPL; ++q) cc[q] = cn[q];
      }
      if (want) {   // the tile's rows down to bit 0, 16 rows per word; lanes write neighbouring columns
        const int nr = min(RB, Na - r0);
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
          const uint64_t x = bits[q] >> (64 - 2 * nr);
          if (col0 + q < Nb) {
            uint32_t* o = mv + (int64_t)(r0 / DTW_MR) * a.tb + col0 + q;
            o[0] = (uint32_t)x;
            if (RB > DTW_MR && nr > DTW_MR) o[a.tb] = (uint32_t)(x >> 32);
          }
        }
      }
      carryD = lane_f(eD, RB - 1);
      carryL = __builtin_amdgcn_readlane(eL, RB - 1);
    }
    __syncthreads();
  }

  // ---- D and L of the end cell sit in the registers of the lane that owns column Nb - 1
  if (col0 / CPL == (Nb - 1) / CPL) {
    const int q = (Nb - 1) % CPL;
    const float d = q == 0 ? D[0] : D[CPL - 1];
    const int l = q == 0 ? Ln[0] : Ln[CPL - 1];
    a.total[b] = d;
    a.length[b] = l;
    sWalk[0] = l;
  }
  if (!want) return;   // block-uniform
  __threadfence_block();
  __syncthreads();

  // ---- backtrack: one 16-row band of move words at a time through LDS (the tiles are free now)
  uint32_t* sM = reinterpret_cast<uint32_t*>(sC);
  const int L = min(sWalk[0], np);
  for (int k = L + tid; k < np; k += blockDim.x) pa[k] = pb[k] = -1;
  int i = Na - 1, j = Nb - 1, k = L - 1;
  while (i >= 0) {   // block-uniform
    // as many 16-row bands of words, columns 0 .. j, as the tiles' LDS holds
    const int band = i / DTW_MR, wd = j + 1;
    const int lo = band + 1 - min(band + 1, DTW_NW * DTW_TILE / wd);
    for (int c = tid; c < (band + 1 - lo) * wd; c += blockDim.x) {
      const int bb = c / wd;
      sM[c] = mv[(int64_t)(lo + bb) * a.tb + (c - bb * wd)];
    }
    __syncthreads();
    if (tid == 0) {
      while (k >= 0) {
        pa[k] = i;
        pb[k] = j;
        --k;
        if (i == 0 && j == 0) {
          i = -1;
          break;
        }
        uint32_t code = (sM[(i / DTW_MR - lo) * wd + j] >> (2 * (i & (DTW_MR - 1)))) & 3u;
        if (i == 0) code = 2;        // (what the recurrence chose there anyway; keeps the walk inside)
        else if (j == 0) code = 1;
        if (code != 2) --i;
        if (code != 1) --j;
        if (i / DTW_MR < lo) break;
      }
      if (k < 0) i = -1;
      sWalk[1] = i, sWalk[2] = j, sWalk[3] = k;
    }
    __syncthreads();
    i = sWalk[1], j = sWalk[2], k = sWalk[3];
    __syncthreads();
  }
}

int dtw_err(const char* msg) { return tt2_invalid("tt2_dtw", msg); }

template <int CPL>
void dtw_launch(const tt2_dtw_args& a, int nf, hipStream_t s) {
  const int waves = a.tb > 0 ? (a.tb + 64 * CPL - 1) / (64 * CPL) : 1;
  if (nf <= 16) hipLaunchKernelGGL((dtw_kernel<CPL, 16>), dim3(a.batch), dim3(64 * waves), 0, s, a);
  else hipLaunchKernelGGL((dtw_kernel<CPL, 32>), dim3(a.batch), dim3(64 * waves), 0, s, a);
}
}  // namespace

extern "C" size_t tt2_dtw_workspace_size(int batch, int ta, int tb, int want_path) {
  if (!want_path || batch <= 0 || ta <= 0 || tb <= 0) return 0;
  return (size_t)batch * ((ta + DTW_MR - 1) / DTW_MR) * tb * sizeof(uint32_t);
}

extern "C" int tt2_dtw(const tt2_dtw_args* p, hipStream_t s) {
  if (!p) return dtw_err("args required");
  if (p->batch < 0 || p->ta < 0 || p->tb < 0) return dtw_err("negative batch / ta / tb");
  if (p->ta > TT2_DTW_MAX_FRAMES || p->tb > TT2_DTW_MAX_FRAMES) return dtw_err("ta / tb exceed TT2_DTW_MAX_FRAMES");
  const int nf = p->c1 - p->c0;
  if (p->c0 < 0 || nf < 1 || nf > TT2_DTW_MAX_FEATS) return dtw_err("features [c0, c1): c0 >= 0, 1..32 of them");
  if (p->a_ld < p->c1 || p->b_ld < p->c1) return dtw_err("a_ld / b_ld below c1");
  if ((p->path_a == nullptr) != (p->path_b == nullptr)) return dtw_err("give both path arrays or neither");
  if (p->batch == 0) return TT2_OK;   // nothing to write: the arrays of an empty batch may be null
  if (!p->total || !p->length) return dtw_err("total / length required");
  const bool want = p->path_a != nullptr;
  const int rc = tt2_need_workspace("tt2_dtw", p->workspace, p->workspace_bytes,
                                    tt2_dtw_workspace_size(p->batch, p->ta, p->tb, want), 4);
  if (rc != TT2_OK) return rc;
  if (p->ta > 0 && p->tb > 0 && (!p->a || !p->b)) return dtw_err("a / b required");
  if (dtw_cpl(p->tb) == 1) dtw_launch<1>(*p, nf, s);
  else dtw_launch<2>(*p, nf, s);
  return tt2_check_launch(hipGetLastError(), "tt2_dtw");
}
