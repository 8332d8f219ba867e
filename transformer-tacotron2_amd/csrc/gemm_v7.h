// gemm_v7.h -- what v10 and v11 (gemm_v10.hip, gemm_v11_impl.h) borrow from v7 (gemm_v7_impl.h): the
// stage geometry, the loader lanes' state and LDS-DMA issue, the fragment read of the 256-row
// images, the epilogue image's row map with the staged residual / gate copies, and the stamp
// hooks and knobs the three kernels share.
#pragma once
#include "gemm_common.h"

namespace {

// Fragment reads of the 256-row LDS images: K-contiguous [rows][8 chunks] with chunk c of
// row r at c ^ (r & 7); M/N-contiguous as 128-column sub-images [64 k][16 chunks] with
// chunk c of row k at c ^ mc_swz(k) (v2's images, stacked).
template <bool KC>
TT2_DEV void g7_frag(Frag8<bf16>& f, const char* img, int r0, int kk, int lane) {
  if (KC) frag2<true>(f, img, r0, kk, lane);
  else frag2<false>(f, img + (r0 >> 7) * 16384, r0 & 127, kk, lane);
}

// Measurement hook: tools/gemm_stamps.hip defines these (and the buffer they write)
// before including this file; the library build compiles them away.  The in-step phase
// build (-DTT2_PHASE=1, tools/g7_phases.py) writes them into the launch probe's per-work-group
// record (TT2_SPAN_W slots, layout at span_begin): s_memtime of MFMA wave 0 at the start of
// K steps 0..11 and after their MFMAs, and at the epilogue's four points.
#if defined(TT2_PHASE) && !defined(G7_STAMP)
#define G7_STAMP(t, slot)                                                                  \
  if (srec && threadIdx.x == 0) {                                                          \
    const int si_ = (t) == nkt ? 27 + (slot) : (t) < 12 ? 3 + 2 * (t) + (slot) : -1;        \
    if (si_ >= 0) srec[si_] = __builtin_amdgcn_s_memtime();                                \
  }
#endif
#ifndef G7_STAMP
#define G7_STAMP(t, slot)
#endif
#ifndef G7_RT
#define G7_RT(slot)
#endif

#ifndef G7_BUF   // plain operands' LDS-DMA copies as buffer_load ... lds (1) or global_load_lds (0)
#define G7_BUF 1
#endif
#ifndef G7_PRIO   // MFMA waves 4-7 (the younger of each SIMD's two) at s_setprio 1 for the K loop:
#define G7_PRIO 0   // bit-identical, within +-2 % per GEMM, the step the same (profiles/r06_g7_prio_ab.txt)
#endif
constexpr int G7_NT = 768;                          // 8 MFMA waves + 4 loader waves
constexpr int G7_A = 256 * 128, G7_B = 128 * 128;   // bytes per stage: 64 k x 2 B per row
constexpr int G7_STAGE = G7_A + G7_B;               // 48 KB
constexpr int G7_STAGES = 3;
constexpr int G7_AI = G7_A / 1024 / 4, G7_BI = G7_B / 1024 / 4;   // copies per loader wave: 8 + 4
constexpr int G7_SMEM = G7_STAGES * G7_STAGE;

// Loader-lane state of one operand (NI copies per step).  Plain operands: a loop-
// invariant byte offset from a wave-uniform base.  Conv operands (implicit im2col,
// ld = C, element (outer, inner) at (outer + tap - pad) * C + ci) also track the
// copy's conv coordinates incrementally (64 k per step, C >= 64 and T >= 64 so one
// conditional wrap suffices): K-contiguous A (k = tap * C + ci): tap and ci of the
// chunk, t of the row; M/N-contiguous B (k = token row): t of the k row, tap of the
// column.  A copy reads the zero page when its chunk is conv padding or k >= ke.
template <int NI> struct G7Lane {
  uint32_t off[NI];
  int t[NI], tap[NI], ci[NI];
  uint32_t vm[NI];   // K-contiguous conv operand with C % 64 == 0: bit tap = row t + tap - pad is inside [0, T)
};

// A K-contiguous conv operand whose channel count is a multiple of 64 keeps every 64-deep K
// step inside one tap, so a copy's validity is one bit of a per-row tap mask (no per-step
// coordinate tracking on the loader waves, whose VALU work slows the MFMA waves' K loop).
TT2_DEV bool g7_conv_fast(const OpDesc& d) { return d.conv_t > 0 && (d.conv_c & 63) == 0; }

template <bool KC, int NI>
TT2_DEV void g7_lane_init(G7Lane<NI>& L, const OpDesc& d, int r0, int kb, int lane, int lw) {
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int inst = lw * NI + i;
    if (KC) {
      const int row = inst * 8 + (lane >> 3);
      const int gc = (lane & 7) ^ (row & 7);
      const int r = min(r0 + row, d.outer_max - 1);
      L.off[i] = (uint32_t)(((int64_t)r * d.ld + gc * 8) * 2);
      if (d.conv_t > 0) {
        const int k = kb + gc * 8;
        L.t[i] = r % d.conv_t;
        L.tap[i] = k / d.conv_c;
        L.ci[i] = k - L.tap[i] * d.conv_c;
        const int lo = max(0, d.conv_pad - L.t[i]), hi = min(31, d.conv_t - 1 - L.t[i] + d.conv_pad);
        L.vm[i] = hi >= lo ? (0xFFFFFFFFu >> (31 - hi)) & (0xFFFFFFFFu << lo) : 0u;   // taps lo..hi
      }
    } else {
      const int sub = inst >> 4, kr = (inst & 15) * 4 + (lane >> 4);
      const int gc = (lane & 15) ^ mc_swz(kr);
      int col = r0 + sub * 128 + gc * 8;
      col = col < d.inner_max ? col : d.inner_max - 8;
      L.off[i] = (uint32_t)(((int64_t)kr * d.ld + col) * 2);
      if (d.conv_t > 0) {
        L.t[i] = (kb + kr) % d.conv_t;
        L.tap[i] = col / d.conv_c;
        L.ci[i] = 0;
      }
    }
  }
}

template <bool KC, int NI>
TT2_DEV void g7_issue(const OpDesc& d, G7Lane<NI>& L, char* lds, int k0, int ke, int lane, int lw, bool tl,
                      bool cfast) {
  const bool conv = d.conv_t > 0;
  const int64_t shift = conv ? (int64_t)d.conv_pad * d.conv_c : 0;
  const char* base = reinterpret_cast<const char*>(d.p) + ((KC ? (int64_t)k0 : (int64_t)k0 * d.ld) - shift) * 2;
  if (!conv && !tl) {
#if G7_BUF && defined(__HIP_DEVICE_COMPILE__)   // (the host pass has no buffer_load_lds builtin)
    // buffer_load ... lds: the step's byte offset in an SGPR, the lane's loop-invariant offset in
    // one VGPR (no 64-bit lane address per copy); operands < 2 GB (the plan's v7 condition)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(d.p), (short)0, 0x7fffffff,
                                                                        0x00020000);
    const unsigned soff = (unsigned)((KC ? (int64_t)k0 : (int64_t)k0 * d.ld) * 2);
#pragma unroll
    for (int i = 0; i < NI; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lvoid_t*)(lds + (lw * NI + i) * 1024), 16, L.off[i], soff, 0, 0);
#else
#pragma unroll
    for (int i = 0; i < NI; ++i)
      __builtin_amdgcn_global_load_lds((gvoid_t*)(base + L.off[i]), (lvoid_t*)(lds + (lw * NI + i) * 1024), 16, 0,
                                       0);
#endif
    return;
  }
  if (KC && cfast) {   // the whole step reads tap k0 / C
    const int tap = k0 / d.conv_c;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const void* src = (L.vm[i] >> tap) & 1u ? (const void*)(base + L.off[i]) : (const void*)g_zero_page;
      __builtin_amdgcn_global_load_lds((gvoid_t*)src, (lvoid_t*)(lds + (lw * NI + i) * 1024), 16, 0, 0);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int inst = lw * NI + i;
    int k;
    if (KC) {
      const int row = inst * 8 + (lane >> 3);
      k = k0 + ((lane & 7) ^ (row & 7)) * 8;
    } else {
      k = k0 + (inst & 15) * 4 + (lane >> 4);
    }
    bool ok = k < ke;
    if (conv) {
      ok = ok && (unsigned)(L.t[i] + L.tap[i] - d.conv_pad) < (unsigned)d.conv_t;
      if (KC) {   // next step: k += 64 within (tap, ci)
        L.ci[i] += 64;
        if (L.ci[i] >= d.conv_c) { L.ci[i] -= d.conv_c; ++L.tap[i]; }
      } else {    // next step: token row += 64
        L.t[i] += 64;
        if (L.t[i] >= d.conv_t) L.t[i] -= d.conv_t;
      }
    }
    const void* src = ok ? (const void*)(base + L.off[i]) : (const void*)g_zero_page;
    __builtin_amdgcn_global_load_lds((gvoid_t*)src, (lvoid_t*)(lds + inst * 1024), 16, 0, 0);
  }
}

// One GEMM problem of a (possibly grouped) v7 launch.  Work item = (split, tile).
struct G7Prob {
  OpDesc A, B;
  EpiParams E;
  int M, N, K, k_split, splits, ntn, items, item0;
  float* ws;   // split-K slabs [splits][M][N] (+ [splits][M] k-sums); used when splits > 1
  int lds_epi; // C leaves through an LDS image in whole 256-B row segments (bf16 C, no split)
  int pre_x;     // the loader waves stage the bf16 residual (1) or gate (2) tile in LDS (lds_epi only)
  int epi_fast;  // straight-line image epilogue for this option set (g7_epi_fast), -1: general path
  unsigned long long* span;   // launch probe's span record (grouped launch: p[0]'s), else null
};

// The epilogue's 256-row image (C, and before it the staged residual / gate in place):
// rows 0..191 fill the ring stage of K step nkt - 3 (the first stage that no later step
// reuses), rows 192..255 the stage of step nkt - 2, so the staged tile can land while the
// last K steps still read the third stage.  Chunk c of row r sits at slot c ^ (r & 15).
TT2_DEV int g7_img_row(int nkt, int r) {
  return r < 192 ? (nkt % 3) * G7_STAGE + r * 256 : ((nkt + 1) % 3) * G7_STAGE + (r - 192) * 256;
}

// Loader waves: stage rows [r0, r0 + 4 * ni * 4) of the residual / gate tile (bf16, 16-B
// aligned rows) into the image, ni copies per wave (rows past M repeat row M - 1).  The copies
// are nontemporal (G7_X_AUX 2 = nt): each line is read once, and as default-policy lines they
// pushed the B operand, which every row tile of the launch re-reads, out of the XCD's L2.
#ifndef G7_X_AUX
#define G7_X_AUX 2
#endif
TT2_DEV void g7_issue_x(const G7Prob& P, const void* x, int64_t ldx, char* smem, int nkt, int m0, int n0, int r0,
                        int ni, int lane, int lw) {
  const char* base = reinterpret_cast<const char*>(x);
  for (int i = 0; i < ni; ++i) {
    const int inst = lw * ni + i, r = r0 + inst * 4 + (lane >> 4);
    const int m = min(m0 + r, P.M - 1), c = (lane & 15) ^ (r & 15);
    __builtin_amdgcn_global_load_lds((gvoid_t*)(base + ((int64_t)m * ldx + n0 + 8 * c) * 2),
                                     (lvoid_t*)(smem + g7_img_row(nkt, r0 + inst * 4)), 16, 0, G7_X_AUX);
  }
}

}  // namespace
