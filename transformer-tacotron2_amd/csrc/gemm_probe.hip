// gemm_probe.hip -- the GEMM launch probe's state and its tt2_probe_* entry points (measurement).
// The GEMM units reach the state through tt2g::probe_take / probe_chunk / probe_disarm
// (gemm_common.h: ProbeScope around a launch, ProbeDisarm around a tt2_gemm call).
#include <vector>

#include "gemm_common.h"

namespace {

// Launch probe (measurement): when armed, the next main GEMM kernel launched on this
// thread records a start / stop event pair at its own dispatch and completion
// (hipExtLaunchKernelGGL), i.e. the kernel's execution time as rocprofv3 reports it,
// without the gaps an event recorded around the launch on the stream adds.
struct ProbeSlot { hipEvent_t start, stop; bool used; };
thread_local std::vector<ProbeSlot> g_probe;
thread_local int g_probe_armed = -1;
// Beside the events, every probe-capable kernel records its own span on the device's
// constant-rate wall clock: each workgroup writes {its start, the end of its last wave after
// that wave's stores completed} to its own pair of a slot's record (plain stores, no shared
// address), and tt2_probe_span_ms takes the earliest start and the latest end.  Nothing is
// added to the stream, so the span of a launch inside a replayed step graph is its in-step
// duration, with no event node (and its dispatch gap) around it.  Records come from one
// pool per thread, allocated (zeroed) by the first tt2_probe_arm, outside any capture.
// (record width: TT2_SPAN_W, gemm_common.h)
#ifdef TT2_PHASE
constexpr int64_t PROBE_SPAN_PAIRS = 1 << 17;
#else
constexpr int64_t PROBE_SPAN_PAIRS = 1 << 20;
#endif
thread_local unsigned long long* g_span = nullptr;
thread_local int64_t g_span_used = 0;
thread_local std::vector<std::pair<int64_t, int>> g_span_rec;   // per slot: pool offset, work groups
// per slot: work groups per launch when one probed call goes out as consecutive launches (a
// capped grouped grid): the span is then the sum of the launches' own spans, as rocprofv3
// times each dispatch (0: one launch)
thread_local std::vector<int> g_span_chunk;

}  // namespace

namespace tt2g {

int probe_take(hipEvent_t& e0, hipEvent_t& e1, unsigned long long*& span, int groups) {
  span = nullptr;
  if (g_probe_armed < 0) return -1;
  const int slot = g_probe_armed;
  ProbeSlot& p = g_probe[slot];
  e0 = p.start;
  e1 = p.stop;
  p.used = true;
  if (g_span && groups > 0 && g_span_used + groups <= PROBE_SPAN_PAIRS) {
    span = g_span + TT2_SPAN_W * g_span_used;
    g_span_rec[slot] = {g_span_used, groups};
    g_span_used += groups;
  }
  g_probe_armed = -1;
  return slot;
}

void probe_chunk(int slot, int wgs) { g_span_chunk[slot] = wgs; }

void probe_disarm() { g_probe_armed = -1; }

}  // namespace tt2g

extern "C" int tt2_probe_arm(void) {
  // timing-only events: no system-scope fence (cache write-back) at the probed kernel's end,
  // which would lengthen it beyond what it takes inside the step
  ProbeSlot p{nullptr, nullptr, false};
  hipError_t e = hipSuccess;
  if (!g_span) {
    e = hipMalloc(&g_span, TT2_SPAN_W * sizeof(unsigned long long) * PROBE_SPAN_PAIRS);
    if (e == hipSuccess) e = hipMemset(g_span, 0, TT2_SPAN_W * sizeof(unsigned long long) * PROBE_SPAN_PAIRS);
    if (e != hipSuccess) {
      if (g_span) (void)hipFree(g_span);
      g_span = nullptr;
      return tt2_check_launch(e, "tt2_probe_arm (span records)");
    }
  }
  e = hipEventCreateWithFlags(&p.start, hipEventDisableSystemFence);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&p.stop, hipEventDisableSystemFence);
  if (e != hipSuccess) return tt2_check_launch(e, "tt2_probe_arm");
  g_probe.push_back(p);
  g_span_rec.push_back({-1, 0});
  g_span_chunk.push_back(0);
  g_probe_armed = (int)g_probe.size() - 1;
  return g_probe_armed;
}

extern "C" float tt2_probe_ms(int slot) {
  if (slot < 0 || slot >= (int)g_probe.size() || !g_probe[slot].used) return -1.f;
  float ms = -1.f;
  if (hipEventSynchronize(g_probe[slot].stop) != hipSuccess) return -1.f;
  if (hipEventElapsedTime(&ms, g_probe[slot].start, g_probe[slot].stop) != hipSuccess) return -1.f;
  return ms;
}

extern "C" float tt2_probe_span_ms(int slot) {
  if (slot < 0 || slot >= (int)g_probe.size() || !g_probe[slot].used || g_span_rec[slot].first < 0) return -1.f;
  const int64_t off = g_span_rec[slot].first;
  const int groups = g_span_rec[slot].second;
  std::vector<unsigned long long> h(TT2_SPAN_W * (size_t)groups);
  if (hipDeviceSynchronize() != hipSuccess) return -1.f;
  if (hipMemcpy(h.data(), g_span + TT2_SPAN_W * off, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
  // zeroed again, so the next replay of a graph must record every pair afresh
  if (hipMemset(g_span + TT2_SPAN_W * off, 0, h.size() * 8) != hipSuccess) return -1.f;
  const int chunk = g_span_chunk[slot] > 0 ? g_span_chunk[slot] : groups;
  unsigned long long total = 0;
  for (int c0 = 0; c0 < groups; c0 += chunk) {   // each launch's own span
    unsigned long long t0 = ~0ull, t1 = 0;
    for (int i = c0; i < std::min(groups, c0 + chunk); ++i) {
      const unsigned long long s0 = h[TT2_SPAN_W * i], s1 = h[TT2_SPAN_W * i + 1];
      if (s0 == 0 || s1 < s0) return -1.f;   // a work group left no record
      t0 = std::min(t0, s0);
      t1 = std::max(t1, s1);
    }
    total += t1 - t0;
  }
  static int khz = 0;
  if (!khz) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) {
      khz = 0;
      return -1.f;
    }
  }
  return (float)((double)total / khz);
}

extern "C" int tt2_probe_span_records(int slot, unsigned long long* out, int cap) {
  if (slot < 0 || slot >= (int)g_probe.size() || !g_probe[slot].used || g_span_rec[slot].first < 0 || !out)
    return -1;
  const int64_t off = g_span_rec[slot].first;
  const int groups = g_span_rec[slot].second;
  if (cap < groups) return -groups - 1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(out, g_span + TT2_SPAN_W * off, (size_t)groups * TT2_SPAN_W * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return groups;
}

// u64 slots per work group in tt2_probe_span_records' output: 2 ({start, end} on the wall
// clock), 32 in the in-step phase build (TT2_PHASE, see TT2_SPAN_W)
extern "C" int tt2_probe_span_width(void) { return TT2_SPAN_W; }

extern "C" void tt2_probe_reset(void) {
  // records of slots never read are zeroed so the pool can be handed out again
  if (g_span && g_span_used) (void)hipMemset(g_span, 0, TT2_SPAN_W * sizeof(unsigned long long) * g_span_used);
  g_span_used = 0;
  g_span_rec.clear();
  g_span_chunk.clear();
  for (ProbeSlot& p : g_probe) {
    (void)hipEventDestroy(p.start);
    (void)hipEventDestroy(p.stop);
  }
  g_probe.clear();
  g_probe_armed = -1;
}
