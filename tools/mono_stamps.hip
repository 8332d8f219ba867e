// In-kernel timeline of the monotonic alignment search (dev tool): builds attention_mono.hip with its
// MONO_STAMP hooks defined (s_memtime per wave; a tick is a shader cycle), runs the benchmark
// shape (B = 16, H = 8, 800 frames x 128 phonemes, bf16, MFMA producer, every utterance full
// length) and prints the DP wave's cycles per DP row (score production overlapped with it) and
// per backtrack step, and the rest of the launch.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form=1 -I include \
//     -I transformer-tacotron2_amd/csrc tools/mono_stamps.hip -o tools/bin/mono_stamps
//   tools/bin/mono_stamps [frames] [phonemes]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

// [utterance < 64][wave < 5][slot < 4]
constexpr size_t ST_N = (size_t)64 * 5 * 4;
__device__ unsigned long long g_st[ST_N];
#define MONO_STAMP(slot)                                                     \
  if ((threadIdx.x & 63) == 0 && blockIdx.x < 64 && (threadIdx.x >> 6) < 5) \
    g_st[((size_t)blockIdx.x * 5 + (threadIdx.x >> 6)) * 4 + (slot)] = __builtin_amdgcn_s_memtime();
#include "../transformer-tacotron2_amd/csrc/attention_mono.hip"
#include "../transformer-tacotron2_amd/csrc/runtime.cpp"

int main(int argc, char** argv) {
  const int B = 16, H = 8, Ty = argc > 1 ? atoi(argv[1]) : 800, Tx = argc > 2 ? atoi(argv[2]) : 128;
  const int d = 512;
  if (Tx > TT2_MONO_MAX_KEYS || Ty > TT2_MONO_MAX_FRAMES || Tx < 1 || Ty < 1) { fprintf(stderr, "shape\n"); return 2; }
  void *q, *k, *ws = nullptr;
  float *lse, *logp;
  int *path, *dur;
  hipMalloc(&q, (size_t)B * Ty * d * 2);
  hipMalloc(&k, (size_t)B * Tx * d * 2);
  hipMalloc(&lse, (size_t)B * H * Ty * 4);
  hipMalloc(&logp, B * 4);
  hipMalloc(&path, (size_t)B * Ty * 4);
  hipMalloc(&dur, (size_t)B * Tx * 4);
  hipMemset(lse, 0, (size_t)B * H * Ty * 4);
  const size_t wsz = tt2_align_monotonic_workspace_size(B, Ty, Tx);
  if (wsz) hipMalloc(&ws, wsz);
  unsigned x = 1;
  for (void* p : {q, k}) {
    std::vector<unsigned short> h((size_t)B * (p == q ? Ty : Tx) * d);
    for (auto& v : h) { x = x * 1664525u + 1013904223u; v = (x & 0x8000 ? 0xbf00 : 0x3f00) + ((x >> 16) & 0xff); }   // bf16 +-[0.5, 1)
    hipMemcpy(p, h.data(), h.size() * 2, hipMemcpyHostToDevice);
  }
  tt2_align_mono_args a{};
  a.q[0] = q; a.k[0] = k; a.lse[0] = lse;
  a.q_ld = a.k_ld = d;
  a.path = path; a.durations = dur; a.logp = logp; a.workspace = ws; a.workspace_bytes = wsz;
  a.n_layers = 1; a.batch = B; a.heads = H; a.head_dim = 64; a.tq = Ty; a.tk = Tx; a.dtype = TT2_DT_BF16;
  a.sel_layer = 0; a.sel_head = 3; a.scale = 0.125f;
  for (int i = 0; i < 5; ++i)
    if (tt2_align_monotonic(&a, 0) != TT2_OK) { fprintf(stderr, "mono: %s\n", tt2_last_error()); return 1; }
  if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "kernel failed\n"); return 1; }
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  hipEventRecord(e0, 0);
  for (int i = 0; i < 20; ++i) tt2_align_monotonic(&a, 0);
  hipEventRecord(e1, 0);
  hipEventSynchronize(e1);
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  std::vector<unsigned long long> st(ST_N);
  hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(g_st), st.size() * 8);
  std::vector<double> dp, bt, tail, all;
  for (int b = 0; b < B; ++b) {
    const unsigned long long* dw = &st[((size_t)b * 5 + 4) * 4];   // the DP wave
    const unsigned long long* w0 = &st[((size_t)b * 5 + 0) * 4];
    dp.push_back((double)(dw[1] - dw[0]));
    bt.push_back((double)(dw[2] - dw[1]));
    tail.push_back((double)(w0[3] - dw[2]));
    all.push_back((double)(w0[3] - w0[0]));
  }
  auto med = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
  printf("Ty %d Tx %d: %.1f us per launch (with stamps)\n", Ty, Tx, ms * 1e3 / 20);
  printf("median over %d utterances, shader cycles: DP phase %.0f = %.1f per row | backtrack %.0f = %.1f per step | "
         "durations + logp %.0f | stamp 0 to 3 %.0f\n",
         B, med(dp), med(dp) / Ty, med(bt), med(bt) / Ty, med(tail), med(all));
  return 0;
}
