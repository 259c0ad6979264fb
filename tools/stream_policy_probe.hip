// Measurement tool (not part of the library): does a cache-policy hint (`nt`) on a once-used STREAM keep that stream from
// displacing a table that is resident in the 256 MiB Infinity Cache?
//
// In the headline step the fp32 residual x (B = 8: 32768 rows x 1152 fp32 = 151 MB) is read four times per block, and between
// two uses the once-used streams of the block go past it: fc1 writes 302 MB of f16 hidden activations, fc2 reads them back; the
// attention kernel writes 75 MB, the out-projection reads them.  All of them use the default policy.  The probe asks whether
// `nt` on the stream (stores, loads, or the LDS DMA the GEMMs load operands with: aux = 2) leaves x in the cache.
//
// One measurement:   read T (untimed: makes T the most recently used bytes)  ->  stream S  ->  re-read T, timed by events.
//   T      fp32 table, 151 MB (x) or 226 MB (x + xn), read with float4 loads, 1 KB of a row per wave instruction
//   S      302 MB of halves: written with u32x4 stores {plain, nt}, then read back with u32x4 loads {plain, nt} or moved into
//          LDS by buffer_load ... lds with aux 0 / 2 (the GEMMs' form); store-only and load-only arms separate the two halves
//   controls: nothing between the two reads of T (resident), and a plain read of a separate 604 MB buffer between (flushed)
// "stream us" is the median time of the stream's own kernels (a hint that only moved the cost into the stream would show there).
// Every arm is run once per round, the arms alternate inside a round, round 0 is a warm-up; min / median / max of the rest.
// Decision rule: a hint governs retention if T's re-read after the hinted stream is faster than after the same stream with
// the default policy by more than the spread (max - min) of the default-policy arm.
//   hipcc -O3 --offload-arch=gfx950 tools/stream_policy_probe.hip -o /tmp/stream_policy_probe && /tmp/stream_policy_probe [repeats]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;

constexpr int NWG = 2048, NT = 256;
constexpr size_t T_SMALL = (size_t)32768 * 1152 * 4;       // x
constexpr size_t T_LARGE = T_SMALL + T_SMALL / 2;          // x + xn
constexpr size_t S_BYTES = (size_t)32768 * 4608 * 2;       // fc1's hidden activations
constexpr size_t F_BYTES = 2 * S_BYTES;                    // the flushing control
static_assert(T_LARGE % (16 * NT) == 0 && S_BYTES % (16 * NT) == 0 && F_BYTES % (16 * NT) == 0, "whole 4 KB workgroup pieces: the kernels have no tail");
static_assert(S_BYTES < (1ull << 32), "the DMA arm addresses S through one 32-bit buffer resource");

enum { PLAIN = 0, NTEMP = 1, DMA0 = 2, DMA2 = 3, NONE = 4 };

// T, and the flushing control: float4 loads, consecutive lanes on consecutive 16 B.  `sink` is never written (the sum of a
// zero-filled buffer is 0), it only keeps the loads alive.
__global__ void __launch_bounds__(NT) read_kernel(const float4* __restrict__ t, size_t n4, float* __restrict__ sink) {
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (size_t)gridDim.x * NT) {
    const float4 v = t[i];
    s += v.x + v.y + v.z + v.w;
  }
  if (s == 12345.f) sink[0] = s;
}

template <int MODE>
__global__ void __launch_bounds__(NT) store_kernel(u32x4* __restrict__ s, size_t n4) {
  const u32x4 v = {0u, 0u, 0u, 0u};
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (size_t)gridDim.x * NT) {
    if constexpr (MODE == NTEMP) __builtin_nontemporal_store(v, s + i);
    else s[i] = v;
  }
}

template <int MODE>
__global__ void __launch_bounds__(NT) load_kernel(const u32x4* __restrict__ s, size_t n4, unsigned* __restrict__ sink) {
  unsigned acc = 0u;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (size_t)gridDim.x * NT) {
    u32x4 v;
    if constexpr (MODE == NTEMP) v = __builtin_nontemporal_load(s + i);
    else v = s[i];
    acc += v.x + v.y + v.z + v.w;
  }
  if (acc == 12345u) sink[0] = acc;
}

// The GEMMs' operand load: every wave instruction moves 1 KB (64 lanes x 16 B) from the buffer into the wave's own LDS slot,
// four slots per wave in rotation.  n4 is a multiple of NT, so every piece is whole and inside the resource; the resource's
// range check would drop anything beyond it in any case.
template <int AUX>
__global__ void __launch_bounds__(NT) dma_kernel(const u32x4* __restrict__ s, size_t n4) {
  __shared__ __attribute__((aligned(1024))) char lds[(NT / 64) * 4 * 1024];
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)s, 0, (unsigned)(n4 * 16), 0x00020000);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  char* const slot = lds + wave * 4 * 1024;
  int k = 0;
  for (size_t p = (size_t)blockIdx.x * NT; p < n4; p += (size_t)gridDim.x * NT, ++k) {
    const unsigned piece = (unsigned)((p + wave * 64) * 16);   // wave-uniform byte offset of this wave's 1 KB
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(slot + (k & 3) * 1024), 16, (unsigned)lane * 16u, piece, 0, AUX);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

struct Arm { const char* name; int st, ld; };   // ld == -1: resident control, ld == -2: flushed control

int main(int argc, char** argv) {
  const int reps = argc > 1 ? std::max(1, atoi(argv[1])) : 15;
  char *T, *S, *F;
  float* sink;
  CK(hipMalloc(&T, T_LARGE));
  CK(hipMalloc(&S, S_BYTES));
  CK(hipMalloc(&F, F_BYTES));
  CK(hipMalloc(&sink, 16));
  CK(hipMemset(T, 0, T_LARGE));
  CK(hipMemset(S, 0, S_BYTES));
  CK(hipMemset(F, 0, F_BYTES));
  hipStream_t st;
  CK(hipStreamCreate(&st));
  hipEvent_t eb, e0, e1;
  CK(hipEventCreate(&eb));
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const Arm arms[] = {
      {"control: nothing between (resident)", NONE, -1},
      {"control: plain read of 604 MB between (flushed)", NONE, -2},
      {"store plain, load plain", PLAIN, PLAIN},
      {"store plain, load nt", PLAIN, NTEMP},
      {"store nt,    load plain", NTEMP, PLAIN},
      {"store nt,    load nt", NTEMP, NTEMP},
      {"store plain, LDS DMA aux 0", PLAIN, DMA0},
      {"store plain, LDS DMA aux 2 (nt)", PLAIN, DMA2},
      {"store nt,    LDS DMA aux 0", NTEMP, DMA0},
      {"store nt,    LDS DMA aux 2 (nt)", NTEMP, DMA2},
      {"store plain only", PLAIN, NONE},
      {"store nt only", NTEMP, NONE},
      {"load plain only", NONE, PLAIN},
      {"load nt only", NONE, NTEMP},
      {"LDS DMA aux 0 only", NONE, DMA0},
      {"LDS DMA aux 2 (nt) only", NONE, DMA2}};
  constexpr int NA = sizeof(arms) / sizeof(arms[0]);
  const size_t s4 = S_BYTES / 16;
  printf("stream_policy_probe: stream S = %.0f MB of halves, %d timed runs per arm, time = re-read of T after the stream\n", S_BYTES / 1e6, reps);
  for (const size_t tbytes : {T_SMALL, T_LARGE}) {
    const size_t t4 = tbytes / 16;
    std::vector<float> us[NA], us_stream[NA];
    for (int r = 0; r < reps + 1; ++r) {   // round 0 = warm-up, not recorded
      for (int a = 0; a < NA; ++a) {
        hipLaunchKernelGGL(read_kernel, dim3(NWG), dim3(NT), 0, st, (const float4*)T, t4, sink);
        CK(hipEventRecord(eb, st));
        if (arms[a].ld == -2) hipLaunchKernelGGL(read_kernel, dim3(NWG), dim3(NT), 0, st, (const float4*)F, F_BYTES / 16, sink);
        if (arms[a].st == PLAIN) hipLaunchKernelGGL(store_kernel<PLAIN>, dim3(NWG), dim3(NT), 0, st, (u32x4*)S, s4);
        if (arms[a].st == NTEMP) hipLaunchKernelGGL(store_kernel<NTEMP>, dim3(NWG), dim3(NT), 0, st, (u32x4*)S, s4);
        if (arms[a].ld == PLAIN) hipLaunchKernelGGL(load_kernel<PLAIN>, dim3(NWG), dim3(NT), 0, st, (const u32x4*)S, s4, (unsigned*)sink);
        if (arms[a].ld == NTEMP) hipLaunchKernelGGL(load_kernel<NTEMP>, dim3(NWG), dim3(NT), 0, st, (const u32x4*)S, s4, (unsigned*)sink);
        if (arms[a].ld == DMA0) hipLaunchKernelGGL(dma_kernel<0>, dim3(NWG), dim3(NT), 0, st, (const u32x4*)S, s4);
        if (arms[a].ld == DMA2) hipLaunchKernelGGL(dma_kernel<2>, dim3(NWG), dim3(NT), 0, st, (const u32x4*)S, s4);
        CK(hipEventRecord(e0, st));
        hipLaunchKernelGGL(read_kernel, dim3(NWG), dim3(NT), 0, st, (const float4*)T, t4, sink);
        CK(hipEventRecord(e1, st));
        CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r) us[a].push_back(ms * 1e3f);
        CK(hipEventElapsedTime(&ms, eb, e0));
        if (r) us_stream[a].push_back(ms * 1e3f);
      }
    }
    printf("\nT = %.0f MB fp32\n", tbytes / 1e6);
    printf("%-50s %9s %9s %9s %8s %10s\n", "between the two reads of T", "min us", "median us", "max us", "TB/s med", "stream us");
    float med[NA], lo[NA], hi[NA];
    for (int a = 0; a < NA; ++a) {
      std::sort(us[a].begin(), us[a].end());
      lo[a] = us[a].front(), hi[a] = us[a].back(), med[a] = us[a][us[a].size() / 2];
      std::sort(us_stream[a].begin(), us_stream[a].end());
      printf("%-50s %9.1f %9.1f %9.1f %8.2f %10.1f\n", arms[a].name, lo[a], med[a], hi[a], tbytes / (med[a] * 1e-6) / 1e12, us_stream[a][us_stream[a].size() / 2]);
    }
    // each hinted arm against the arm that streams the same bytes with the default policy
    const int pairs[][2] = {{3, 2}, {4, 2}, {5, 2}, {7, 6}, {8, 6}, {9, 6}, {11, 10}, {13, 12}, {15, 14}};
    bool any = false;
    for (const auto& p : pairs) {
      const float gain = med[p[1]] - med[p[0]], spread = hi[p[1]] - lo[p[1]];
      const bool yes = gain > spread;
      any |= yes;
      printf("  %-34s vs default: %+7.1f us, default arm's spread %6.1f us -> %s\n", arms[p[0]].name, -gain, spread, yes ? "RETAINS" : "no");
    }
    printf("verdict at T = %.0f MB: %s\n", tbytes / 1e6, any ? "a hinted stream leaves more of T in the Infinity Cache" : "no hint governs retention");
  }
  return 0;
}
