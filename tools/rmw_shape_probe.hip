// Measurement tool (not part of the library): what the ACCESS SHAPE of the gated GEMMs' fp32 read-modify-write epilogue
// (gemm_pw.hip, EPI_GATE_RES_F32:  x[m][n] += gate[n] * (acc + bias)) costs on its own, without the GEMM in front of it.
//
// The residual stream of the headline shape (B = 8: 32768 rows x 1152 fp32 = 151 MB) is walked as the 12-wave kernel walks it:
// 256 workgroups of 8 (consumer) waves, 256 x 192 output tiles (768 of them, three per workgroup), wave (grp, wn) owns rows
// grp * 128 ... + 127 and columns wn * 48 ... + 47 of its tile.  Only the way a wave's 128 x 48 floats are requested differs:
//   a  the fragment-wise epilogue (GemmArgs::rmw_mode 0; "today" in the output: the only form when the probe was run): lane
//      (r, c) = (lane & 15, lane >> 4) -> row r, 16 B at column group c of a 16 x 16 accumulator fragment.  One instruction =
//      16 rows x 64 B: sixteen half 128-byte lines.
//   b  8 rows x 128 B per instruction.  A wave's 192-byte span holds one and a half lines, so whole lines need a PAIR of waves
//      (wn 0/1, 2/3) over a 96-column = 3-line span; here each wave of a pair takes 64 rows x 96 columns.  In the GEMM the
//      accumulators would have to cross between the two waves (LDS + a barrier of their own).
//   c  5 1/3 rows x 192 B per instruction: a wave's own 16 x 48 fragment row as 192 pieces of 16 B, lane p -> row p / 12,
//      piece p % 12 -- the nearest to "4 rows x 256 B" that the 192-byte wave span allows, and what a wave-private patch gives.
//   d  what a wave can do ALONE in registers (lane l <-> l ^ 8 exchange of two adjacent fragments): the 128-byte-aligned line
//      of its span as 8 rows x 128 B, the other 64 B as in (a) (half lines shared with the neighbouring wave): rmw_mode 1.
// Each shape runs with 2 (today's) and 4 residual loads in flight ahead of the stores.  24 load + 24 store instructions per
// wave and tile in every shape.  Before every timed launch a 512 MiB scratch buffer is streamed so that the residual comes
// from HBM, not from the Infinity Cache (in the model the 151 MB state is not cache resident between two gated GEMMs).
// gate[n] are multiples of 0.25 and the "accumulator" is 1.0, so after R launches every element must be exactly R * gate[n].
//   hipcc -O3 --offload-arch=gfx950 tools/rmw_shape_probe.hip -o /tmp/rmw_shape_probe && /tmp/rmw_shape_probe [repeats]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int M = 32768, N = 1152, BM = 256, BN = 192, WTN = 48;
constexpr int TILES_M = M / BM, TILES_N = N / BN, NWG = 256, NTILE = TILES_M * TILES_N;
static_assert(M % BM == 0 && N % BN == 0, "whole tiles only: the kernels below have no bounds checks");

// One access of the wave's sub-tile: instruction q (0..23) of the shape -> this lane's float4, and the column it starts at.
template <int SHAPE>
__device__ __forceinline__ void locate(int q, int lane, int grp, int wn, int& row, int& col) {
  if constexpr (SHAPE == 0) {          // 8 fragment rows x 3 fragments, 16 rows x 64 B
    row = grp * 128 + (q / 3) * 16 + (lane & 15);
    col = wn * WTN + (q % 3) * 16 + (lane >> 4) * 4;
  } else if constexpr (SHAPE == 1) {   // wave pair: 64 rows x 96 columns per wave, 8 rows x one 128-byte line
    row = grp * 128 + (wn & 1) * 64 + (q / 3) * 8 + (lane >> 3);
    col = (wn >> 1) * 96 + (q % 3) * 32 + (lane & 7) * 4;
  } else if constexpr (SHAPE == 2) {   // 16 x 48 fragment row = 192 pieces of 16 B over three instructions
    const int p = (q % 3) * 64 + lane;
    row = grp * 128 + (q / 3) * 16 + p / 12;
    col = wn * WTN + (p % 12) * 4;
  } else {                             // the aligned line of the span in two instructions of 8 rows, the half line as today
    const int line0 = (wn & 1) ? 16 : 0, half0 = (wn & 1) ? 0 : 32;   // odd spans start 64 B into a line
    const int k = q % 3;
    if (k < 2) {
      row = grp * 128 + (q / 3) * 16 + k * 8 + (lane >> 3);
      col = wn * WTN + line0 + (lane & 7) * 4;
    } else {
      row = grp * 128 + (q / 3) * 16 + (lane & 15);
      col = wn * WTN + half0 + (lane >> 4) * 4;
    }
  }
}

template <int SHAPE, int AHEAD>
__global__ void __launch_bounds__(512) rmw_kernel(float* __restrict__ x, const float* __restrict__ gate, float v) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = wave >> 2, wn = wave & 3;
  for (int t = blockIdx.x; t < NTILE; t += NWG) {
    const int tm = t / TILES_N, tn = t % TILES_N;
    float* const base = x + (size_t)tm * BM * N + tn * BN;
    constexpr int NQ = 24;
    float4 qa[AHEAD];
    auto ptr = [&](int q) -> float* {
      int row, col;
      locate<SHAPE>(q, lane, grp, wn, row, col);
      return base + (size_t)row * N + col;
    };
#pragma unroll
    for (int a = 0; a < AHEAD; ++a) qa[a] = *(const float4*)ptr(a);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float4 rr = qa[q % AHEAD];
      if (q + AHEAD < NQ) qa[q % AHEAD] = *(const float4*)ptr(q + AHEAD);
      asm volatile("" ::: "memory");
      int row, col;
      locate<SHAPE>(q, lane, grp, wn, row, col);
      const float4 g4 = *(const float4*)(gate + tn * BN + col);
      rr.x += g4.x * v; rr.y += g4.y * v; rr.z += g4.z * v; rr.w += g4.w * v;
      *(float4*)ptr(q) = rr;
    }
  }
}

// plain float4 stream over the same buffer, one wave instruction = 1 KB of one row (the LayerNorm pass's shape): the yardstick
__global__ void __launch_bounds__(256) stream_rmw_kernel(float4* __restrict__ x, const float4* __restrict__ gate, float v, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    float4 rr = x[i];
    const float4 g4 = gate[i % (N / 4)];
    rr.x += g4.x * v; rr.y += g4.y * v; rr.z += g4.z * v; rr.w += g4.w * v;
    x[i] = rr;
  }
}

__global__ void __launch_bounds__(256) flush_kernel(float4* __restrict__ s, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    float4 q = s[i];
    q.x += 1.0f;
    s[i] = q;
  }
}

struct Case { const char* name; void (*launch)(float*, const float*, hipStream_t); };
template <int SHAPE, int AHEAD>
static void launch_shape(float* x, const float* g, hipStream_t st) { hipLaunchKernelGGL((rmw_kernel<SHAPE, AHEAD>), dim3(NWG), dim3(512), 0, st, x, g, 1.0f); }
static void launch_stream(float* x, const float* g, hipStream_t st) {
  hipLaunchKernelGGL(stream_rmw_kernel, dim3(NWG * 8), dim3(256), 0, st, (float4*)x, (const float4*)g, 1.0f, (size_t)M * N / 4);
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? std::max(1, atoi(argv[1])) : 15;
  const size_t n = (size_t)M * N, scratch_n4 = (512ull << 20) / 16;
  float *x, *gate;
  float4* scratch;
  CK(hipMalloc(&x, n * 4));
  CK(hipMalloc(&gate, N * 4));
  CK(hipMalloc(&scratch, scratch_n4 * 16));
  CK(hipMemset(x, 0, n * 4));
  CK(hipMemset(scratch, 0, scratch_n4 * 16));
  std::vector<float> hg(N);
  for (int i = 0; i < N; ++i) hg[i] = 0.25f * (float)(i % 7 + 1);
  CK(hipMemcpy(gate, hg.data(), N * 4, hipMemcpyHostToDevice));
  hipStream_t st;
  CK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const Case cases[] = {
      {"a  16 rows x  64 B, 2 ahead (today)", launch_shape<0, 2>}, {"a  16 rows x  64 B, 4 ahead", launch_shape<0, 4>},
      {"b   8 rows x 128 B, 2 ahead (wave pair)", launch_shape<1, 2>}, {"b   8 rows x 128 B, 4 ahead (wave pair)", launch_shape<1, 4>},
      {"c 5.3 rows x 192 B, 2 ahead", launch_shape<2, 2>}, {"c 5.3 rows x 192 B, 4 ahead", launch_shape<2, 4>},
      {"d 8 x 128 B + 16 x 64 B, 2 ahead (one wave)", launch_shape<3, 2>}, {"d 8 x 128 B + 16 x 64 B, 4 ahead (one wave)", launch_shape<3, 4>},
      {"float4 stream, 1 KB of a row per instruction", launch_stream}};
  constexpr int NC = sizeof(cases) / sizeof(cases[0]);
  std::vector<float> us[NC];
  int launches = 0;
  for (int r = 0; r < reps + 1; ++r) {   // round 0 = warm-up, not recorded; the shapes alternate inside every round
    for (int c = 0; c < NC; ++c) {
      hipLaunchKernelGGL(flush_kernel, dim3(2048), dim3(256), 0, st, scratch, scratch_n4);
      CK(hipEventRecord(e0, st));
      cases[c].launch(x, gate, st);
      CK(hipEventRecord(e1, st));
      CK(hipEventSynchronize(e1));
      CK(hipGetLastError());
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r) us[c].push_back(ms * 1e3f);
      ++launches;
    }
  }
  // every element was touched exactly once per launch
  std::vector<float> hx(n);
  CK(hipMemcpy(hx.data(), x, n * 4, hipMemcpyDeviceToHost));
  size_t bad = 0;
  for (size_t i = 0; i < n; ++i) bad += hx[i] != (float)launches * hg[i % N];
  printf("rmw_shape_probe: x[%d][%d] fp32 (%.1f MB), 256 workgroups x 8 waves, %d timed launches per shape, cold buffer\n", M, N, n * 4 / 1e6, reps);
  printf("check: %zu of %zu elements differ from launches * gate (%s)\n", bad, n, bad ? "FAIL" : "ok");
  printf("%-50s %9s %9s %9s %8s\n", "shape", "min us", "median us", "max us", "TB/s med");
  for (int c = 0; c < NC; ++c) {
    std::sort(us[c].begin(), us[c].end());
    const float med = us[c][us[c].size() / 2];
    printf("%-50s %9.1f %9.1f %9.1f %8.2f\n", cases[c].name, us[c].front(), med, us[c].back(), 2.0 * n * 4 / (med * 1e-6) / 1e12);
  }
  return bad ? 1 : 0;
}
