// LoRA fine-tuning of the four block linears (DESIGN.md 4.4 "LoRA"): y = x W_eff^T + b with W_eff = W + s B A, W [N, K] and b frozen,
// A [r, K] and B [N, r] trained, s = alpha / r.  The forward and every input-gradient GEMM run on the MERGED half operand copies
// (lora_pack_kernel writes half(W + s B A) where the plain pack writes half(W)), so the only new work of a step is the adapter
// gradients behind dY [M, N] (loss-scaled domain, as every dY of the backward):
//     h = s x A^T  [M, r]      g = s dY B  [M, r]      dB = dY^T h  [N, r]      dA = g^T x  [r, K]
// (s rides on h instead of on dB: h has no other reader).  h and g are kept as split pairs [hi | lo]: hi = the half nearest to the
// value, lo = half((value - hi) 2^LO_SHIFT): ~2 x the mantissa, and the scaled remainder keeps what falls below f16's normal range
// (g = s dY B is a few percent of a dY that is itself small).  On the test fixture the pair moved the worst adapter gradient from
// 6.2e-4 to 6.1e-4 relative L2 only -- what is left is the training step's own error plus the half rounding of the operand copies
// A_h / Bt_h (tests/test_lora_training.py) -- so the pair is insurance for small gradients, not what holds the bound.  Two bodies on the 16x16x32 MFMA with fp32 accumulation:
//   lora_down_kernel    row-local  small[M, 2 R16] = [hi | lo] of scale * big[M, Kbig] Wd[R16, Kbig]^T; R16 = r padded to a multiple
//                       of 16 with zero rows in the half copy of Wd.  32 or 64 rows per workgroup, the contraction split over its four waves in
//                       128-column chunks and summed through LDS in wave order; both operands come straight from global memory
//                       (a lane's four fragments of a chunk are 64 contiguous bytes: the contraction slots are permuted alike for
//                       both operands, so the product is exact).
//   lora_outer_kernel   partial[chunk][R16 x 128 columns] = (hi + lo 2^-LO_SHIFT)[rows of chunk, R16]^T big[rows of chunk, 128 columns]
//                       (two accumulators, joined at the store): the contraction runs over rows, so both tiles are staged row-major
//                       in LDS and the fragments come out through the hardware transpose read exactly as in gemm_tn.hip (same slot permutation for both operands).  The
//                       partials are stored in the adapter's own layout -- [r, Kbig] for dA, [Kbig, r] for dB, padding rows never
//                       stored -- and launch_split_reduce sums them in chunk order (no atomics), unscales and assigns / adds.
// lora_operands_kernel writes the zero-padded half copies A_h [R16, K] and Bt_h [R16, N] the down launches read.
#include <algorithm>

#include "common.h"
#include "mfma_util.h"

namespace latte {
namespace {

// the remainder half of a split pair is scaled into the operand type's normal range: x 2^(mantissa bits + 1)
template <int DT>
constexpr float lo_scale() { return DT == LATTE_DTYPE_BF16 ? 256.0f : 2048.0f; }

// W_eff[n][k] = W + s sum_j B[n][j] A[j][k]: fp32, the rank index ascending, one fma per term and one for the sum -- the pack and
// the merge entry share this body, so half(merged fp32 weight) is the pack's half bit for bit.  A zero sum (B = 0, the initial
// state) leaves W's own bits.
// (the sum: acc = fma(B[n][j], A[j][k], acc) for j = 0 .. r - 1 from 0, in lora_pack_kernel)
__device__ __forceinline__ float lora_join(float w, float s, float acc) { return acc == 0.f ? w : __builtin_fmaf(s, acc, w); }

// One launch for every block weight (the tile plan of pack_weights_kernel, train_fin.hip).  wf == nullptr: the half operand copies
// [N, K] and [K, N] of W_eff (untargeted linears: of W); wf != nullptr: the fp32 W_eff itself, targeted linears only (merge entry).
template <int DT>
__global__ void __launch_bounds__(256) lora_pack_kernel(const LoraPackDesc* __restrict__ descs, PackPlan pl, int r, float s) {
  __shared__ float tile[32][33];
  __shared__ float As[64][32];
  __shared__ float Bs[32][65];
  const int blk = blockIdx.x / pl.tiles_per_block;
  int t = blockIdx.x - blk * pl.tiles_per_block;
  const int j = (t >= pl.tile0[1]) + (t >= pl.tile0[2]) + (t >= pl.tile0[3]);
  t -= pl.tile0[j];
  const LoraPackDesc d = descs[blk * 4 + j];
  if (d.wf && !d.A) return;   // merge: nothing to add (block-uniform)
  const int tk = (d.K + 31) >> 5;
  const int n0 = (t / tk) * 32, k0 = (t % tk) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  if (d.A) {
    for (int q = ty; q < r; q += 8) As[q][tx] = k0 + tx < d.K ? d.A[(size_t)q * d.K + k0 + tx] : 0.f;
    for (int i = threadIdx.x; i < 32 * r; i += 256) {
      const int row = i / r, q = i - row * r;
      Bs[row][q] = n0 + row < d.N ? d.B[(size_t)(n0 + row) * r + q] : 0.f;
    }
    __syncthreads();
  }
  // a thread owns column tx of rows ty + 8 i: one read of A[j][tx] serves its four sums (one fma chain per element, rank index ascending)
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (d.A) {
    for (int q = 0; q < r; ++q) {
      const float a = As[q][tx];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(Bs[ty + 8 * i][q], a, acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = ty + 8 * i;
    float v = 0.f;
    if (n0 + row < d.N && k0 + tx < d.K) {
      const size_t at = (size_t)(n0 + row) * d.K + k0 + tx;
      v = lora_join(d.w[at], s, acc[i]);
      if (d.wf) d.wf[at] = v;
      else d.wn[at] = f2h<DT>(v);
    }
    tile[row][tx] = v;
  }
  if (d.wf) return;
  __syncthreads();
  for (int row = ty; row < 32; row += 8)
    if (k0 + row < d.K && n0 + tx < d.N) d.wt[(size_t)(k0 + row) * d.N + n0 + tx] = f2h<DT>(tile[tx][row]);
}

// a_h [R16, K] = half(A), bt_h [R16, N] = half(B)^T, rows r .. R16 - 1 zero; blockIdx.y = table entry
template <int DT>
__global__ void __launch_bounds__(256) lora_operands_kernel(const LoraPackDesc* __restrict__ descs, int r, int R16) {
  const LoraPackDesc d = descs[blockIdx.y];
  if (!d.A) return;
  const size_t na = (size_t)R16 * d.K, nb = (size_t)R16 * d.N;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += (size_t)gridDim.x * 256) {
    if (i < na) {
      const int q = (int)(i / d.K);
      d.a_h[i] = q < r ? f2h<DT>(d.A[i]) : (half_t)0;
    } else {
      const size_t o = i - na;
      const int q = (int)(o / d.N), n = (int)(o - (size_t)q * d.N);
      d.bt_h[o] = q < r ? f2h<DT>(d.B[(size_t)n * r + q]) : (half_t)0;
    }
  }
}

// ------------------------------------------------------------------------------------------------ down
// RT = R16 / 16 column tiles of the small output; TR row tiles of 16 rows per workgroup: 4 at rank 64 (the Wd fragments, read from L2, are
// reused by four row tiles), 2 below (twice the workgroups: at M = 20 480, 320 workgroups of 64 rows left the 256 CUs short of loads in flight)
template <int DT, int RT, int TR>
__global__ void __launch_bounds__(256) lora_down_kernel(const half_t* __restrict__ big, const half_t* __restrict__ wd,
                                                        half_t* __restrict__ out, int M, int Kbig, float scale) {
  constexpr int R16 = RT * 16;
  constexpr int ROWS = 16 * TR;
  extern __shared__ __attribute__((aligned(16))) char down_smem[];
  float (*red)[ROWS][R16] = (float (*)[ROWS][R16])down_smem;   // [4]: every wave's partial sums
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fl = lane & 15, gq = lane >> 4;
  const int m0 = blockIdx.x * (16 * TR);
  f32x4 acc[TR][RT];
#pragma unroll
  for (int t = 0; t < TR; ++t)
#pragma unroll
    for (int n = 0; n < RT; ++n) acc[t][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int chunks = Kbig >> 7;
  for (int c = wave; c < chunks; c += 4) {
    // MFMA s of the chunk contracts k = 128 c + 32 s + 8 gq + {0..7} in lane group gq: one load instruction takes 64 contiguous bytes
    // of each of its 16 rows
    const int kb = c * 128 + gq * 8;
    u32x4 a[TR][4], b[RT][4];
#pragma unroll
    for (int t = 0; t < TR; ++t) {
      const u32x4* p = (const u32x4*)(big + (size_t)(m0 + 16 * t + fl) * Kbig + kb);
#pragma unroll
      for (int s = 0; s < 4; ++s) a[t][s] = p[4 * s];
    }
#pragma unroll
    for (int n = 0; n < RT; ++n) {
      const u32x4* p = (const u32x4*)(wd + (size_t)(16 * n + fl) * Kbig + kb);
#pragma unroll
      for (int s = 0; s < 4; ++s) b[n][s] = p[4 * s];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int t = 0; t < TR; ++t)
#pragma unroll
        for (int n = 0; n < RT; ++n) acc[t][n] = mfma16<DT>(a[t][s], b[n][s], acc[t][n]);   // D[m = 4 gq + reg][column fl]
  }
#pragma unroll
  for (int t = 0; t < TR; ++t)
#pragma unroll
    for (int n = 0; n < RT; ++n)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[wave][16 * t + 4 * gq + q][16 * n + fl] = acc[t][n][q];
  __syncthreads();
  // every thread joins four neighbouring columns in wave order and stores 8 bytes of hi and 8 of lo
  for (int i = threadIdx.x; i < ROWS * (R16 / 4); i += 256) {
    const int row = i / (R16 / 4), col = (i % (R16 / 4)) * 4;
    const float4 p0 = *(const float4*)&red[0][row][col], p1 = *(const float4*)&red[1][row][col];
    const float4 p2 = *(const float4*)&red[2][row][col], p3 = *(const float4*)&red[3][row][col];
    const float v[4] = {(((p0.x + p1.x) + p2.x) + p3.x) * scale, (((p0.y + p1.y) + p2.y) + p3.y) * scale,
                        (((p0.z + p1.z) + p2.z) + p3.z) * scale, (((p0.w + p1.w) + p2.w) + p3.w) * scale};
    half_t hi[4], lo[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      hi[q] = f2h<DT>(v[q]);
      lo[q] = f2h<DT>((v[q] - h2f<DT>(hi[q])) * lo_scale<DT>());
    }
    half_t* o = out + (size_t)(m0 + row) * (2 * R16) + col;
    *(uint2*)o = make_uint2((unsigned)hi[0] | ((unsigned)hi[1] << 16), (unsigned)hi[2] | ((unsigned)hi[3] << 16));
    *(uint2*)(o + R16) = make_uint2((unsigned)lo[0] | ((unsigned)lo[1] << 16), (unsigned)lo[2] | ((unsigned)lo[3] << 16));
  }
}

// ------------------------------------------------------------------------------------------------ outer
struct OuterArgs {
  const half_t* small;   // [M, 2 R16]: hi | lo
  const half_t* big;     // [M, Kbig]
  float* out;            // [chunks][r_valid Kbig]
  int M, Kbig, m_chunk, r_valid;
};
// KR: the partials are [Kbig][r_valid] (dB's layout), else [r_valid][Kbig] (dA's).  Either way a lane's four accumulator registers are
// four consecutive floats of the output: the MFMA's row index is the layout's fast index.
template <int DT, int RT, bool KR>
__global__ void __launch_bounds__(256) lora_outer_kernel(OuterArgs g) {
  constexpr int R16 = RT * 16;
  constexpr int PB = 288, PS = 64 * RT + 32;              // odd multiples of 32 B: the transpose reads of gemm_tn.hip
  constexpr int IMGB = 64 * PB, IMGS = 64 * PS, STG = IMGB + IMGS;
  constexpr int CHS = R16 / 4;                            // 16-byte chunks per row of the small tile (hi | lo)
  constexpr int JS = (64 * CHS + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 stages x (big image + small image)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fl = lane & 15, gq = lane >> 4;
  const int k0 = blockIdx.x * 128;
  const int m_begin = blockIdx.y * g.m_chunk;
  const int m_end = min(g.M, m_begin + g.m_chunk);
  float* outp = g.out + (size_t)blockIdx.y * g.r_valid * g.Kbig;
  const int brow = tid >> 4, bch = tid & 15;
  auto load_tiles = [&](int m0, u32x4* rb, u32x4* rs) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + brow + 16 * j;
      rb[j] = (u32x4){0u, 0u, 0u, 0u};
      if (m < m_end) rb[j] = *(const u32x4*)(g.big + (size_t)m * g.Kbig + k0 + bch * 8);
    }
#pragma unroll
    for (int j = 0; j < JS; ++j) {
      const int i = tid + 256 * j, m = m0 + i / CHS;
      rs[j] = (u32x4){0u, 0u, 0u, 0u};
      if (i < 64 * CHS && m < m_end) rs[j] = *(const u32x4*)(g.small + (size_t)m * (2 * R16) + (i % CHS) * 8);
    }
  };
  auto store_tiles = [&](int buf, const u32x4* rb, const u32x4* rs) {
    char* b = smem + buf * STG;
    char* s = b + IMGB;
#pragma unroll
    for (int j = 0; j < 4; ++j) *(u32x4*)(b + (brow + 16 * j) * PB + bch * 16) = rb[j];
#pragma unroll
    for (int j = 0; j < JS; ++j) {
      const int i = tid + 256 * j;
      if (i < 64 * CHS) *(u32x4*)(s + (i / CHS) * PS + (i % CHS) * 16) = rs[j];
    }
  };
  f32x4 acc[RT][2], acl[RT][2];   // the products of hi and of lo
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = acl[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  u32x4 rb[4], rs[JS];
  load_tiles(m_begin, rb, rs);
  store_tiles(0, rb, rs);
  __syncthreads();
  int buf = 0;
  for (int m0 = m_begin; m0 < m_end; m0 += 64, buf ^= 1) {
    const bool more = m0 + 64 < m_end;
    if (more) load_tiles(m0 + 64, rb, rs);
    const char* b = smem + buf * STG;
    const char* s = b + IMGB;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      // fragment of column block c: contraction rows {32 ks + 4 gq + 0..3} and {+16}, the same slots for both operands
      const int rrow = 32 * ks + 4 * gq + (fl >> 2), rcol = (fl & 3) * 8;
      u32x4 sf[2 * RT], bf[2];   // column blocks 0 .. RT - 1: hi, RT .. 2 RT - 1: lo
#pragma unroll
      for (int c = 0; c < 2 * RT; ++c) {
        const char* p = s + rrow * PS + rcol + c * 32;
        const u32x2 lo = lds_tr16(p), hi = lds_tr16(p + 16 * PS);
        sf[c] = (u32x4){lo[0], lo[1], hi[0], hi[1]};
      }
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const char* p = b + rrow * PB + rcol + (wave * 2 + c) * 32;
        const u32x2 lo = lds_tr16(p), hi = lds_tr16(p + 16 * PB);
        bf[c] = (u32x4){lo[0], lo[1], hi[0], hi[1]};
      }
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if constexpr (KR) {   // D[r = 4 gq + reg][k = fl]
            acc[i][j] = mfma16<DT>(sf[i], bf[j], acc[i][j]);
            acl[i][j] = mfma16<DT>(sf[RT + i], bf[j], acl[i][j]);
          } else {              // D[k = 4 gq + reg][r = fl]
            acc[i][j] = mfma16<DT>(bf[j], sf[i], acc[i][j]);
            acl[i][j] = mfma16<DT>(bf[j], sf[RT + i], acl[i][j]);
          }
        }
    }
    if (more) store_tiles(buf ^ 1, rb, rs);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      constexpr float IL = 1.0f / lo_scale<DT>();
      const float4 v = make_float4(acc[i][j][0] + acl[i][j][0] * IL, acc[i][j][1] + acl[i][j][1] * IL, acc[i][j][2] + acl[i][j][2] * IL,
                                   acc[i][j][3] + acl[i][j][3] * IL);
      if constexpr (KR) {
        const int r0 = 16 * i + 4 * gq, k = k0 + wave * 32 + 16 * j + fl;
        if (r0 < g.r_valid) *(float4*)(outp + (size_t)k * g.r_valid + r0) = v;
      } else {
        const int r = 16 * i + fl, k = k0 + wave * 32 + 16 * j + 4 * gq;
        if (r < g.r_valid) *(float4*)(outp + (size_t)r * g.Kbig + k) = v;
      }
    }
}

int lora_r16(int r) { return (r + 15) / 16 * 16; }
bool rank_ok(int r) { return r == 4 || r == 8 || r == 16 || r == 32 || r == 64; }

}  // namespace

// rows per partial of the outer product (a multiple of 64) -> number of partials: about two workgroups per CU, and never more
// partial bytes than a handful of passes over the big operand
int lora_outer_plan(int M, int Kbig, int* chunk) {
  const int tiles = std::max(1, Kbig / 128);
  const int splits = std::max(1, std::min(M / 64, (512 + tiles - 1) / tiles));
  *chunk = ((M + splits - 1) / splits + 63) / 64 * 64;
  return (M + *chunk - 1) / *chunk;
}

int launch_lora_down(const half_t* big, const half_t* wd, half_t* out, int M, int Kbig, int r, float scale, int dtype, hipStream_t st) {
  if (!rank_ok(r) || M <= 0 || M % 64 || Kbig <= 0 || Kbig % 128) return fail(LATTE_ERR_INVALID, "lora_down: need rank in {4, 8, 16, 32, 64}, M % 64 == 0, Kbig % 128 == 0");
  const int rows = lora_r16(r) == 64 ? 64 : 32;   // rows per workgroup (the kernel's TR)
  if ((uint64_t)M * Kbig >= (1ull << 40)) return fail(LATTE_ERR_INVALID, "lora_down: operand too large");
  const int rt = lora_r16(r) / 16;
  const dim3 grid(M / rows), block(256);
  const int lds = 4 * rows * lora_r16(r) * 4;   // the four waves' partial sums (64 KB at rank 64)
#define CALL(DT, RT, TR) launch_lds<lora_down_kernel<DT, RT, TR>>(grid, block, lds, st, big, wd, out, M, Kbig, scale)
#define BY_RT(DT) (rt == 1 ? CALL(DT, 1, 2) : rt == 2 ? CALL(DT, 2, 2) : CALL(DT, 4, 4))
  if (dtype == LATTE_DTYPE_BF16) return BY_RT(LATTE_DTYPE_BF16);
  if (dtype == LATTE_DTYPE_F16) return BY_RT(LATTE_DTYPE_F16);
#undef BY_RT
#undef CALL
  return fail(LATTE_ERR_INVALID, "lora_down: unknown dtype");
}

// partial: float [ceil(M / m_chunk)][r Kbig]; kr != 0: each partial is [Kbig][r] (dB), else [r][Kbig] (dA)
int launch_lora_outer(const half_t* small, const half_t* big, float* partial, int M, int Kbig, int r, int m_chunk, int kr, int dtype,
                      hipStream_t st) {
  if (!rank_ok(r) || M <= 0 || M % 64 || Kbig <= 0 || Kbig % 128 || m_chunk <= 0 || m_chunk % 64)
    return fail(LATTE_ERR_INVALID, "lora_outer: need rank in {4, 8, 16, 32, 64}, M % 64 == 0, Kbig % 128 == 0, m_chunk % 64 == 0");
  const int rt = lora_r16(r) / 16;
  OuterArgs a{small, big, partial, M, Kbig, m_chunk, r};
  const dim3 grid(Kbig / 128, (M + m_chunk - 1) / m_chunk), block(256);
  const int lds = 2 * (64 * 288 + 64 * (64 * rt + 32));
#define CALL(DT, RT) (kr ? launch_lds<lora_outer_kernel<DT, RT, true>>(grid, block, lds, st, a) \
                         : launch_lds<lora_outer_kernel<DT, RT, false>>(grid, block, lds, st, a))
#define BY_RT(DT) (rt == 1 ? CALL(DT, 1) : rt == 2 ? CALL(DT, 2) : CALL(DT, 4))
  if (dtype == LATTE_DTYPE_BF16) return BY_RT(LATTE_DTYPE_BF16);
  if (dtype == LATTE_DTYPE_F16) return BY_RT(LATTE_DTYPE_F16);
#undef BY_RT
#undef CALL
  return fail(LATTE_ERR_INVALID, "lora_outer: unknown dtype");
}

// descs_dev: LoraPackDesc [blocks][4].  Entries with wf set receive the fp32 merged weight instead of the half copies.
int launch_pack_weights_lora(const LoraPackDesc* descs_dev, int blocks, const PackPlan& pl, int r, float s, int dtype, hipStream_t st) {
  if (!rank_ok(r)) return fail(LATTE_ERR_INVALID, "pack_weights_lora: rank must be one of 4, 8, 16, 32, 64");
  const dim3 grid(blocks * pl.tiles_per_block);
  if (dtype == LATTE_DTYPE_BF16) hipLaunchKernelGGL(lora_pack_kernel<LATTE_DTYPE_BF16>, grid, dim3(256), 0, st, descs_dev, pl, r, s);
  else if (dtype == LATTE_DTYPE_F16) hipLaunchKernelGGL(lora_pack_kernel<LATTE_DTYPE_F16>, grid, dim3(256), 0, st, descs_dev, pl, r, s);
  else return fail(LATTE_ERR_INVALID, "pack_weights_lora: unknown dtype");
  LATTE_HIP(hipGetLastError());
  return LATTE_OK;
}

int launch_lora_operands(const LoraPackDesc* descs_dev, int entries, int r, int dtype, hipStream_t st) {
  if (!rank_ok(r)) return fail(LATTE_ERR_INVALID, "lora_operands: rank must be one of 4, 8, 16, 32, 64");
  const dim3 grid(64, entries);
  if (dtype == LATTE_DTYPE_BF16) hipLaunchKernelGGL(lora_operands_kernel<LATTE_DTYPE_BF16>, grid, dim3(256), 0, st, descs_dev, r, lora_r16(r));
  else if (dtype == LATTE_DTYPE_F16) hipLaunchKernelGGL(lora_operands_kernel<LATTE_DTYPE_F16>, grid, dim3(256), 0, st, descs_dev, r, lora_r16(r));
  else return fail(LATTE_ERR_INVALID, "lora_operands: unknown dtype");
  LATTE_HIP(hipGetLastError());
  return LATTE_OK;
}

}  // namespace latte
