// T5 v1.1 encoder kernels (gfx950): embedding gather, RMSNorm from the fp32 residual stream, the relative-position bias table,
// self-attention with a per-head (key - query) bias and a per-sample key mask on unscaled scores, the gated activation, and the
// small-M weight-streaming projection  C[M, N] = A[M, K] . W[N, K]^T  with split operand pairs on both sides.
//
// Operand scheme (f16): every projection operand X is carried as the pair  hi = f16(X),  lo = f16((X - hi) * 2^11)  (T5_LO_SCALE keeps
// the remainder of small weights out of the f16 subnormals), and a product is  Ahi.Whi + 2^-11 (Alo.Whi + Ahi.Wlo)  in two fp32
// accumulators; the lo.lo term (2^-22) is dropped.  Attention takes q, k, v and the probabilities as plain f16.
#include <algorithm>

#include "mfma_util.h"

namespace latte {
namespace {

constexpr float T5_LO_SCALE = 2048.f, T5_LO_INV = 1.f / 2048.f;
constexpr float F16_MAX = 65504.f;

__device__ __forceinline__ void split_lo(float v, _Float16& hi, _Float16& lo) {
  const float c = __builtin_fminf(__builtin_fmaxf(v, -F16_MAX), F16_MAX);
  hi = (_Float16)c;
  const float r = (v - (float)hi) * T5_LO_SCALE;
  lo = (_Float16)__builtin_fminf(__builtin_fmaxf(r, -F16_MAX), F16_MAX);
}

// ---- embedding gather: x[m, :] = table[ids[m], :] (no scaling); an id outside the vocabulary reads row 0
__global__ void t5_embed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ table, float* __restrict__ x, int D, int vocab) {
  const int m = blockIdx.x;
  int64_t id = ids[m];
  if (id < 0 || id >= vocab) id = 0;
  const float4* src = (const float4*)(table + (size_t)id * D);
  float4* dst = (float4*)(x + (size_t)m * D);
  for (int i = threadIdx.x; i < D / 4; i += blockDim.x) dst[i] = src[i];
}

// ---- x[m, :] += sum_s slab[s][m, :] (s ascending: a fixed order), then RMSNorm: y = w * x * rsqrt(mean(x^2) + eps), statistics fp32.
// y goes out as the split pair (out_hi / out_lo, [.., D]) or as fp32 (out_f32: the final layer norm).  One workgroup per row.
__global__ __launch_bounds__(256) void t5_res_norm_kernel(float* __restrict__ x, const float* __restrict__ slabs, int nsplit, size_t slab_stride,
                                                          const float* __restrict__ w, half_t* __restrict__ out_hi,
                                                          half_t* __restrict__ out_lo, float* __restrict__ out_f32, int D, float eps) {
  const int m = blockIdx.x, tid = threadIdx.x;
  float* xr = x + (size_t)m * D;
  float ss = 0.f;
  for (int i = tid; i < D; i += 256) {
    float v = xr[i];
    if (nsplit > 0) {
      for (int s = 0; s < nsplit; ++s) v += slabs[s * slab_stride + (size_t)m * D + i];
      xr[i] = v;
    }
    ss += v * v;
  }
  __shared__ float red[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  ss = (red[0] + red[1]) + (red[2] + red[3]);
  const float r = rsqrtf(ss / (float)D + eps);
  if (!w) return;   // residual add only
  for (int i = tid; i < D; i += 256) {
    const float y = w[i] * (xr[i] * r);
    if (out_f32) {
      out_f32[(size_t)m * D + i] = y;
    } else {
      _Float16 hi, lo;
      split_lo(y, hi, lo);
      out_hi[(size_t)m * D + i] = h16_bits(hi);
      out_lo[(size_t)m * D + i] = h16_bits(lo);
    }
  }
}

// ---- table[h][d] = rel[bucket[d]][h] for d = (key - query) + Lmax - 1 in [0, 2 Lmax - 1)
__global__ void t5_bias_table_kernel(const float* __restrict__ rel, const int* __restrict__ bucket, float* __restrict__ table, int heads,
                                     int span) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= heads * span) return;
  const int h = i / span, d = i - h * span;
  table[i] = rel[bucket[d] * heads + h];
}

// ---- weight pack: fp32 -> the split pair
__global__ void t5_pack_w_kernel(const float* __restrict__ w, half_t* __restrict__ hi, half_t* __restrict__ lo, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    _Float16 a, b;
    split_lo(w[i], a, b);
    hi[i] = h16_bits(a);
    lo[i] = h16_bits(b);
  }
}

// ---- q | k | v (f16, [M, N]) = sum of the projection's split-K slabs
__global__ void t5_reduce_h16_kernel(const float* __restrict__ slabs, int nsplit, size_t slab_stride, half_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = slabs[i];
  for (int s = 1; s < nsplit; ++s) v += slabs[s * slab_stride + i];
  v = __builtin_fminf(__builtin_fmaxf(v, -F16_MAX), F16_MAX);
  out[i] = h16_bits((_Float16)v);
}

__device__ __forceinline__ float gelu_new(float x) {
  return 0.5f * x * (1.f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}

// ---- h = gelu_new(u0) * u1 with [u0 | u1] = the [M, 2 F] product against [wi_0; wi_1] (slabs summed here), out as the split pair [M, F]
__global__ void t5_gated_act_kernel(const float* __restrict__ slabs, int nsplit, size_t slab_stride, half_t* __restrict__ out_hi,
                                    half_t* __restrict__ out_lo, int M, int F) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)M * F) return;
  const size_t m = i / F, f = i - m * F;
  const size_t a = m * 2 * F + f;
  float u0 = slabs[a], u1 = slabs[a + F];
  for (int s = 1; s < nsplit; ++s) {
    u0 += slabs[s * slab_stride + a];
    u1 += slabs[s * slab_stride + a + F];
  }
  _Float16 hi, lo;
  split_lo(gelu_new(u0) * u1, hi, lo);
  out_hi[i] = h16_bits(hi);
  out_lo[i] = h16_bits(lo);
}

// ---- small-M projection.  Workgroup = 4 waves = 64 output columns x up to 256 rows (blockIdx.z: row blocks of 256) x one K chunk
// (blockIdx.y).  Each wave owns one 16-column tile and streams its weight fragments straight from global memory to registers (read once
// per row block); the activation pair goes through LDS in 32-deep K steps, shared by the four waves.  The next step's global loads are
// issued before the current step's MFMAs.  The fp32 partial product of the chunk is written to slab blockIdx.y.
constexpr int PG_BK = 32, PG_PITCH = 40 /* halfs: 80-byte rows */, PG_ROWS = 256, PG_MT = 16;

__global__ __launch_bounds__(256) void t5_proj_kernel(const half_t* __restrict__ Ahi, const half_t* __restrict__ Alo,
                                                      const half_t* __restrict__ Whi, const half_t* __restrict__ Wlo,
                                                      float* __restrict__ slabs, size_t slab_stride, int M, int N, int K, int k_chunk) {
  __shared__ __attribute__((aligned(16))) half_t lds[2 * PG_ROWS * PG_PITCH];
  half_t* sh = lds;
  half_t* sl = lds + PG_ROWS * PG_PITCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.z * PG_ROWS;
  const int rows = min(M - row0, PG_ROWS);            // valid rows of this block (A is allocated in whole 256-row blocks)
  const int mtiles = (rows + 15) >> 4;
  const int k_begin = blockIdx.y * k_chunk, k_end = min(K, k_begin + k_chunk);
  const int n0 = blockIdx.x * 64 + wave * 16;
  // staging map: chunk c = tid + 256 i (i < 4) -> row c >> 2, 16-byte piece c & 3
  const half_t* ga_hi = Ahi + (size_t)(row0 + (tid >> 2)) * K + (tid & 3) * 8;
  const half_t* ga_lo = Alo + (size_t)(row0 + (tid >> 2)) * K + (tid & 3) * 8;
  const size_t w_off = (size_t)(n0 + (lane & 15)) * K + (lane >> 4) * 8;
  u32x4 ra_hi[4], ra_lo[4], rw_hi, rw_lo;
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra_hi[i] = *(const u32x4*)(ga_hi + (size_t)i * 64 * K + k0);
      ra_lo[i] = *(const u32x4*)(ga_lo + (size_t)i * 64 * K + k0);
    }
    rw_hi = *(const u32x4*)(Whi + w_off + k0);
    rw_lo = *(const u32x4*)(Wlo + w_off + k0);
  };
  f32x4 acc1[PG_MT], acc2[PG_MT];
#pragma unroll
  for (int i = 0; i < PG_MT; ++i) acc1[i] = acc2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  fetch(k_begin);
  for (int k0 = k_begin; k0 < k_end; k0 += PG_BK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = ((tid >> 2) + i * 64) * PG_PITCH + (tid & 3) * 8;
      *(u32x4*)(sh + off) = ra_hi[i];
      *(u32x4*)(sl + off) = ra_lo[i];
    }
    const u32x4 wh = rw_hi, wl = rw_lo;
    __syncthreads();
    if (k0 + PG_BK < k_end) fetch(k0 + PG_BK);
    const int frag = (lane & 15) * PG_PITCH + (lane >> 4) * 8;
#pragma unroll
    for (int mt = 0; mt < PG_MT; ++mt) {
      if (mt < mtiles) {
        const u32x4 ah = *(const u32x4*)(sh + mt * 16 * PG_PITCH + frag);
        const u32x4 al = *(const u32x4*)(sl + mt * 16 * PG_PITCH + frag);
        acc1[mt] = mfma16<LATTE_DTYPE_F16>(ah, wh, acc1[mt]);
        acc2[mt] = mfma16<LATTE_DTYPE_F16>(al, wh, acc2[mt]);
        acc2[mt] = mfma16<LATTE_DTYPE_F16>(ah, wl, acc2[mt]);
      }
    }
  }
  float* out = slabs + blockIdx.y * slab_stride;
  const int col = n0 + (lane & 15);
#pragma unroll
  for (int mt = 0; mt < PG_MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = mt * 16 + (lane >> 4) * 4 + r;
      if (row < rows) out[(size_t)(row0 + row) * N + col] = acc1[mt][r] + acc2[mt][r] * T5_LO_INV;
    }
  }
}

// ---- self-attention, hd = 64.  grid (ceil(L / 64), heads, B); a wave owns 16 query rows, the workgroup walks the keys in tiles of 64:
// K tile and V^T tile in LDS, scores on the MFMA (f16 operands), + table[h][key - query] and -inf on masked keys, online softmax in
// fp32, probabilities through a per-wave LDS tile into the second MFMA.  A masked key's weight is exactly 0.
constexpr int AT_PITCH = 72;   // halfs: 144-byte rows

__global__ __launch_bounds__(256) void t5_attention_kernel(const half_t* __restrict__ qkv, const float* __restrict__ table,
                                                           const float* __restrict__ mask, half_t* __restrict__ out_hi,
                                                           half_t* __restrict__ out_lo, int L, int heads, int Lmax) {
  __shared__ __attribute__((aligned(16))) half_t Ks[64 * AT_PITCH];
  __shared__ __attribute__((aligned(16))) half_t Vt[64 * AT_PITCH];
  __shared__ __attribute__((aligned(16))) half_t Ps[4 * 16 * AT_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.y, b = blockIdx.z;
  const int inner = heads * 64, ld = 3 * inner;
  const half_t* base = qkv + (size_t)b * L * ld;
  const int q0 = blockIdx.x * 64 + wave * 16;
  const int fr = lane & 15, fq = lane >> 4;
  // Q fragments (A operand): row q0 + fr, d = 32 s + 8 fq ..; rows past L read row L - 1 (never stored)
  u32x4 qf[2];
  {
    const int qr = min(q0 + fr, L - 1);
    const half_t* qp = base + (size_t)qr * ld + h * 64 + fq * 8;
    qf[0] = *(const u32x4*)qp;
    qf[1] = *(const u32x4*)(qp + 32);
  }
  const float* trow = table + (size_t)h * (2 * Lmax - 1) + (Lmax - 1);
  const float* mrow = mask ? mask + (size_t)b * L : nullptr;
  float m_run[4], l_run[4];
  f32x4 o[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = -1e30f; l_run[r] = 0.f; }
#pragma unroll
  for (int n = 0; n < 4; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  half_t* pw = Ps + wave * 16 * AT_PITCH;
  for (int kt = 0; kt < L; kt += 64) {
    __syncthreads();
    // stage: 512 16-byte pieces of K and of V; piece c -> key c >> 3, d = 8 (c & 7)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + i * 256, key = c >> 3, d8 = (c & 7) * 8;
      u32x4 kv = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
      if (kt + key < L) {
        const half_t* p = base + (size_t)(kt + key) * ld + h * 64 + d8;
        kv = *(const u32x4*)(p + inner);
        vv = *(const u32x4*)(p + 2 * inner);
      }
      *(u32x4*)(Ks + key * AT_PITCH + d8) = kv;
#pragma unroll
      for (int j = 0; j < 8; ++j) Vt[(d8 + j) * AT_PITCH + key] = (half_t)(vv[j >> 1] >> (16 * (j & 1)));
    }
    __syncthreads();
    f32x4 s[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      s[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const u32x4 kf = *(const u32x4*)(Ks + (n * 16 + fr) * AT_PITCH + ks * 32 + fq * 8);
        s[n] = mfma16<LATTE_DTYPE_F16>(qf[ks], kf, s[n]);
      }
    }
    // bias + mask; this lane: key kt + 16 n + fr, query rows q0 + 4 fq + r
    float tmax[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int key = kt + n * 16 + fr;
      const bool valid = key < L && (!mrow || mrow[key] > 0.5f);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = min(q0 + fq * 4 + r, L - 1);
        const float v = valid ? s[n][r] + trow[key - qrow] : -INFINITY;
        s[n][r] = v;
        tmax[r] = fmaxf(tmax[r], v);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) tmax[r] = fmaxf(tmax[r], __shfl_xor(tmax[r], off));
      const float m_new = fmaxf(m_run[r], tmax[r]);
      const float alpha = expf(m_run[r] - m_new);
      m_run[r] = m_new;
      float rs = 0.f;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const float p = expf(s[n][r] - m_new);
        // the probability the second product sees is the f16 one: sum the rounded value so that the row still sums to one
        const _Float16 ph = (_Float16)p;
        rs += (float)ph;
        pw[(fq * 4 + r) * AT_PITCH + n * 16 + fr] = h16_bits(ph);
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) rs += __shfl_xor(rs, off);
      l_run[r] = l_run[r] * alpha + rs;
#pragma unroll
      for (int n = 0; n < 4; ++n) o[n][r] *= alpha;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const u32x4 pf = *(const u32x4*)(pw + fr * AT_PITCH + ks * 32 + fq * 8);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const u32x4 vf = *(const u32x4*)(Vt + (n * 16 + fr) * AT_PITCH + ks * 32 + fq * 8);
        o[n] = mfma16<LATTE_DTYPE_F16>(pf, vf, o[n]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + fq * 4 + r;
    if (qrow >= L) continue;
    const float inv = l_run[r] > 0.f ? 1.f / l_run[r] : 0.f;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      _Float16 hi, lo;
      split_lo(o[n][r] * inv, hi, lo);
      const size_t idx = ((size_t)b * L + qrow) * inner + h * 64 + n * 16 + fr;
      out_hi[idx] = h16_bits(hi);
      out_lo[idx] = h16_bits(lo);
    }
  }
}

}  // namespace

int launch_t5_embed(const int64_t* ids, const float* table, float* x, int M, int D, int vocab, hipStream_t st) {
  if (M <= 0 || D % 4) return fail(LATTE_ERR_INVALID, "t5_embed: bad shape");
  hipLaunchKernelGGL(t5_embed_kernel, dim3(M), dim3(256), 0, st, ids, table, x, D, vocab);
  LATTE_HIP(hipGetLastError());
  return LATTE_OK;
}

int launch_t5_res_norm(float* x, const float* slabs, int nsplit, size_t slab_stride, const float* w, half_t* out_hi, half_t* out_lo,
                       float* out_f32, int M, int D, float eps, hipStream_t st) {
  if (M <= 0 || D <= 0 || (w && !out_f32 && (!out_hi || !out_lo))) return fail(LATTE_ERR_INVALID, "t5_res_norm: bad arguments");
  hipLaunchKernelGGL(t5_res_norm_kernel, dim3(M), dim3(256), 0, st, x, slabs, nsplit, slab_stride, w, out_hi, out_lo, out_f32, D, eps);
  LATTE_HIP(hipGetLastError());
  return LATTE_OK;
}

int launch_t5_bias_table(const float* rel, const int* bucket, float* table, int heads, int span, hipStream_t st) {
  const int n = heads * span;
  hipLaunchKernelGGL(t5_bias_table_kernel, dim3((n + 255) / 256), dim3(256), 0, st, rel, bucket, table, heads, span);
  LATTE_HIP(hipGetLastError());
  return LATTE_OK;
}

int launch_t5_pack_w(const float* w, half_t* hi, half_t* lo, size_t n, hipStream_t st) {
  const int blocks = (int)std::min<size_t>((n + 255) / 256, 65536);
  hipLaunchKernelGGL(t5_pack_w_kernel, dim3(blocks), dim3(256), 0, st, w, hi, lo, n);
  LATTE_HIP(hipGetLastError());
  return LATTE_OK;
}

int launch_t5_reduce_h16(const float* slabs, int nsplit, size_t slab_stride, half_t* out, size_t n, hipStream_t st) {
  hipLaunchKernelGGL(t5_reduce_h16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, slabs, nsplit, slab_stride, out, n);
  LATTE_HIP(hipGetLastError());
  return LATTE_OK;
}

int launch_t5_gated_act(const float* slabs, int nsplit, size_t slab_stride, half_t* out_hi, half_t* out_lo, int M, int F, hipStream_t st) {
  const size_t n = (size_t)M * F;
  hipLaunchKernelGGL(t5_gated_act_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, slabs, nsplit, slab_stride, out_hi, out_lo, M, F);
  LATTE_HIP(hipGetLastError());
  return LATTE_OK;
}

// K chunks of a projection: a function of (N, K) alone, so that a row's result does not depend on how many rows the call has
int t5_proj_splits(int N, int K) {
  int s = 512 / (N / 64);
  s = std::max(1, std::min(s, 8));
  while (s > 1 && (K % (s * PG_BK) != 0)) --s;
  return s;
}

// A pair: [rows rounded up to 256, K] (rows past M are read, never stored); W pair: [N, K]; slabs: t5_proj_splits(N, K) x slab_stride floats
int launch_t5_proj(const half_t* Ahi, const half_t* Alo, const half_t* Whi, const half_t* Wlo, float* slabs, size_t slab_stride, int M,
                   int N, int K, hipStream_t st) {
  if (M <= 0 || N % 64 || K % PG_BK) return fail(LATTE_ERR_INVALID, "t5_proj: N must be a multiple of 64 and K of 32");
  const int splits = t5_proj_splits(N, K);
  hipLaunchKernelGGL(t5_proj_kernel, dim3(N / 64, splits, (M + PG_ROWS - 1) / PG_ROWS), dim3(256), 0, st, Ahi, Alo, Whi, Wlo, slabs,
                     slab_stride, M, N, K, K / splits);
  LATTE_HIP(hipGetLastError());
  return LATTE_OK;
}

int launch_t5_attention(const half_t* qkv, const float* table, const float* mask, half_t* out_hi, half_t* out_lo, int B, int L, int heads,
                        int Lmax, hipStream_t st) {
  if (B <= 0 || L <= 0 || L > Lmax || heads <= 0) return fail(LATTE_ERR_INVALID, "t5_attention: bad shape");
  hipLaunchKernelGGL(t5_attention_kernel, dim3((L + 63) / 64, heads, B), dim3(256), 0, st, qkv, table, mask, out_hi, out_lo, L, heads, Lmax);
  LATTE_HIP(hipGetLastError());
  return LATTE_OK;
}

}  // namespace latte
