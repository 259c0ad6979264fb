// Device helpers shared by every .hip file that are not about MFMA fragments (those: mfma_util.h): half <-> fp32 conversions on
// bit patterns, the 64-lane sum, SiLU and the GELU(tanh) pair, and the FP4 block quantisation.  gfx950 only.
#pragma once
#include "common.h"

namespace latte {
namespace {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// half bits -> fp32: one value, the two halves of a word, the four halves of two words
template <int DT>
__device__ __forceinline__ float h2f(unsigned short h) {
  if constexpr (DT == LATTE_DTYPE_BF16) return __builtin_bit_cast(float, (unsigned int)h << 16);
  else return (float)__builtin_bit_cast(_Float16, h);
}
template <int DT>
__device__ __forceinline__ void unpack2(unsigned int u, float& a, float& b) {
  if constexpr (DT == LATTE_DTYPE_BF16) {
    a = __builtin_bit_cast(float, u << 16);
    b = __builtin_bit_cast(float, u & 0xffff0000u);
  } else {
    const f16x2 h = __builtin_bit_cast(f16x2, u);
    a = (float)h[0];
    b = (float)h[1];
  }
}
template <int DT>
__device__ __forceinline__ void unpack4(const uint2 p, float& a, float& b, float& c, float& d) {
  a = h2f<DT>((unsigned short)(p.x & 0xffffu)); b = h2f<DT>((unsigned short)(p.x >> 16));
  c = h2f<DT>((unsigned short)(p.y & 0xffffu)); d = h2f<DT>((unsigned short)(p.y >> 16));
}

// fp32 -> the bits of the nearest half
__device__ __forceinline__ unsigned short h16_bits(_Float16 h) { return __builtin_bit_cast(unsigned short, h); }
template <int DT>
__device__ __forceinline__ unsigned short f2h(float v) {
  if constexpr (DT == LATTE_DTYPE_BF16) {
    const __bf16 h = (__bf16)v;
    return __builtin_bit_cast(unsigned short, h);
  } else {
    return h16_bits((_Float16)v);
  }
}

__device__ __forceinline__ float silu(float x) { return x / (1.0f + __expf(-x)); }

// GELU(tanh approximation) = x * sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3)   (latte.py:170)
// = x / (1 + exp2(x (a + b x^2))) with a = -2 log2(e) sqrt(2/pi), b = 0.044715 a: 3 mul + 1 fma + 1 add + exp2 + rcp.
// gelu_sig is the sigmoid factor alone (the backward needs it: gelu'(x) = s + x s (1 - s) 2 u', train.hip).
__device__ __forceinline__ float gelu_sig(float x) {
  const float p = __builtin_fmaf(x * x, -0.10294324f, -2.3022082f);
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(p * x));
}
__device__ __forceinline__ float gelu_tanh(float x) { return x * gelu_sig(x); }

// FP4 (e2m1) block quantisation with a power-of-two scale (round 6): the E8M0 exponent for a block whose largest magnitude is `amax`
// -- ONE BELOW the smallest e with amax / 2^e <= 6 (the format's largest value): the top binade of the block saturates at 6 and everything
// else gains a bit (remainders of N(0, 1)-like rows keep 1.7 - 2.2 % of their variance instead of 3 - 4.6 %, heavy-tailed rows 5.6 % instead
// of 12 %: simulation in DESIGN.md section 2), clamped to the scale byte's range -- and four values -> one
// half-word of four codes (element j in bits 4 j) by the hardware convert (round to nearest even, saturating at +-6).
__device__ __forceinline__ int quant4_exponent(float amax) {
  if (!(amax > 0.f)) return -127;
  int ex;
  const float m = __builtin_frexpf(amax * (1.0f / 6.0f), &ex);   // amax / 6 = m 2^ex, m in [0.5, 1)
  const int e = (m == 0.5f ? ex - 1 : ex) - 1;
  return e < -127 ? -127 : e > 127 ? 127 : e;
}
__device__ __forceinline__ unsigned int quant4_pk4(float v0, float v1, float v2, float v3, float scale_pow2) {
  unsigned int w = 0;
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v0, v1, scale_pow2, 0);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v2, v3, scale_pow2, 1);
  return w & 0xffffu;
}

// Philox4x32-10 (Salmon et al. 2011): counter = element-quad index, key = seed.
__device__ __forceinline__ void philox_round(unsigned int (&c)[4], unsigned int k0, unsigned int k1) {
  const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
  const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
  const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c[1] ^ k0;
  const unsigned int n1 = (unsigned int)p1;
  const unsigned int n2 = (unsigned int)(p0 >> 32) ^ c[3] ^ k1;
  const unsigned int n3 = (unsigned int)p0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

// The four standard normals of element quad q of a draw at (seed, offset): quad q covers elements [4q, 4q+4) of THAT draw; the counter
// is the global element-quad index.  The one definition of the stream: fill_normal_kernel, known_blend_kernel's inline draw
// (pointwise.hip) and moment_sample_kernel's (moments.hip).
__device__ __forceinline__ void philox_normal_quad(unsigned long long seed, unsigned long long offset, size_t q, float (&z)[4]) {
  const unsigned long long ctr = (offset >> 2) + q;
  unsigned int c[4] = {(unsigned int)ctr, (unsigned int)(ctr >> 32), (unsigned int)(offset & 3), 0u};
  unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = ((float)(c[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    z[2 * h] = r * cs;
    z[2 * h + 1] = r * sn;
  }
}

// One element of DiagonalGaussianDistribution from its mean and its RAW logvar (clamped to [-30, 20] here): what 1 mode * scale,
// 2 (mean + exp(0.5 logvar) *z) * scale (z is read for what 2 only), 3 logvar, 4 std, 5 var.  The one definition of that arithmetic:
// posterior_kernel (vae.hip) and moment_sample_kernel (moments.hip) agree bit for bit because both call this.
__device__ __forceinline__ float posterior_value(float mean, float logvar, const float* __restrict__ z, float scale, int what) {
#pragma clang fp contract(off)
  const float lv = fminf(fmaxf(logvar, -30.0f), 20.0f);
  if (what == 1) return mean * scale;
  if (what == 2) return (mean + expf(0.5f * lv) * *z) * scale;
  if (what == 3) return lv;
  if (what == 4) return expf(0.5f * lv);
  return expf(lv);
}

}  // namespace
}  // namespace latte
