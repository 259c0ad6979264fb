// Training batches from stored VAE moments: gather rows of a moment store [n_rows, 8, hw] (fp32 or f16; channels
// 0..3 the mean, 4..7 the logvar: latte_vae_encode's out_mode 0) and draw the posterior on them, in one launch per 256 output rows.
// latte_moment_sample of include/latte_amd.h.  gfx950 only.
#include "common.h"
#include "device_util.h"

namespace latte {

namespace {

constexpr int MOMENT_ROWS_PER_LAUNCH = 256;
// The source rows of one launch, passed BY VALUE in the kernel arguments (2 KiB): the launch copies them, so there is no staging buffer
// whose lifetime a later call could end, and no host synchronisation.  Read with a block-uniform index (blockIdx.y): scalar loads.
struct MomentRows {
  long long r[MOMENT_ROWS_PER_LAUNCH];
};

// Eight consecutive elements of the store from element e (a multiple of 8): one 16-byte access of halves, two of floats.
__device__ __forceinline__ void moment_load8(const void* __restrict__ store, int store_half, size_t e, float (&v)[8]) {
  if (store_half) {
    const uint4 u = *(const uint4*)((const unsigned short*)store + e);
    unpack2<LATTE_DTYPE_F16>(u.x, v[0], v[1]);
    unpack2<LATTE_DTYPE_F16>(u.y, v[2], v[3]);
    unpack2<LATTE_DTYPE_F16>(u.z, v[4], v[5]);
    unpack2<LATTE_DTYPE_F16>(u.w, v[6], v[7]);
  } else {
    const float4 a = *(const float4*)((const float*)store + e), b = *(const float4*)((const float*)store + e + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}

// grid (ceil(octs / 256), rows of this launch): block row y is output row row0 + y = store row rows.r[y].  One thread per OCT, eight
// consecutive elements of one channel (hw % 8 == 0, so an oct never leaves its channel):
//   what 0: out [n, 8, hw] = the row, upcast -- octs = hw per row;
//   what 1 | 2: out [n, 4, hw] = posterior_value(mean, logvar, z) -- octs = hw / 2 per row; the mean oct at channel c and the logvar oct
//   at channel 4 + c, two float4 of noise and of out.  z: the caller's slab [n, 4, hw], or (noise == NULL) drawn here: output element i
//   takes what fill_normal_kernel(seed, offset) writes at i (oct g of the WHOLE call = element quads 2 g and 2 g + 1).
// Every index is 64-bit: rows.r[y] * 8 * hw * 2 bytes passes 2^32 for any real data set.
__global__ void __launch_bounds__(256) moment_sample_kernel(const void* __restrict__ store, int store_half, MomentRows rows, int row0, int hw,
                                                            const float* __restrict__ noise, unsigned long long seed,
                                                            unsigned long long offset, float scale, int what, float* __restrict__ out) {
  const int octs = what == 0 ? hw : hw >> 1;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= octs) return;
  const size_t src = (size_t)rows.r[blockIdx.y] * 8 * (size_t)hw;   // first element of the store row
  const size_t g = ((size_t)row0 + blockIdx.y) * (size_t)octs + o;    // this oct among the call's output octs
  float v[8];
  if (what == 0) {
    moment_load8(store, store_half, src + (size_t)o * 8, v);
  } else {
    float mean[8], lv[8], z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    moment_load8(store, store_half, src + (size_t)o * 8, mean);
    moment_load8(store, store_half, src + (size_t)4 * hw + (size_t)o * 8, lv);
    if (what == 2) {
      if (noise) {
        const float4 a = ((const float4*)noise)[2 * g], b = ((const float4*)noise)[2 * g + 1];
        z[0] = a.x; z[1] = a.y; z[2] = a.z; z[3] = a.w;
        z[4] = b.x; z[5] = b.y; z[6] = b.z; z[7] = b.w;
      } else {
        float za[4], zb[4];
        philox_normal_quad(seed, offset, 2 * g, za);
        philox_normal_quad(seed, offset, 2 * g + 1, zb);
#pragma unroll
        for (int j = 0; j < 4; ++j) { z[j] = za[j]; z[4 + j] = zb[j]; }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = posterior_value(mean[j], lv[j], &z[j], scale, what);
  }
  ((float4*)out)[2 * g] = make_float4(v[0], v[1], v[2], v[3]);
  ((float4*)out)[2 * g + 1] = make_float4(v[4], v[5], v[6], v[7]);
}

}  // namespace

}  // namespace latte

using namespace latte;

extern "C" {

int latte_moment_sample(const void* store, int store_half, int64_t n_rows, int hw, const int64_t* rows, int n_out, const float* noise,
                        uint64_t seed, uint64_t offset, float scale, int what, float* out, void* stream) {
  if (!store || !rows || !out) return fail(LATTE_ERR_INVALID, "moment_sample: null argument");
  if (store_half != 0 && store_half != 1) return fail(LATTE_ERR_INVALID, "moment_sample: store_half must be 0 (fp32) or 1 (f16)");
  if (n_rows <= 0 || hw <= 0 || n_out <= 0) return fail(LATTE_ERR_INVALID, "moment_sample: bad shape");
  if (hw % 8) return fail(LATTE_ERR_INVALID, "moment_sample: H * W must be a multiple of 8 (16-byte accesses of eight halves)");
  if (what < 0 || what > 2) return fail(LATTE_ERR_INVALID, "moment_sample: what must be 0 (moments), 1 (mode) or 2 (sample)");
  if (what == 2 && !noise && seed == LATTE_SEED_NONE)
    return fail(LATTE_ERR_INVALID, "moment_sample: sample needs noise or a seed (noise == NULL with seed == LATTE_SEED_NONE)");
  if ((uintptr_t)store % 16 || (uintptr_t)out % 16 || (what == 2 && (uintptr_t)noise % 16))
    return fail(LATTE_ERR_INVALID, "moment_sample: store, noise and out must be 16-byte aligned");
  // every row before anything is launched: a wrong table can never read outside the store, and a refused call leaves out untouched
  for (int r = 0; r < n_out; ++r)
    if (rows[r] < 0 || rows[r] >= n_rows)
      return fail(LATTE_ERR_INVALID, "moment_sample: rows[" + std::to_string(r) + "] = " + std::to_string((long long)rows[r]) +
                                         " is outside the store's " + std::to_string((long long)n_rows) + " rows");
  const int octs = what == 0 ? hw : hw / 2;
  MomentRows mr;
  for (int row0 = 0; row0 < n_out; row0 += MOMENT_ROWS_PER_LAUNCH) {
    const int m = n_out - row0 < MOMENT_ROWS_PER_LAUNCH ? n_out - row0 : MOMENT_ROWS_PER_LAUNCH;
    for (int r = 0; r < MOMENT_ROWS_PER_LAUNCH; ++r) mr.r[r] = r < m ? (long long)rows[row0 + r] : 0;
    hipLaunchKernelGGL(moment_sample_kernel, dim3((octs + 255) / 256, m), dim3(256), 0, (hipStream_t)stream, store, store_half, mr, row0, hw,
                       what == 2 ? noise : nullptr, (unsigned long long)seed, (unsigned long long)offset, scale, what, out);
    LATTE_HIP(hipGetLastError());
  }
  return LATTE_OK;
}

}  // extern "C"
