// Video preprocessing in front of the VAE encoder: the reference's per-item frame pipeline (datasets/__init__.py:13-76,
// datasets/video_transforms.py)  ToTensorVideo -> [RandomHorizontalFlipVideo] -> UCFCenterCropVideo | CenterCropResizeVideo ->
// Normalize(0.5, 0.5)  as ONE launch: gathered uint8 NHWC frames [N, Hs, Ws, 3] -> fp32 NCHW [N, 3, out_h, out_w] in [-1, 1], the
// in_mode 0 input of latte_vae_encode.
//
// Every output pixel is  ((blend of four taps of x / 255) - 0.5) / 0.5  in torch's order of operations (UpSampleKernel.cpp: the row
// blends first, then the two rows), with torch's source coordinate  scale * (dst + 0.5) - 0.5  clamped below at 0, the lower tap
// clamped at the last row / column and the weight clamped to [0, 1].  The whole file is compiled without multiply-add contraction:
// a fused coordinate differs from torch's by one ulp, and one ulp at a coordinate near 300 is 3e-5 in the blend weight.
#include "common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace latte {

namespace {

// torch's area_pixel_compute_source_index (align_corners = False, not cubic)
__device__ __forceinline__ float vt_src_coord(float scale, int dst) {
  const float s = scale * ((float)dst + 0.5f) - 0.5f;
  return s < 0.f ? 0.f : s;
}

// lower tap, upper tap and the upper tap's weight along one axis of `size` source elements
__device__ __forceinline__ void vt_taps(float scale, int dst, int size, int& a, int& b, float& lam) {
  const float r = vt_src_coord(scale, dst);
  a = min((int)r, size - 1);
  lam = fminf(fmaxf(r - (float)a, 0.f), 1.f);
  b = a + (a < size - 1 ? 1 : 0);
}

// One thread: four horizontally adjacent outputs of one row, all three channels.  Neighbouring threads write neighbouring 16-byte
// pieces of each plane (1 KiB per wave and plane); the uint8 taps of a wave come from two source rows and stay in the caches.
__global__ __launch_bounds__(256) void video_transform_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ flip,
                                                              float* __restrict__ out, int n, latte_video_plan p, int vec) {
  const int qw = (p.out_w + 3) >> 2;
  const long total = (long)n * p.out_h * qw;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int xq = (int)(t % qw);
  const long r = t / qw;
  const int oy = (int)(r % p.out_h);
  const int f = (int)(r / p.out_h);

  int ya, yb;
  float ly;
  vt_taps(p.scale_h, oy + p.crop_i, p.reg_h, ya, yb, ly);
  const float wy0 = 1.f - ly;
  const uint8_t* frame = src + (size_t)f * p.src_h * p.src_w * 3;
  const uint8_t* rowa = frame + (size_t)(p.reg_y + ya) * p.src_w * 3;
  const uint8_t* rowb = frame + (size_t)(p.reg_y + yb) * p.src_w * 3;
  const bool mirrored = flip != nullptr && flip[f] != 0;

  float v[3][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ox = min(xq * 4 + i, p.out_w - 1);   // past the row's end: computed again, not stored
    int xa, xb;
    float lx;
    vt_taps(p.scale_w, ox + p.crop_j, p.reg_w, xa, xb, lx);
    const float wx0 = 1.f - lx;
    int ca = p.reg_x + xa, cb = p.reg_x + xb;      // columns of the (flipped) frame -> columns of the stored one
    if (mirrored) { ca = p.src_w - 1 - ca; cb = p.src_w - 1 - cb; }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float s00 = (float)rowa[ca * 3 + c] / 255.f, s01 = (float)rowa[cb * 3 + c] / 255.f;
      const float s10 = (float)rowb[ca * 3 + c] / 255.f, s11 = (float)rowb[cb * 3 + c] / 255.f;
      const float top = s00 * wx0 + s01 * lx;
      const float bot = s10 * wx0 + s11 * lx;
      v[c][i] = ((top * wy0 + bot * ly) - 0.5f) / 0.5f;
    }
  }
  const size_t plane = (size_t)p.out_h * p.out_w;
  float* o = out + (size_t)f * 3 * plane + (size_t)oy * p.out_w + (size_t)xq * 4;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (vec) {
      *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (xq * 4 + i < p.out_w) o[c * plane + i] = v[c][i];
    }
  }
}

// Python's round() of d / 2.0 for an integer d >= 0: halves go to the even neighbour
int round_half_even_half(int d) {
  const int k = d / 2;
  return (d & 1) ? k + (k & 1) : k;
}

}  // namespace

}  // namespace latte

using namespace latte;

extern "C" {

int latte_video_transform_plan(int kind, int src_h, int src_w, int out_h, int out_w, latte_video_plan* plan) {
  if (!plan) return fail(LATTE_ERR_INVALID, "video_transform_plan: null plan");
  if (src_h < 1 || src_w < 1) return fail(LATTE_ERR_INVALID, "video_transform_plan: source frames must be at least 1 x 1");
  latte_video_plan p = {};
  p.kind = kind; p.src_h = src_h; p.src_w = src_w;
  if (kind == LATTE_VT_NONE) {
    if ((out_h && out_h != src_h) || (out_w && out_w != src_w))
      return fail(LATTE_ERR_INVALID, "video_transform_plan: LATTE_VT_NONE keeps the frame size (pass out_h = out_w = 0 or the source size)");
    p.out_h = p.mid_h = p.reg_h = src_h;
    p.out_w = p.mid_w = p.reg_w = src_w;
    p.scale_h = p.scale_w = 1.f;
  } else if (kind == LATTE_VT_UCF_CENTER_CROP) {
    if (out_h < 1 || out_w < 1) return fail(LATTE_ERR_INVALID, "video_transform_plan: output size must be at least 1 x 1");
    // resize_scale (video_transforms.py:52-57): the scale factor in double, torch's floor(float(dim) * scale) intermediate size and
    // the GIVEN scale's reciprocal, cast to float, as the coordinate scale of both axes
    const double scale = (double)out_h / (double)(src_h < src_w ? src_h : src_w);
    p.mid_h = (int)std::floor((double)src_h * scale);
    p.mid_w = (int)std::floor((double)src_w * scale);
    // center_crop (:80-90) raises this; so does the Python layer (ValueError) on this message
    if (p.mid_h < out_h || p.mid_w < out_w) return fail(LATTE_ERR_INVALID, "height and width must be no smaller than crop_size");
    p.crop_i = round_half_even_half(p.mid_h - out_h);
    p.crop_j = round_half_even_half(p.mid_w - out_w);
    p.scale_h = p.scale_w = (float)(1.0 / scale);
    p.reg_h = src_h; p.reg_w = src_w;
    p.out_h = out_h; p.out_w = out_w;
  } else if (kind == LATTE_VT_CENTER_CROP_RESIZE) {
    if (out_h < 1 || out_w < 1) return fail(LATTE_ERR_INVALID, "video_transform_plan: output size must be at least 1 x 1");
    // center_crop_using_short_edge (:93-105), then resize to the size (:47-50): no scale factor, so torch uses in / out in float
    if (src_h < src_w) { p.reg_h = p.reg_w = src_h; p.reg_x = round_half_even_half(src_w - src_h); }
    else { p.reg_h = p.reg_w = src_w; p.reg_y = round_half_even_half(src_h - src_w); }
    p.scale_h = (float)p.reg_h / (float)out_h;
    p.scale_w = (float)p.reg_w / (float)out_w;
    p.mid_h = p.out_h = out_h; p.mid_w = p.out_w = out_w;
  } else {
    return fail(LATTE_ERR_INVALID, "video_transform_plan: kind must be LATTE_VT_NONE, LATTE_VT_UCF_CENTER_CROP or LATTE_VT_CENTER_CROP_RESIZE");
  }
  *plan = p;
  return LATTE_OK;
}

int latte_video_transform(const uint8_t* src, int n, int src_h, int src_w, int kind, int out_h, int out_w, const uint8_t* flip, float* out,
                          void* stream) {
  if (!src || !out) return fail(LATTE_ERR_INVALID, "video_transform: null argument");
  if (n < 1) return fail(LATTE_ERR_INVALID, "video_transform: needs at least one frame");
  latte_video_plan p;
  if (int rc = latte_video_transform_plan(kind, src_h, src_w, out_h, out_w, &p)) return rc;
  // what the kernel indexes: taps inside the region, the region inside the frame, 32-bit tap offsets within a frame
  if (p.reg_y < 0 || p.reg_x < 0 || p.reg_y + p.reg_h > src_h || p.reg_x + p.reg_w > src_w || p.crop_i < 0 || p.crop_j < 0)
    return fail(LATTE_ERR_INVALID, "video_transform: internal plan out of range");
  if ((int64_t)src_h * src_w * 3 > INT32_MAX) return fail(LATTE_ERR_INVALID, "video_transform: a source frame must stay below 2^31 bytes");
  const int64_t threads = (int64_t)n * p.out_h * ((p.out_w + 3) / 4);
  const int64_t blocks = (threads + 255) / 256;
  if (blocks > INT32_MAX) return fail(LATTE_ERR_INVALID, "video_transform: too many output pixels for one launch");
  const int vec = (p.out_w % 4 == 0) && ((uintptr_t)out % 16 == 0);
  hipLaunchKernelGGL(video_transform_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, flip, out, n, p, vec);
  LATTE_HIP(hipGetLastError());
  return LATTE_OK;
}

}  // extern "C"
