// Host logic of the SD-VAE decoder and encoder: weight ingestion by diffusers state-dict key, workspace, decode(), encode().
//
//   AutoencoderKL.decode(z).sample      diffusers 0.24.0 (un-vendored; oracle/vae_oracle.py restates it)
//   called by the reference at          /root/reference/sample/sample.py:113-115, sample_ddp.py:165-168
//   uint8 video conversion              /root/reference/sample/sample.py:122
//
// Activation layout: NHWC.  The decoder's RESIDUAL STREAM (conv_in output, every ResnetBlock2D / attention / upsampler
// output) is fp32 -- two ping-pong buffers -- so the skip path is never rounded: with a half stream each of the ~20
// block outputs added one half rounding of the whole activation and the f16 decode ended at 1.35e-3 rel-L2 against the
// fp32 restatement (round 1).  conv1's output inside a ResnetBlock2D is fp32 as well (it only feeds GroupNorm 2).  Only
// the MFMA operands (GroupNorm+SiLU outputs, attention q/k/v/P, the half copies the shortcut / upsampler convs read) are
// half: three half scratch buffers, all sized for the largest map ([N, 8h, 8w, 256]).
#include <cmath>
#include <string>
#include <vector>

#include "event_profile.h"
#include "weight_store.h"

using namespace latte;

namespace {
thread_local EventProfile* g_kprof = nullptr;   // armed by profile_vae_call on its thread
}  // namespace

namespace latte {
void kprof_mark(int cls, hipStream_t st) {
  if (g_kprof) g_kprof->mark(cls, st);
}
}  // namespace latte

namespace {

// The body of latte_vae_profile_decode / _encode: `call` (the decode / encode) with a HIP event behind every launch, then the per-class sums
template <class Call>
int profile_vae_call(const std::string& name, float* ms_out, int* launches_out, int n, hipStream_t st, Call call) {
  if (!ms_out || !launches_out || n < VC_NUM_CLASSES) return fail(LATTE_ERR_INVALID, name + ": bad arguments");
  EventProfile prof;
  g_kprof = &prof;
  kprof_mark(VC_START, st);
  int rc = call();
  g_kprof = nullptr;
  if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(LATTE_ERR_HIP, name + ": device error");
  return prof.collect(name, ms_out, launches_out, n, rc);
}

// WeightSlot::kind; rows / cols of a slot are cout / cin; dst_lo (VP_CONV3 / VP_LINEAR_H16): the f16 rounding residual of the packed
// weight (split-operand passes), or nullptr
enum VPack { VP_F32, VP_CONV3, VP_LINEAR_H16, VP_SMALL_T, VP_SMALL, VP_CONVT };
struct Resnet {
  int cin, cout;
  float *n1w, *n1b, *n2w, *n2b, *c1b, *c2b, *scb = nullptr;
  half_t *c1w, *c2w, *scw = nullptr;
  half_t *c1w_lo = nullptr, *c2w_lo = nullptr, *scw_lo = nullptr;   // f16 rounding residuals of the weights (temporal decoder's split passes)
};
// TemporalResnetBlock + AlphaBlender of a SpatioTemporalResBlock (AutoencoderKLTemporalDecoder): Conv3d (3,1,1) weights as
// [C][3 C] half; conv2 and its bias are kept in fp32 too and folded with sigmoid(mix_factor) before the first decode
struct TResnet {
  int c = 0;
  float *n1w, *n1b, *n2w, *n2b, *c1b, *c2b, *c2b_eff, *c2w_f32, *mix;
  half_t *c1w, *c2w, *c1w_lo, *c2w_lo;   // _lo: the f16 rounding residual of the weights (split-operand convolution)
};

}  // namespace

struct latte_vae {
  int h = 0, max_frames = 0, dtype = 0;
  int ch[4] = {128, 256, 512, 512};   // block_out_channels
  WeightSlots weights;
  DeviceArena arena;
  float *pq_w, *pq_b, *ci_wt, *ci_b, *co_w, *co_b, *no_w, *no_b;
  Resnet mid[2];
  Resnet up[4][3];
  half_t* upc_w[3];
  half_t* upc_w_lo[3] = {nullptr, nullptr, nullptr};   // temporal decoder: f16 rounding residual of the upsampler weights
  float* upc_b[3];
  float *agn_w, *agn_b, *aq_b, *ak_b, *av_b, *ao_b, *ao_b_eff, *zero_bias;
  float* ao_w_f32;     // to_out weight in fp32 (for the folded bias  Wo bv + bo)
  half_t *aq_w, *ak_w, *av_w, *ao_w;
  half_t* buf[3];      // half scratch (MFMA operands)
  float* sbuf[2];      // fp32 residual stream, ping-pong
  float* tbuf;         // fp32 conv1 output of a ResnetBlock2D (GroupNorm 2 normalises it before anything rounds it)
  float* ones;         // [512] gate vector of ones (attention out-projection through the gated fp32 residual epilogue)
  half_t* zeros;
  float *pq_out, *scores, *gn_partial, *gn_stats;
  bool bias_folded = false;
  // AutoencoderKLTemporalDecoder mode (latte_vae_create_temporal): every resnet is a SpatioTemporalResBlock, no
  // post_quant_conv, time_conv_out after conv_out; one decode call = ONE video chunk of n_frames frames
  bool temporal = false;
  TResnet tmid[2], tup[4][3];
  float *tco_w = nullptr, *tco_b = nullptr;
  // SD-VAE ENCODER mode (latte_vae_create_encoder): h is the latent size, img = 8 h the image size; encoder.* / quant_conv.* slots only
  bool encoder = false;
  int img = 0;
  Resnet down[4][2];
  half_t *dnc_w[3] = {nullptr, nullptr, nullptr}, *dnc_w_lo[3] = {nullptr, nullptr, nullptr};   // Downsample2D conv weights (+ f16 residual)
  float* dnc_b[3] = {nullptr, nullptr, nullptr};
  float *eco_raw = nullptr, *eco_rb = nullptr, *eq_w = nullptr, *eq_b = nullptr;   // conv_out [8][9 * 512] packed, its bias, quant_conv 8 x 8 + 8
  float *eco_w = nullptr, *eco_b = nullptr;   // conv_out with quant_conv folded in (fp32, at the first encode after a load)
  float* moments = nullptr;                   // [max_frames, 8, h, w] when the caller asked for mode / sample
};

namespace {

int make_resnet(latte_vae* v, Resnet& r, const std::string& p, int cin, int cout) {
  r.cin = cin; r.cout = cout;
  int rc;
  if ((rc = v->arena.alloc(&r.n1w, cin)) || (rc = v->arena.alloc(&r.n1b, cin)) || (rc = v->arena.alloc(&r.n2w, cout)) ||
      (rc = v->arena.alloc(&r.n2b, cout)) || (rc = v->arena.alloc(&r.c1b, cout)) || (rc = v->arena.alloc(&r.c2b, cout)) ||
      (rc = v->arena.alloc(&r.c1w, (size_t)cout * cin * 9)) || (rc = v->arena.alloc(&r.c2w, (size_t)cout * cout * 9)))
    return rc;
  v->weights.add(p + "norm1.weight", cin, VP_F32, r.n1w);
  v->weights.add(p + "norm1.bias", cin, VP_F32, r.n1b);
  v->weights.add(p + "conv1.weight", (int64_t)cout * cin * 9, VP_CONV3, r.c1w, cout, cin);
  if ((rc = v->arena.alloc(&r.c1w_lo, (size_t)cout * cin * 9)) || (rc = v->arena.alloc(&r.c2w_lo, (size_t)cout * cout * 9))) return rc;
  v->weights.back().dst_lo = r.c1w_lo;
  v->weights.add(p + "conv1.bias", cout, VP_F32, r.c1b);
  v->weights.add(p + "norm2.weight", cout, VP_F32, r.n2w);
  v->weights.add(p + "norm2.bias", cout, VP_F32, r.n2b);
  v->weights.add(p + "conv2.weight", (int64_t)cout * cout * 9, VP_CONV3, r.c2w, cout, cout);
  v->weights.back().dst_lo = r.c2w_lo;
  v->weights.add(p + "conv2.bias", cout, VP_F32, r.c2b);
  if (cin != cout) {
    if ((rc = v->arena.alloc(&r.scw, (size_t)cout * cin)) || (rc = v->arena.alloc(&r.scb, cout))) return rc;
    v->weights.add(p + "conv_shortcut.weight", (int64_t)cout * cin, VP_LINEAR_H16, r.scw);
    if ((rc = v->arena.alloc(&r.scw_lo, (size_t)cout * cin))) return rc;
    v->weights.back().dst_lo = r.scw_lo;
    v->weights.add(p + "conv_shortcut.bias", cout, VP_F32, r.scb);
  }
  return LATTE_OK;
}

int make_tresnet(latte_vae* v, TResnet& t, const std::string& p, int c) {
  t.c = c;
  int rc;
  if ((rc = v->arena.alloc(&t.n1w, c)) || (rc = v->arena.alloc(&t.n1b, c)) || (rc = v->arena.alloc(&t.n2w, c)) || (rc = v->arena.alloc(&t.n2b, c)) ||
      (rc = v->arena.alloc(&t.c1b, c)) || (rc = v->arena.alloc(&t.c2b, c)) || (rc = v->arena.alloc(&t.c2b_eff, c)) ||
      (rc = v->arena.alloc(&t.c2w_f32, (size_t)c * c * 3)) || (rc = v->arena.alloc(&t.mix, 4)) || (rc = v->arena.alloc(&t.c1w, (size_t)c * c * 3)) ||
      (rc = v->arena.alloc(&t.c2w, (size_t)c * c * 3)) || (rc = v->arena.alloc(&t.c1w_lo, (size_t)c * c * 3)) ||
      (rc = v->arena.alloc(&t.c2w_lo, (size_t)c * c * 3)))
    return rc;
  const std::string q = p + "temporal_res_block.";
  v->weights.add(q + "norm1.weight", c, VP_F32, t.n1w);
  v->weights.add(q + "norm1.bias", c, VP_F32, t.n1b);
  v->weights.add(q + "conv1.weight", (int64_t)c * c * 3, VP_CONVT, &t, c, c);
  v->weights.add(q + "conv1.bias", c, VP_F32, t.c1b);
  v->weights.add(q + "norm2.weight", c, VP_F32, t.n2w);
  v->weights.add(q + "norm2.bias", c, VP_F32, t.n2b);
  v->weights.add(q + "conv2.weight", (int64_t)c * c * 3, VP_F32, t.c2w_f32);
  v->weights.add(q + "conv2.bias", c, VP_F32, t.c2b);
  v->weights.add(p + "time_mixer.mix_factor", 1, VP_F32, t.mix);
  return LATTE_OK;
}

// Which convolutions of the temporal decoder run as split-operand products (round 6).  Bits 0..4: the spatial resnets of {mid block, up block
// 0..3} add the pass on the activation's f16 rounding residual; bits 5..9: the temporal resnets of the same stages run hi*hi + lo*hi + hi*lo
// instead of one pass; bit 10: the 1x1 shortcuts' half copy of the stream as hi + lo (a second GEMM pass); bit 11: conv_out reads its input as
// hi + lo; bits 12..14: the upsampler convolution of up block 0..2 adds the pass on the residual of its half copy of the stream; bits 15..19: the
// spatial resnets of the five stages add the pass on the WEIGHTS' f16 rounding residual; bit 20: the shortcuts' weight residual; bits 21..23: the
// upsamplers' weight residual.
// latte_debug_set_choice("vae_split", (1 << 24) | mask) overrides the default (measurement / parity sweeps).
// The encoder uses the same bit layout with its own stages (resnets: bit 0 = mid block, 1 + i = down block i; bits 12..14 / 21..23 = the
// down-sampler of down block i; bit 11 = conv_out).
// vae_decode_impl / vae_encode_impl read the mask ONCE, at their top, and pass it down by value: a call runs entirely on the mask it started
// with, whatever a concurrent latte_debug_set_choice does meanwhile.
constexpr int VAE_SPLIT_DEFAULT_TEMPORAL = 0x319c03, VAE_SPLIT_DEFAULT_SPATIAL = 0x301c00;
constexpr int VAE_SPLIT_DEFAULT_ENCODER = 0xf07c00;   // 1.01e-3 -> 7.7e-4 worst of five draws for +0.8 ms
struct SplitMask {   // stage: 0 = mid block, 1 + i = up / down block i; i: up- / down-sampler of block i
  int m;
  bool act(int stage) const { return (m >> stage) & 1; }
  bool temporal(int stage) const { return (m >> (5 + stage)) & 1; }
  bool shortcut() const { return (m >> 10) & 1; }
  bool conv_out() const { return (m >> 11) & 1; }
  bool resample(int i) const { return (m >> (12 + i)) & 1; }
  bool weight(int stage) const { return (m >> (15 + stage)) & 1; }
  bool shortcut_weight() const { return (m >> 20) & 1; }
  bool resample_weight(int i) const { return (m >> (21 + i)) & 1; }
};
SplitMask vae_split_mask(int dflt) {
  const int c = debug_choice(DBG_VAE_SPLIT);
  return SplitMask{(c >> 24) == 1 ? (c & 0xffffff) : dflt};
}

int gemm_h16(const half_t* A, const half_t* W, const float* bias, void* out, const half_t* res, int M, int N, int K, int epi,
             int dtype, hipStream_t st) {
  GemmArgs g{};
  g.A = A; g.W = W; g.bias = bias; g.out = out; g.res = res; g.M = M; g.N = N; g.K = K; g.rows_per_sample = M;
  // plain 128 x 128 kernel: small, oddly shaped problems (round 6: the library's own tile choice for the 1x1 shortcuts of the large maps
  // measured the same decode time, profiles/r6_vae_split_sweep.log)
  const int rc_ = launch_gemm(g, epi, dtype, 1, st);
  kprof_mark(VC_ATTN, st);                              // (only the mid-block attention and the 1x1 shortcuts come through here)
  return rc_;
}

// Split-operand 3x3 convolution into the fp32 map `out`: out = conv(hi, w) + bias (+ res), then -- accumulating into out -- conv(lo, w) when
// lo, the f16 rounding residual of the activation, is given, and conv(hi, w_lo) when w_lo, the residual of the weight, is.
// up / rows / down: launch_conv3x3's nearest-x2 gather, 3-tap (Conv3d (3,1,1)) and stride-2 forms
int split_conv(const latte_vae* v, const half_t* hi, const half_t* lo, const half_t* w, const half_t* w_lo, const float* bias, int N, int H, int W,
               int cin, int cout, int up, const float* res, float* out, int rows, int down, hipStream_t st) {
  int rc;
  if ((rc = launch_conv3x3(hi, w, bias, nullptr, nullptr, v->zeros, N, H, W, cin, cout, up, v->dtype, st, res, out, rows, down))) return rc;
  if (lo && (rc = launch_conv3x3(lo, w, v->zero_bias, nullptr, nullptr, v->zeros, N, H, W, cin, cout, up, v->dtype, st, out, out, rows, down))) return rc;
  if (w_lo) return launch_conv3x3(hi, w_lo, v->zero_bias, nullptr, nullptr, v->zeros, N, H, W, cin, cout, up, v->dtype, st, out, out, rows, down);
  return LATTE_OK;
}

// ResnetBlock2D on the fp32 stream: x = *s -> *s (in place when cin == cout, else through *s2 and the two are swapped);
// b, c, d: half scratch.  [N, H, W, C]
int run_resnet(latte_vae* v, const Resnet& r, float** s, float** s2, half_t* b, half_t* c, half_t* d, int N, int H, int W,
               hipStream_t st, int stage, SplitMask mask) {
  int rc;
  const int HW = H * W, dt = v->dtype;
  float* x = *s;
  // temporal-decoder mode: the activation operand of both 3x3 convolutions is split hi + lo (b = the f16 rounding residual of the
  // GroupNorm output) and a second pass adds conv(lo): the decoder with twice as many blocks per stage stays under the 1e-3 bar
  // (round 6: per decoder stage -- SplitMask::act(stage), 0 = mid block, 1 + i = up block i)
  half_t* lo = mask.act(stage) ? b : nullptr;
  const bool wlo = mask.weight(stage);   // + the pass hi * (weight residual)
  if (r.cin != r.cout) {   // conv_shortcut 1x1 = a GEMM over pixels on a half copy of the stream, fp32 result (first: b is free here)
    float* y = *s2;
    if (mask.shortcut()) {   // the half copy as hi + lo: y = hi W^T + b, then y += lo W^T (gated-residual epilogue, gate = 1)
      if ((rc = launch_convert_f32_to_h16_split(x, d, b, (int64_t)N * HW * r.cin, dt, st))) return rc;
      kprof_mark(VC_SMALL, st);
      if ((rc = gemm_h16(d, r.scw, r.scb, y, nullptr, N * HW, r.cout, r.cin, EPI_BIAS_F32, dt, st))) return rc;
      GemmArgs g{};
      g.A = b; g.W = r.scw; g.bias = v->zero_bias; g.out = y; g.gate = v->ones; g.gate_stride = 0;
      g.M = N * HW; g.N = r.cout; g.K = r.cin; g.rows_per_sample = N * HW;
      const int sc_variant = 1;
      if ((rc = launch_gemm(g, EPI_GATE_RES_F32, dt, sc_variant, st))) return rc;
      kprof_mark(VC_ATTN, st);
      if (r.scw_lo && mask.shortcut_weight()) {   // + hi * (weight residual)
        g.A = d; g.W = r.scw_lo;
        if ((rc = launch_gemm(g, EPI_GATE_RES_F32, dt, sc_variant, st))) return rc;
        kprof_mark(VC_ATTN, st);
      }
    } else {
      if ((rc = launch_convert_f32_to_h16(x, d, (int64_t)N * HW * r.cin, dt, st))) return rc;
      kprof_mark(VC_SMALL, st);
      if ((rc = gemm_h16(d, r.scw, r.scb, y, nullptr, N * HW, r.cout, r.cin, EPI_BIAS_F32, dt, st))) return rc;
    }
  }
  if ((rc = launch_groupnorm(x, 1, c, r.n1w, r.n1b, v->gn_partial, v->gn_stats, N, HW, r.cin, 1, dt, st, 1e-6f, groupnorm_max_slabs(), lo))) return rc;
  if ((rc = split_conv(v, c, lo, r.c1w, wlo ? r.c1w_lo : nullptr, r.c1b, N, H, W, r.cin, r.cout, 0, nullptr, v->tbuf, 0, 0, st))) return rc;
  if ((rc = launch_groupnorm(v->tbuf, 1, c, r.n2w, r.n2b, v->gn_partial, v->gn_stats, N, HW, r.cout, 1, dt, st, 1e-6f, groupnorm_max_slabs(), lo))) return rc;
  float* y = r.cin != r.cout ? *s2 : x;   // conv2 adds onto the shortcut's result, or onto the stream in place
  if ((rc = split_conv(v, c, lo, r.c2w, wlo ? r.c2w_lo : nullptr, r.c2b, N, H, W, r.cout, r.cout, 0, y, y, 0, 0, st))) return rc;
  if (r.cin != r.cout) std::swap(*s, *s2);
  return LATTE_OK;
}

// TemporalResnetBlock + AlphaBlender on the fp32 stream of ONE video [T, H, W, C]: the frames are the rows of an "image"
// [T][H W], so the Conv3d (3,1,1) is the implicit-GEMM conv kernel with 3 taps along the rows and GroupNorm sees T H W pixels
int run_tresnet(latte_vae* v, const TResnet& t, float* x, half_t* c, half_t* clo, int T, int H, int W, hipStream_t st, int stage, SplitMask mask) {
  // The two Conv3d run as SPLIT-OPERAND convolutions: activation = hi + lo and weight = hi + lo in f16 (lo = the rounding
  // residual), three MFMA passes hi*hi + lo*hi + hi*lo accumulated in the fp32 output -- the temporal branch then adds ~1e-6 of
  // error instead of one more f16 roundoff per block (with single-pass convolutions the decode measured 1.04e-3 against the
  // fp32 restatement, above the 1e-3 bar; a 3-tap convolution costs a third of a 3x3 one, so three passes cost one)
  int rc;
  const int HW = H * W, dt = v->dtype, C = t.c;
  const bool split = mask.temporal(stage);   // clear: single-pass temporal convolutions at this stage
  if (!split) clo = nullptr;
  if ((rc = launch_groupnorm(x, 1, c, t.n1w, t.n1b, v->gn_partial, v->gn_stats, 1, T * HW, C, 1, dt, st, 1e-5f, groupnorm_max_slabs() * T, clo))) return rc;
  if ((rc = split_conv(v, c, clo, t.c1w, split ? t.c1w_lo : nullptr, t.c1b, 1, T, HW, C, C, 0, nullptr, v->tbuf, 1, 0, st))) return rc;
  if ((rc = launch_groupnorm(v->tbuf, 1, c, t.n2w, t.n2b, v->gn_partial, v->gn_stats, 1, T * HW, C, 1, dt, st, 1e-5f, groupnorm_max_slabs() * T, clo))) return rc;
  // out = x_spatial + sigmoid(mix) * (conv2 + bias): weights and bias were folded with the blend factor
  return split_conv(v, c, clo, t.c2w, split ? t.c2w_lo : nullptr, t.c2b_eff, 1, T, HW, C, C, 0, x, x, 1, 0, st);
}

// softmax rows sum to 1, so  to_out(P (V0 + 1 bv^T)) = to_out(P V0) + (Wo bv + bo): the value bias is folded into the output bias
// (once after a weight load) and V^T is produced directly by a GEMM (no transpose kernel)
int fold_attention_bias(latte_vae* v, hipStream_t st) {
  const int top = v->ch[3];
  return launch_small_linear(IN_PLAIN, v->av_b, nullptr, v->ao_w_f32, v->ao_b, nullptr, nullptr, v->ao_b_eff, 1, top, top, top, st);
}

// The stage-trace test hooks (latte_debug_vae_trace / _encode_trace): the stages of a call are numbered as they come and stage `stop_after`
// ends it with a copy of that activation (fp32, dims d0..d3) in `out`; who: the hook's error prefix
struct StageTrace {
  int stop_after; float* out; int64_t* numel; int* dims; const char* who;
  int stage_no = 0;
  bool hit(const float* src, int d0, int d1, int d2, int d3, hipStream_t st, int& rc) {
    if (stage_no++ != stop_after) return false;
    const int64_t n = (int64_t)d0 * d1 * d2 * d3;
    rc = LATTE_OK;
    if (hipMemcpyAsync(out, src, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, st) != hipSuccess)
      rc = fail(LATTE_ERR_HIP, std::string(who) + ": copy failed");
    *numel = n;
    dims[0] = d0; dims[1] = d1; dims[2] = d2; dims[3] = d3;
    return true;
  }
};

int vae_create_impl(int latent_size, int max_frames, int compute_dtype, bool temporal, latte_vae_t** out);
int vae_create_encoder_impl(int image_size, int max_frames, int compute_dtype, latte_vae_t** out);

}  // namespace

extern "C" {

int latte_vae_create(int latent_size, int max_frames, int compute_dtype, latte_vae_t** out) {
  return vae_create_impl(latent_size, max_frames, compute_dtype, false, out);
}
int latte_vae_create_temporal(int latent_size, int max_frames, int compute_dtype, latte_vae_t** out) {
  return vae_create_impl(latent_size, max_frames, compute_dtype, true, out);
}
int latte_vae_create_encoder(int image_size, int max_frames, int compute_dtype, latte_vae_t** out) {
  return vae_create_encoder_impl(image_size, max_frames, compute_dtype, out);
}

}  // extern "C"

namespace {
// UNetMidBlock2D's attention: weights and scratch under prefix a ("decoder.mid_block.attentions.0." / "encoder.mid_block.attentions.0.")
int make_mid_attention(latte_vae* v, const std::string& a) {
  const int top = v->ch[3];
  int rc;
#define ATRY(x) do { if ((rc = (x))) return rc; } while (0)
  ATRY(v->arena.alloc(&v->agn_w, top)); ATRY(v->arena.alloc(&v->agn_b, top));
  ATRY(v->arena.alloc(&v->aq_b, top)); ATRY(v->arena.alloc(&v->ak_b, top)); ATRY(v->arena.alloc(&v->av_b, top)); ATRY(v->arena.alloc(&v->ao_b, top));
  ATRY(v->arena.alloc(&v->ao_b_eff, top)); ATRY(v->arena.alloc(&v->zero_bias, 4096));
  ATRY(v->arena.alloc(&v->aq_w, (size_t)top * top)); ATRY(v->arena.alloc(&v->ak_w, (size_t)top * top));
  ATRY(v->arena.alloc(&v->av_w, (size_t)top * top)); ATRY(v->arena.alloc(&v->ao_w, (size_t)top * top));
  ATRY(v->arena.alloc(&v->ao_w_f32, (size_t)top * top));
  v->weights.add(a + "group_norm.weight", top, VP_F32, v->agn_w);
  v->weights.add(a + "group_norm.bias", top, VP_F32, v->agn_b);
  v->weights.add(a + "to_q.weight", (int64_t)top * top, VP_LINEAR_H16, v->aq_w);
  v->weights.add(a + "to_q.bias", top, VP_F32, v->aq_b);
  v->weights.add(a + "to_k.weight", (int64_t)top * top, VP_LINEAR_H16, v->ak_w);
  v->weights.add(a + "to_k.bias", top, VP_F32, v->ak_b);
  v->weights.add(a + "to_v.weight", (int64_t)top * top, VP_LINEAR_H16, v->av_w);
  v->weights.add(a + "to_v.bias", top, VP_F32, v->av_b);
  v->weights.add(a + "to_out.0.weight", (int64_t)top * top, VP_LINEAR_H16, v->ao_w);
  v->weights.add(a + "to_out.0.bias", top, VP_F32, v->ao_b);
#undef ATRY
  return LATTE_OK;
}

// UNetMidBlock2D's attention on the fp32 stream a [N, H, W, 512] (in place): 1 head, dim 512, tokens = H*W per frame; b, c, d: half scratch
int run_mid_attention(latte_vae* v, float* a, half_t* b, half_t* c, half_t* d, int N, int H, int W, hipStream_t st) {
  int rc;
  const int dt = v->dtype, top = v->ch[3];
  const int L = H * W;
  if (L % 128 != 0) return fail(LATTE_ERR_INVALID, "vae: H*W must be a multiple of 128 for the attention GEMMs");
  if ((rc = launch_groupnorm(a, 1, c, v->agn_w, v->agn_b, v->gn_partial, v->gn_stats, N, L, top, 0, dt, st))) return rc;
  if ((rc = gemm_h16(c, v->aq_w, v->aq_b, b, nullptr, N * L, top, top, EPI_BIAS_H16, dt, st))) return rc;   // q  [N L, 512]
  if ((rc = gemm_h16(c, v->ak_w, v->ak_b, d, nullptr, N * L, top, top, EPI_BIAS_H16, dt, st))) return rc;   // k  [N L, 512]
  half_t* vt = b + (size_t)N * L * top;   // V0^T per frame [512, L], behind q in buffer b
  half_t* pm = d + (size_t)N * L * top;   // P per frame [L, L], behind k in buffer d
  half_t* o = c + (size_t)N * L * top;    // attention output [N L, 512], behind the normed input in buffer c
  const float scale = 1.0f / std::sqrt((float)top);
  for (int f = 0; f < N; ++f) {
    const half_t* hf = c + (size_t)f * L * top;
    if ((rc = gemm_h16(v->av_w, hf, v->zero_bias, vt, nullptr, top, L, top, EPI_BIAS_H16, dt, st))) return rc;          // V0^T = Wv h^T
    if ((rc = gemm_h16(b + (size_t)f * L * top, d + (size_t)f * L * top, v->zero_bias, v->scores, nullptr, L, L, top,
                       EPI_BIAS_F32, dt, st))) return rc;                                                               // S = q k^T
    if ((rc = launch_softmax_rows(v->scores, pm, L, L, scale, dt, st))) return rc;
    if ((rc = gemm_h16(pm, vt, v->zero_bias, o + (size_t)f * L * top, nullptr, L, top, L, EPI_BIAS_H16, dt, st))) return rc;  // P V0
  }
  {  // to_out + residual straight into the fp32 stream: stream += 1 * (o Wo^T + b_eff)
    GemmArgs g{};
    g.A = o; g.W = v->ao_w; g.bias = v->ao_b_eff; g.out = a; g.gate = v->ones; g.gate_stride = 0;
    g.M = N * L; g.N = top; g.K = top; g.rows_per_sample = N * L;
    if ((rc = launch_gemm(g, EPI_GATE_RES_F32, dt, 1, st))) return rc;
    kprof_mark(VC_ATTN, st);
  }
  return LATTE_OK;
}

// The scratch both kinds of handle need, behind their weights: big = elements of the largest NHWC map, L = h * w of the latent (the
// attention's tokens); *per_latent = [max_frames, ch, h, w] fp32 (the decoder's post_quant_conv output / the encoder's moments)
int alloc_workspace(latte_vae* v, size_t big, size_t L, float** per_latent, int ch) {
  int rc;
  for (int i = 0; i < 3; ++i) if ((rc = v->arena.alloc(&v->buf[i], big))) return rc;
  for (int i = 0; i < 2; ++i) if ((rc = v->arena.alloc(&v->sbuf[i], big))) return rc;
  if ((rc = v->arena.alloc(&v->tbuf, big)) || (rc = v->arena.alloc(&v->ones, 512))) return rc;
  const std::vector<float> one(512, 1.0f);
  LATTE_HIP(hipMemcpy(v->ones, one.data(), sizeof(float) * 512, hipMemcpyHostToDevice));
  if ((rc = v->arena.alloc(&v->zeros, 64)) || (rc = v->arena.alloc(per_latent, (size_t)v->max_frames * ch * L)) ||
      (rc = v->arena.alloc(&v->scores, L * L)) || (rc = v->arena.alloc(&v->gn_partial, (size_t)v->max_frames * groupnorm_max_slabs() * 64)) ||
      (rc = v->arena.alloc(&v->gn_stats, (size_t)v->max_frames * 64)))
    return rc;
  return v->weights.alloc_stage(v->arena, true);
}

int vae_create_impl(int latent_size, int max_frames, int compute_dtype, bool temporal, latte_vae_t** out) {
  if (!out || latent_size <= 0 || max_frames <= 0) return fail(LATTE_ERR_INVALID, "vae_create: bad arguments");
  if (compute_dtype != LATTE_DTYPE_F16)
    return fail(LATTE_ERR_INVALID, "vae_create: the decoder runs f16 MFMA operands only (the reference decodes in fp16, sample.py:74; "
                                   "bf16 operands measured 7e-3 against the fp32 restatement and are not offered)");
  if (latent_size % 16 != 0 || latent_size > 64)
    return fail(LATTE_ERR_INVALID, "vae_create: latent_size must be a multiple of 16, at most 64");
  auto* v = new latte_vae();
  v->h = latent_size; v->max_frames = max_frames; v->dtype = compute_dtype; v->temporal = temporal;
  const int top = v->ch[3];
  const std::string sp = temporal ? "spatial_res_block." : "";
  int rc = LATTE_OK;
#define TRY(x) do { if ((rc = (x))) { latte_vae_destroy(v); return rc; } } while (0)
  TRY(v->arena.alloc(&v->pq_w, 16)); TRY(v->arena.alloc(&v->pq_b, 4));
  TRY(v->arena.alloc(&v->ci_wt, (size_t)36 * top)); TRY(v->arena.alloc(&v->ci_b, top));
  TRY(v->arena.alloc(&v->co_w, (size_t)27 * v->ch[0])); TRY(v->arena.alloc(&v->co_b, 4));
  TRY(v->arena.alloc(&v->no_w, v->ch[0])); TRY(v->arena.alloc(&v->no_b, v->ch[0]));
  if (!temporal) {
    v->weights.add("post_quant_conv.weight", 16, VP_F32, v->pq_w);
    v->weights.add("post_quant_conv.bias", 4, VP_F32, v->pq_b);
  } else {   // AutoencoderKLTemporalDecoder has no post_quant_conv: the 1x1 kernel runs with the identity
    const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    LATTE_HIP(hipMemcpy(v->pq_w, eye, sizeof(eye), hipMemcpyHostToDevice));
  }
  v->weights.add("decoder.conv_in.weight", (int64_t)top * 36, VP_SMALL_T, v->ci_wt, top, 4);
  v->weights.add("decoder.conv_in.bias", top, VP_F32, v->ci_b);
  TRY(make_resnet(v, v->mid[0], "decoder.mid_block.resnets.0." + sp, top, top));
  if (temporal) TRY(make_tresnet(v, v->tmid[0], "decoder.mid_block.resnets.0.", top));
  TRY(make_mid_attention(v, "decoder.mid_block.attentions.0."));
  TRY(make_resnet(v, v->mid[1], "decoder.mid_block.resnets.1." + sp, top, top));
  if (temporal) TRY(make_tresnet(v, v->tmid[1], "decoder.mid_block.resnets.1.", top));
  int prev = top;
  for (int i = 0; i < 4; ++i) {
    const int cout = v->ch[3 - i];
    for (int r = 0; r < 3; ++r) {
      const std::string rp = "decoder.up_blocks." + std::to_string(i) + ".resnets." + std::to_string(r) + ".";
      TRY(make_resnet(v, v->up[i][r], rp + sp, r == 0 ? prev : cout, cout));
      if (temporal) TRY(make_tresnet(v, v->tup[i][r], rp, cout));
    }
    prev = cout;
    if (i < 3) {
      TRY(v->arena.alloc(&v->upc_w[i], (size_t)cout * cout * 9));
      TRY(v->arena.alloc(&v->upc_b[i], cout));
      const std::string p = "decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv.";
      v->weights.add(p + "weight", (int64_t)cout * cout * 9, VP_CONV3, v->upc_w[i], cout, cout);
      TRY(v->arena.alloc(&v->upc_w_lo[i], (size_t)cout * cout * 9));
      v->weights.back().dst_lo = v->upc_w_lo[i];
      v->weights.add(p + "bias", cout, VP_F32, v->upc_b[i]);
    }
  }
  v->weights.add("decoder.conv_norm_out.weight", v->ch[0], VP_F32, v->no_w);
  v->weights.add("decoder.conv_norm_out.bias", v->ch[0], VP_F32, v->no_b);
  v->weights.add("decoder.conv_out.weight", (int64_t)27 * v->ch[0], VP_SMALL, v->co_w, 3, v->ch[0]);
  v->weights.add("decoder.conv_out.bias", 3, VP_F32, v->co_b);
  if (temporal) {
    TRY(v->arena.alloc(&v->tco_w, 27)); TRY(v->arena.alloc(&v->tco_b, 4));
    v->weights.add("decoder.time_conv_out.weight", 27, VP_F32, v->tco_w);      // [3, 3, 3, 1, 1] = (co, ci, tap)
    v->weights.add("decoder.time_conv_out.bias", 3, VP_F32, v->tco_b);
  }

  // workspace: the largest NHWC map is [N, 8h, 8w, 256] (output of up_blocks.2's upsampler)
  const size_t big = (size_t)max_frames * (8 * latent_size) * (8 * latent_size) * 256;
  TRY(alloc_workspace(v, big, (size_t)latent_size * latent_size, &v->pq_out, 4));
#undef TRY
  *out = v;
  return LATTE_OK;
}

// diffusers Encoder (down_block_types 4 x DownEncoderBlock2D, layers_per_block 2, double_z) + quant_conv of the sd-vae-ft architecture
int vae_create_encoder_impl(int image_size, int max_frames, int compute_dtype, latte_vae_t** out) {
  if (!out || image_size <= 0 || max_frames <= 0) return fail(LATTE_ERR_INVALID, "vae_create_encoder: bad arguments");
  if (compute_dtype != LATTE_DTYPE_F16)
    return fail(LATTE_ERR_INVALID, "vae_create_encoder: the encoder runs f16 MFMA operands only (as the decoder; bf16 operands are not offered)");
  if (image_size % 128 != 0 || image_size > 512)
    return fail(LATTE_ERR_INVALID, "vae_create_encoder: image_size must be a multiple of 128, at most 512 (the latent's h * w a multiple of 128 "
                                   "for the mid-block attention GEMMs)");
  auto* v = new latte_vae();
  v->encoder = true;
  v->img = image_size; v->h = image_size / 8; v->max_frames = max_frames; v->dtype = compute_dtype;
  const int top = v->ch[3];
  int rc = LATTE_OK;
#define TRY(x) do { if ((rc = (x))) { latte_vae_destroy(v); return rc; } } while (0)
  TRY(v->arena.alloc(&v->ci_wt, (size_t)27 * v->ch[0])); TRY(v->arena.alloc(&v->ci_b, v->ch[0]));
  v->weights.add("encoder.conv_in.weight", (int64_t)v->ch[0] * 27, VP_SMALL_T, v->ci_wt, v->ch[0], 3);
  v->weights.add("encoder.conv_in.bias", v->ch[0], VP_F32, v->ci_b);
  int prev = v->ch[0];
  for (int i = 0; i < 4; ++i) {
    const int cout = v->ch[i];
    for (int r = 0; r < 2; ++r)
      TRY(make_resnet(v, v->down[i][r], "encoder.down_blocks." + std::to_string(i) + ".resnets." + std::to_string(r) + ".", r == 0 ? prev : cout, cout));
    prev = cout;
    if (i < 3) {
      TRY(v->arena.alloc(&v->dnc_w[i], (size_t)cout * cout * 9)); TRY(v->arena.alloc(&v->dnc_w_lo[i], (size_t)cout * cout * 9));
      TRY(v->arena.alloc(&v->dnc_b[i], cout));
      const std::string p = "encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv.";
      v->weights.add(p + "weight", (int64_t)cout * cout * 9, VP_CONV3, v->dnc_w[i], cout, cout);
      v->weights.back().dst_lo = v->dnc_w_lo[i];
      v->weights.add(p + "bias", cout, VP_F32, v->dnc_b[i]);
    }
  }
  TRY(make_resnet(v, v->mid[0], "encoder.mid_block.resnets.0.", top, top));
  TRY(make_mid_attention(v, "encoder.mid_block.attentions.0."));
  TRY(make_resnet(v, v->mid[1], "encoder.mid_block.resnets.1.", top, top));
  TRY(v->arena.alloc(&v->no_w, top)); TRY(v->arena.alloc(&v->no_b, top));
  v->weights.add("encoder.conv_norm_out.weight", top, VP_F32, v->no_w);
  v->weights.add("encoder.conv_norm_out.bias", top, VP_F32, v->no_b);
  TRY(v->arena.alloc(&v->eco_raw, (size_t)8 * 9 * top)); TRY(v->arena.alloc(&v->eco_rb, 8));
  TRY(v->arena.alloc(&v->eq_w, 64)); TRY(v->arena.alloc(&v->eq_b, 8));
  TRY(v->arena.alloc(&v->eco_w, (size_t)8 * 9 * top)); TRY(v->arena.alloc(&v->eco_b, 8));
  v->weights.add("encoder.conv_out.weight", (int64_t)8 * 9 * top, VP_SMALL, v->eco_raw, 8, top);
  v->weights.add("encoder.conv_out.bias", 8, VP_F32, v->eco_rb);
  v->weights.add("quant_conv.weight", 64, VP_F32, v->eq_w);
  v->weights.add("quant_conv.bias", 8, VP_F32, v->eq_b);

  // workspace: the largest NHWC map is [N, H, W, 128] at the full image size (conv_in, down block 0)
  const size_t big = (size_t)max_frames * image_size * image_size * v->ch[0];
  TRY(alloc_workspace(v, big, (size_t)v->h * v->h, &v->moments, 8));
#undef TRY
  *out = v;
  return LATTE_OK;
}
}  // namespace

extern "C" {

void latte_vae_destroy(latte_vae_t* v) {
  delete v;   // the arena frees every device block
}

int latte_vae_num_keys(const latte_vae_t* v) { return v ? v->weights.size() : 0; }
const char* latte_vae_key(const latte_vae_t* v, int i) { return v ? v->weights.key(i) : nullptr; }

int latte_vae_load_tensor(latte_vae_t* v, const char* key, const float* data, int64_t numel, int on_device, void* stream) {
  if (!v || !key || !data) return fail(LATTE_ERR_INVALID, "vae_load_tensor: null argument");
  hipStream_t st = (hipStream_t)stream;
  WeightSlot* slot = nullptr;
  const float* src = nullptr;
  int rc = v->weights.begin_load("vae_load_tensor", key, data, numel, on_device, st, &slot, &src);
  if (rc) return rc;
  WeightSlot& s = *slot;
  switch (s.kind) {
    case VP_F32: LATTE_HIP(hipMemcpyAsync(s.dst, src, sizeof(float) * numel, hipMemcpyDeviceToDevice, st)); break;
    case VP_CONV3: rc = launch_pack_conv_w(src, (half_t*)s.dst, s.rows, s.cols, v->dtype, st, (half_t*)s.dst_lo); break;
    case VP_LINEAR_H16:
      rc = s.dst_lo ? launch_convert_f32_to_h16_split(src, (half_t*)s.dst, (half_t*)s.dst_lo, numel, v->dtype, st)
                    : launch_convert_f32_to_h16(src, (half_t*)s.dst, numel, v->dtype, st);
      break;
    case VP_SMALL_T: rc = launch_pack_small_w(src, (float*)s.dst, s.rows, s.cols, 1, st); break;
    case VP_SMALL: rc = launch_pack_small_w(src, (float*)s.dst, s.rows, s.cols, 0, st); break;
    case VP_CONVT: {
      TResnet* t = (TResnet*)s.dst;
      rc = launch_pack_conv_t(src, t->c1w, s.rows, s.cols, nullptr, v->dtype, st, t->c1w_lo);
      break;
    }
  }
  if (rc) return rc;
  if (s.key == "decoder.mid_block.attentions.0.to_out.0.weight" || s.key == "encoder.mid_block.attentions.0.to_out.0.weight")
    LATTE_HIP(hipMemcpyAsync(v->ao_w_f32, src, sizeof(float) * numel, hipMemcpyDeviceToDevice, st));
  if ((rc = v->weights.end_load(s, on_device, st))) return rc;
  v->bias_folded = false;
  return LATTE_OK;
}

int latte_vae_check_weights(latte_vae_t* v) {
  if (!v) return fail(LATTE_ERR_INVALID, "vae_check_weights: null");
  return v->weights.check_loaded();
}

static int vae_decode_impl(latte_vae_t* v, const float* z, int n_frames, float z_scale, int out_mode, void* out, void* stream,
                           int stop_after, float* trace_out, int64_t* trace_numel, int* trace_dims);

// One decode with a HIP event behind every launch: ms_out[c] / launches_out[c] per VaeKernelClass (conv3x3, GroupNorm statistics,
// GroupNorm apply, mid-block attention + 1x1 shortcut GEMMs, small kernels).  Synchronises the stream.
int latte_vae_profile_decode(latte_vae_t* v, const float* z, int n_frames, float z_scale, int out_mode, void* out, float* ms_out,
                             int* launches_out, int n, void* stream) {
  return profile_vae_call("vae_profile_decode", ms_out, launches_out, n, (hipStream_t)stream,
                          [&] { return vae_decode_impl(v, z, n_frames, z_scale, out_mode, out, stream, -1, nullptr, nullptr, nullptr); });
}

int latte_vae_decode(latte_vae_t* v, const float* z, int n_frames, float z_scale, int out_mode, void* out, void* stream) {
  return vae_decode_impl(v, z, n_frames, z_scale, out_mode, out, stream, -1, nullptr, nullptr, nullptr);
}

/* test hook (include/latte_amd_debug.h): run the decoder up to and including stage `stop_after` and return that stage's
 * NHWC activation as fp32. */
int latte_debug_vae_trace(latte_vae_t* v, const float* z, int n_frames, float z_scale, int stop_after, float* trace_out,
                          int64_t* trace_numel, int* trace_dims, void* stream) {
  if (!trace_out || !trace_numel || !trace_dims || stop_after < 0) return fail(LATTE_ERR_INVALID, "vae_trace: bad arguments");
  return vae_decode_impl(v, z, n_frames, z_scale, 0, trace_out, stream, stop_after, trace_out, trace_numel, trace_dims);
}

static int vae_decode_impl(latte_vae_t* v, const float* z, int n_frames, float z_scale, int out_mode, void* out, void* stream,
                           int stop_after, float* trace_out, int64_t* trace_numel, int* trace_dims) {
  if (!v || !z || !out) return fail(LATTE_ERR_INVALID, "vae_decode: null argument");
  if (v->encoder) return fail(LATTE_ERR_INVALID, "vae_decode: this handle is an encoder (latte_vae_create_encoder); decode needs a decoder handle");
  if (n_frames <= 0 || n_frames > v->max_frames) return fail(LATTE_ERR_STATE, "vae_decode: n_frames exceeds max_frames");
  if (out_mode != 0 && out_mode != 1) return fail(LATTE_ERR_INVALID, "vae_decode: out_mode must be 0 (fp32 NCHW) or 1 (uint8 NHWC)");
  int rc = latte_vae_check_weights(v);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int N = n_frames, dt = v->dtype, top = v->ch[3];
  int H = v->h, W = v->h;
  const SplitMask mask = vae_split_mask(v->temporal ? VAE_SPLIT_DEFAULT_TEMPORAL : VAE_SPLIT_DEFAULT_SPATIAL);
  if (!v->bias_folded) {
    if ((rc = fold_attention_bias(v, st))) return rc;
    if (v->temporal) {   // AlphaBlender folded into conv2 of every temporal resnet: out = x_spatial + sigmoid(mix) (conv2 + b)
      auto fold = [&](TResnet& t) -> int {
        int r2 = launch_pack_conv_t(t.c2w_f32, t.c2w, t.c, t.c, t.mix, dt, st, t.c2w_lo);
        return r2 ? r2 : launch_scale_by_sigmoid(t.c2b, t.c2b_eff, t.c, t.mix, st);
      };
      for (int k = 0; k < 2; ++k) if ((rc = fold(v->tmid[k]))) return rc;
      for (int i = 0; i < 4; ++i) for (int r = 0; r < 3; ++r) if ((rc = fold(v->tup[i][r]))) return rc;
    }
    v->bias_folded = true;
  }
  half_t *b = v->buf[0], *c = v->buf[1], *d = v->buf[2];
  float *a = v->sbuf[0], *a2 = v->sbuf[1];   // the fp32 residual stream and its ping-pong partner
  int cur_c = top;
  // stage numbering: 0 conv_in | 1 mid.resnet0 | 2 mid.attention | 3 mid.resnet1 | then per up block: 3 resnets (+ upsampler)
  StageTrace tr{stop_after, trace_out, trace_numel, trace_dims, "vae_trace"};
  auto traced = [&](int& rc_out) { return tr.hit(a, N, H, W, cur_c, st, rc_out); };
  if ((rc = launch_post_quant(z, v->pq_w, v->pq_b, v->pq_out, N, H * W, z_scale, st))) return rc;
  if ((rc = launch_conv_in(v->pq_out, v->ci_wt, v->ci_b, a, N, H, W, top, st))) return rc;
  if (traced(rc)) return rc;
  if ((rc = run_resnet(v, v->mid[0], &a, &a2, b, c, d, N, H, W, st, 0, mask))) return rc;
  if (v->temporal && (rc = run_tresnet(v, v->tmid[0], a, c, d, N, H, W, st, 0, mask))) return rc;
  if (traced(rc)) return rc;
  if ((rc = run_mid_attention(v, a, b, c, d, N, H, W, st))) return rc;
  if (traced(rc)) return rc;
  if ((rc = run_resnet(v, v->mid[1], &a, &a2, b, c, d, N, H, W, st, 0, mask))) return rc;
  if (v->temporal && (rc = run_tresnet(v, v->tmid[1], a, c, d, N, H, W, st, 0, mask))) return rc;
  if (traced(rc)) return rc;
  for (int i = 0; i < 4; ++i) {
    for (int r = 0; r < 3; ++r) {
      if ((rc = run_resnet(v, v->up[i][r], &a, &a2, b, c, d, N, H, W, st, 1 + i, mask))) return rc;
      if (v->temporal && (rc = run_tresnet(v, v->tup[i][r], a, c, d, N, H, W, st, 1 + i, mask))) return rc;
      cur_c = v->up[i][r].cout;
      if (traced(rc)) return rc;
    }
    if (i < 3) {  // Upsample2D: nearest x2 folded into the conv's gather (on a half copy of the stream), fp32 result
      const int cch = v->ch[3 - i];
      const bool ups_lo = mask.resample(i);   // the half copy as hi + lo, a second pass on lo
      if (ups_lo) rc = launch_convert_f32_to_h16_split(a, d, c, (int64_t)N * H * W * cch, dt, st);
      else rc = launch_convert_f32_to_h16(a, d, (int64_t)N * H * W * cch, dt, st);
      if (rc) return rc;
      kprof_mark(VC_SMALL, st);
      // (a null upc_w_lo[i] or a clear bit 21 + i: no pass on the weight residual)
      if ((rc = split_conv(v, d, ups_lo ? c : nullptr, v->upc_w[i], mask.resample_weight(i) ? v->upc_w_lo[i] : nullptr, v->upc_b[i], N, H, W, cch, cch,
                           1, nullptr, a2, 0, 0, st))) return rc;
      std::swap(a, a2);
      H *= 2;
      W *= 2;
      if (traced(rc)) return rc;
    }
  }
  if (stop_after >= 0) return fail(LATTE_ERR_INVALID, "vae_trace: stage index beyond the last traced stage");
  half_t* co_lo = mask.conv_out() ? b : nullptr;   // conv_out reads the GroupNorm output as hi + lo (its weights are fp32)
  if ((rc = launch_groupnorm(a, 1, c, v->no_w, v->no_b, v->gn_partial, v->gn_stats, N, H * W, v->ch[0], 1, dt, st, 1e-6f, groupnorm_max_slabs(), co_lo))) return rc;
  if (!v->temporal) return launch_conv_out(c, v->co_w, v->co_b, out, N, H, W, v->ch[0], out_mode, dt, st, co_lo);
  // conv_out to fp32 NCHW frames, then time_conv_out over the frames of the chunk
  if ((rc = launch_conv_out(c, v->co_w, v->co_b, v->tbuf, N, H, W, v->ch[0], 0, dt, st, co_lo))) return rc;
  return launch_time_conv_out(v->tbuf, v->tco_w, v->tco_b, out, N, H * W, out_mode, st);
}

// ------------------------------------------------------------------------------------------------ SD-VAE encoder
// AutoencoderKL.encode(x).latent_dist (diffusers 0.24.0; the reference's training step, train.py:204-211):
//   conv_in (3 -> 128) -> 4 x DownEncoderBlock2D (2 ResnetBlock2D each, Downsample2D = pad (0, 1, 0, 1) + 3x3 stride 2 on blocks 0..2)
//   -> UNetMidBlock2D (resnet, attention, resnet) -> GroupNorm + SiLU -> conv_out (512 -> 8) -> quant_conv (8 -> 8) = the moments.
// The same fp32 residual stream / half MFMA operand scheme as the decoder; the down-sampler is the implicit-GEMM conv's stride-2 gather
// (launch_conv3x3 down = 1) on a half copy of the stream.
static int vae_encode_impl(latte_vae_t* v, const void* x, int n_frames, int in_mode, const float* noise, float scale, int out_mode, float* out,
                           void* stream, int stop_after, float* trace_out, int64_t* trace_numel, int* trace_dims) {
  if (!v || !x || !out) return fail(LATTE_ERR_INVALID, "vae_encode: null argument");
  if (!v->encoder) return fail(LATTE_ERR_INVALID, "vae_encode: this handle is a decoder; encode needs latte_vae_create_encoder");
  if (n_frames <= 0 || n_frames > v->max_frames) return fail(LATTE_ERR_STATE, "vae_encode: n_frames exceeds max_frames");
  if (in_mode != 0 && in_mode != 1) return fail(LATTE_ERR_INVALID, "vae_encode: in_mode must be 0 (fp32 NCHW) or 1 (uint8 NHWC)");
  if (out_mode < 0 || out_mode > 2) return fail(LATTE_ERR_INVALID, "vae_encode: out_mode must be 0 (moments), 1 (mode) or 2 (sample)");
  if (out_mode == 2 && !noise) return fail(LATTE_ERR_INVALID, "vae_encode: out_mode 2 (sample) needs noise [N, 4, h, w]");
  int rc = latte_vae_check_weights(v);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int N = n_frames, dt = v->dtype, top = v->ch[3];
  const SplitMask mask = vae_split_mask(VAE_SPLIT_DEFAULT_ENCODER);
  if (!v->bias_folded) {   // the attention's value bias and quant_conv into conv_out
    if ((rc = fold_attention_bias(v, st))) return rc;
    if ((rc = launch_fold_quant_conv(v->eco_raw, v->eco_rb, v->eq_w, v->eq_b, v->eco_w, v->eco_b, 9 * top, st))) return rc;
    v->bias_folded = true;
  }
  half_t *b = v->buf[0], *c = v->buf[1], *d = v->buf[2];
  float *a = v->sbuf[0], *a2 = v->sbuf[1];
  int H = v->img, W = v->img, cur_c = v->ch[0];
  // stage numbering: 0 conv_in | per down block i: resnets 0, 1 (+ down-sampler, i < 3) -> 1..11 | 12 mid.resnet0 | 13 mid.attention |
  // 14 mid.resnet1 | 15 the moments
  StageTrace tr{stop_after, trace_out, trace_numel, trace_dims, "vae_encode_trace"};
  auto traced = [&](int& rc_out) { return tr.hit(a, N, H, W, cur_c, st, rc_out); };
  if ((rc = launch_enc_conv_in(x, in_mode, v->ci_wt, v->ci_b, a, N, H, W, st))) return rc;
  if (traced(rc)) return rc;
  for (int i = 0; i < 4; ++i) {
    for (int r = 0; r < 2; ++r) {
      if ((rc = run_resnet(v, v->down[i][r], &a, &a2, b, c, d, N, H, W, st, 1 + i, mask))) return rc;
      cur_c = v->down[i][r].cout;
      if (traced(rc)) return rc;
    }
    if (i < 3) {   // Downsample2D: pad (0, 1, 0, 1) + stride 2 in the conv's gather, on a half copy of the stream (split: hi d + lo c)
      const bool dn_lo = mask.resample(i);
      if (dn_lo) rc = launch_convert_f32_to_h16_split(a, d, c, (int64_t)N * H * W * cur_c, dt, st);
      else rc = launch_convert_f32_to_h16(a, d, (int64_t)N * H * W * cur_c, dt, st);
      if (rc) return rc;
      kprof_mark(VC_SMALL, st);
      if ((rc = split_conv(v, d, dn_lo ? c : nullptr, v->dnc_w[i], mask.resample_weight(i) ? v->dnc_w_lo[i] : nullptr, v->dnc_b[i], N, H, W, cur_c, cur_c,
                           0, nullptr, a2, 0, 1, st))) return rc;
      std::swap(a, a2);
      H /= 2;
      W /= 2;
      if (traced(rc)) return rc;
    }
  }
  if ((rc = run_resnet(v, v->mid[0], &a, &a2, b, c, d, N, H, W, st, 0, mask))) return rc;
  if (traced(rc)) return rc;
  if ((rc = run_mid_attention(v, a, b, c, d, N, H, W, st))) return rc;
  if (traced(rc)) return rc;
  if ((rc = run_resnet(v, v->mid[1], &a, &a2, b, c, d, N, H, W, st, 0, mask))) return rc;
  if (traced(rc)) return rc;
  half_t* co_lo = mask.conv_out() ? b : nullptr;   // conv_out reads the GroupNorm output as hi + lo (its weights are fp32)
  if ((rc = launch_groupnorm(a, 1, c, v->no_w, v->no_b, v->gn_partial, v->gn_stats, N, H * W, top, 1, dt, st, 1e-6f, groupnorm_max_slabs(), co_lo))) return rc;
  float* mom = (out_mode == 0 && stop_after < 0) ? out : v->moments;
  if ((rc = launch_enc_conv_out(c, co_lo, v->eco_w, v->eco_b, mom, N, H, W, top, dt, st))) return rc;
  if (stop_after >= 0) {
    if (tr.hit(mom, N, 8, H, W, st, rc)) return rc;
    return fail(LATTE_ERR_INVALID, "vae_encode_trace: stage index beyond the last traced stage (15, the moments)");
  }
  if (out_mode == 0) return LATTE_OK;
  return launch_posterior(mom, noise, N, H * W, scale, out_mode, out, st);
}

int latte_vae_encode(latte_vae_t* v, const void* x, int n_frames, int in_mode, const float* noise, float scale, int out_mode, float* out,
                     void* stream) {
  return vae_encode_impl(v, x, n_frames, in_mode, noise, scale, out_mode, out, stream, -1, nullptr, nullptr, nullptr);
}

int latte_vae_posterior(const float* moments, const float* noise, int n, int hw, float scale, int what, float* out, void* stream) {
  if (!moments || !out) return fail(LATTE_ERR_INVALID, "vae_posterior: null argument");
  return launch_posterior(moments, noise, n, hw, scale, what, out, (hipStream_t)stream);
}

int latte_vae_profile_encode(latte_vae_t* v, const void* x, int n_frames, int in_mode, const float* noise, float scale, int out_mode, float* out,
                             float* ms_out, int* launches_out, int n, void* stream) {
  return profile_vae_call("vae_profile_encode", ms_out, launches_out, n, (hipStream_t)stream, [&] {
    return vae_encode_impl(v, x, n_frames, in_mode, noise, scale, out_mode, out, stream, -1, nullptr, nullptr, nullptr);
  });
}

/* test hook (include/latte_amd_debug.h): run the encoder up to and including stage `stop_after` */
int latte_debug_vae_encode_trace(latte_vae_t* v, const void* x, int n_frames, int in_mode, int stop_after, float* trace_out,
                                 int64_t* trace_numel, int* trace_dims, void* stream) {
  if (!trace_out || !trace_numel || !trace_dims || stop_after < 0) return fail(LATTE_ERR_INVALID, "vae_encode_trace: bad arguments");
  return vae_encode_impl(v, x, n_frames, in_mode, nullptr, 1.0f, 0, trace_out, stream, stop_after, trace_out, trace_numel, trace_dims);
}

}  // extern "C"
