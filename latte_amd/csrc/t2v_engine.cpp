// LatteT2V (Latte-1 text-to-video) denoiser forward on the MI355X kernels -- SURVEY.md section 8(f) rank 2.
//
//   LatteT2V.forward                 /root/reference/models/latte_t2v.py:677-941
//   BasicTransformerBlock_ (temporal) :126-396     FeedForward :69-124     AdaLayerNormSingle :398-428
//   spatial block / Attention / PatchEmbed / CaptionProjection / CombinedTimestepSizeEmbeddings: diffusers==0.24.0
//   (not vendored in the reference; restated in oracle/diffusers_standin.py -- parity unpinned for those leaves)
//
// Layout: the same canonical token order as the class-conditional engine (row = (b*F + f)*T + t, fp32 residual stream,
// half GEMM operands); the [B, C, F, H, W] input / output of the reference is permuted once at each end.  Per forward:
//   temb = MLP(sincos(t)); t6 = Linear(SiLU(temb)); mod = adaLN-single tables + t6 (one row per sample)
//   ctx  = caption projection of the T5 tokens (two GEMMs, GELU-tanh between), shared by the frames of a sample
//   spatial block : LN-modulate -> fused q|k|v GEMM -> self-attention over T tokens -> out GEMM (gated residual)
//                   -> q GEMM on the UN-normalised stream, k|v GEMM on ctx -> cross-attention (additive mask bias)
//                   -> out GEMM (residual, gate 1) -> LN-modulate -> fc1 GELU -> fc2 (gated residual)
//   temporal block: the same without cross-attention, attention over the F frames of a token (row stride T);
//                   temp_pos_embed is added in front of the first one
//   head          : LN-modulate with scale_shift_table + temb -> proj_out -> unpatchify
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/latte_amd.h"
#include "block.h"
#include "plan.h"

using namespace latte;

namespace {

enum T2VKind { TK_F32, TK_F32_TRANSPOSE, TK_H16 };   // WeightSlot::kind

struct T2VBlock : BlockLinears {   // attn1 and ff; attn1.to_out is proj
  half_t *q2_w, *kv2_w, *o2_w;     // attn2 (cross-attention): spatial blocks only
  float *q2_b, *kv2_b, *o2_b;
};

void sincos_1d(int dim, const std::vector<double>& pos, std::vector<double>& out /* [n][dim] */) {
  const int half = dim / 2, n = (int)pos.size();
  out.assign((size_t)n * dim, 0.0);
  for (int m = 0; m < n; ++m)
    for (int d = 0; d < half; ++d) {
      const double omega = 1.0 / std::pow(10000.0, (double)d / (dim / 2.0));
      const double v = pos[m] * omega;
      out[(size_t)m * dim + d] = std::sin(v);
      out[(size_t)m * dim + half + d] = std::cos(v);
    }
}

// The block policy of this engine (BlockCtx, block.h).  These values reproduce the launches t2v_core made while it carried its own copy of
// the block body; they are inherited, NOT measured against the class-conditional engine's defaults.
constexpr int T2V_RMW_MODE = 0;             // gated GEMMs (attn2's out-projection too): fragment-wise residual accesses (engine.cpp: line-wise)
constexpr int T2V_STREAM_POLICY = 0;        // no `nt` hints on the once-used streams
constexpr int T2V_GATED_SPLIT_K = 1;        // never split: a gated GEMM is one launch_gemm at every batch (and no split-K workspace exists)
constexpr bool T2V_TEMP_EMBED_IN_FC2 = false;   // temp_pos_embed through block 1's first LayerNorm pass, and only when F > 1
constexpr int T2V_GEMM_VARIANT = 0;         // every GEMM on the per-shape tile choice
constexpr int T2V_GUIDED_SPLIT = 0;         // plain f16 operands in guided chains too
constexpr EventProfile* T2V_PROFILE = nullptr;   // no per-launch events

}  // namespace

struct latte_t2v {
  latte_t2v_config_t cfg;
  int max_batch = 0, D = 0, T = 0, G = 0, F = 0, H = 0, P = 0, KPE = 0, Hm = 0, hd = 0, heads = 0, L = 0, Cc = 0, maxk = 0;
  int nblk = 0;            // 2 * num_layers: block 2i = spatial i, 2i + 1 = temporal i
  int fuse_qkv_attn = 3;   // as latte_engine: bit 0 spatial / bit 1 temporal blocks run to_q|k|v + attention as ONE kernel (qkv_attn.hip)
                           // where the shape allows it (256 tokens per frame / 16 frames); latte_t2v_set_option("fuse_qkv_attn", ...)
  int64_t rows_pad = 0, trows_pad = 0;
  std::vector<T2VBlock> blocks;
  float *tables = nullptr, *head_table = nullptr, *pos = nullptr, *temp = nullptr, *pe_wt = nullptr, *pe_b = nullptr,
        *t1_w = nullptr, *t1_b = nullptr, *t2_w = nullptr, *t2_b = nullptr, *ada_w = nullptr, *ada_b = nullptr, *fin_wt = nullptr,
        *fin_b = nullptr, *cap1_b = nullptr, *cap2_b = nullptr, *ones = nullptr;
  half_t *cap1_w = nullptr, *cap2_w = nullptr;
  float *xin = nullptr, *xres = nullptr, *temb0 = nullptr, *temb = nullptr, *t6 = nullptr, *mod = nullptr, *out_bf = nullptr,
        *kbias = nullptr;
  half_t *xn = nullptr, *qkv = nullptr, *hbuf = nullptr, *ctx_in = nullptr, *ctx1 = nullptr, *ctx = nullptr, *kv = nullptr;
  // text context of a chain (latte_t2v_set_text): cross-attention K|V of EVERY spatial block + the additive mask bias,
  // functions of the text alone, computed once instead of once per denoising step
  half_t* kv_all = nullptr;         // [num_layers][trows_pad][2D]
  int txt_batch = 0, txt_nk = 0;    // > 0: a text context for that many samples / tokens is installed
  bool txt_has_mask = false;
  int64_t* tsteps = nullptr;        // device copy of a chain's timesteps (latte_t2v_guided_ddim_loop)
  int tsteps_cap = 0;
  // latte_t2v_guided_linear_loop: a ring of three remembered outputs and the scaled denoiser input, max_batch / 2 latents each
  float *hist[3] = {nullptr, nullptr, nullptr}, *x_scaled = nullptr;
  // overlapping temporal windows (taken from the arena by the first windowed loop): the gathered clips, max_batch / 2 latents, and the
  // merged output of the guidance pair (the size of out_bf)
  float *win_clips = nullptr, *win_merged = nullptr;
  WeightSlots weights;
  DeviceArena arena;
};

extern "C" {

int latte_t2v_create(const latte_t2v_config_t* cfg, int max_batch, latte_t2v_t** out) {
  if (!cfg || !out || max_batch <= 0) return fail(LATTE_ERR_INVALID, "t2v_create: bad arguments");
  const auto& c = *cfg;
  const int D = c.num_attention_heads * c.attention_head_dim;
  if (c.attention_head_dim != 64 && c.attention_head_dim != 72) return fail(LATTE_ERR_INVALID, "t2v_create: attention_head_dim must be 64 or 72");
  if (D % 128 != 0 || D > 1152) return fail(LATTE_ERR_INVALID, "t2v_create: heads * head_dim must be a multiple of 128, at most 1152");
  if (c.cross_attention_dim != D) return fail(LATTE_ERR_INVALID, "t2v_create: cross_attention_dim must equal the inner dimension (caption projection output)");
  if (c.caption_channels <= 0 || c.caption_channels % 64) return fail(LATTE_ERR_INVALID, "t2v_create: caption_channels must be a multiple of 64");
  if (c.patch_size <= 0 || c.sample_size % c.patch_size) return fail(LATTE_ERR_INVALID, "t2v_create: sample_size % patch_size != 0");
  if (c.in_channels != 4) return fail(LATTE_ERR_INVALID, "t2v_create: in_channels must be 4");
  if (c.num_layers <= 0 || c.video_length <= 0 || c.max_text_tokens <= 0) return fail(LATTE_ERR_INVALID, "t2v_create: bad sizes");
  // f16 operands only: the type the reference runs this transformer in (sample_t2x.py:29 `.to(device, dtype=torch.float16)`).  With
  // bf16 operands the guidance pair (scale 7.5, pipeline_latte.py:752-754) amplifies the 2^-9 operand roundoff past the 1e-3
  // parity bar on every stress case (measured < 3e-3), so the type is not offered.
  if (c.compute_dtype != LATTE_DTYPE_F16) return fail(LATTE_ERR_INVALID, "t2v_create: LatteT2V runs with f16 MFMA operands only (LATTE_DTYPE_F16)");

  auto* e = new latte_t2v();
  e->cfg = c;
  e->max_batch = max_batch;
  e->D = D;
  e->heads = c.num_attention_heads;
  e->hd = c.attention_head_dim;
  e->G = c.sample_size / c.patch_size;
  e->T = e->G * e->G;
  e->F = c.video_length;
  e->H = c.sample_size;
  e->P = c.patch_size * c.patch_size * c.out_channels;
  e->KPE = c.in_channels * c.patch_size * c.patch_size;
  e->Hm = 4 * D;
  e->L = c.num_layers;
  e->nblk = 2 * c.num_layers;
  e->Cc = c.caption_channels;
  e->maxk = c.max_text_tokens;
  e->rows_pad = ((int64_t)max_batch * e->F * e->T + 255) / 256 * 256;
  e->trows_pad = ((int64_t)max_batch * e->maxk + 255) / 256 * 256;
  int rc = LATTE_OK;
#define TRY(x) do { if ((rc = (x))) { latte_t2v_destroy(e); return rc; } } while (0)
  TRY(e->arena.alloc(&e->tables, (size_t)e->nblk * 6 * D));
  TRY(e->arena.alloc(&e->head_table, (size_t)2 * D));
  TRY(e->arena.alloc(&e->pos, (size_t)e->T * D));
  TRY(e->arena.alloc(&e->temp, (size_t)e->F * D));
  TRY(e->arena.alloc(&e->pe_wt, (size_t)e->KPE * D));
  TRY(e->arena.alloc(&e->pe_b, (size_t)D));
  TRY(e->arena.alloc(&e->t1_w, (size_t)D * 256));
  TRY(e->arena.alloc(&e->t1_b, (size_t)D));
  TRY(e->arena.alloc(&e->t2_w, (size_t)D * D));
  TRY(e->arena.alloc(&e->t2_b, (size_t)D));
  TRY(e->arena.alloc(&e->ada_w, (size_t)6 * D * D));
  TRY(e->arena.alloc(&e->ada_b, (size_t)6 * D));
  TRY(e->arena.alloc(&e->fin_wt, (size_t)D * e->P));
  TRY(e->arena.alloc(&e->fin_b, (size_t)e->P));
  TRY(e->arena.alloc(&e->cap1_w, (size_t)D * e->Cc));
  TRY(e->arena.alloc(&e->cap1_b, (size_t)D));
  TRY(e->arena.alloc(&e->cap2_w, (size_t)D * D));
  TRY(e->arena.alloc(&e->cap2_b, (size_t)D));
  TRY(e->arena.alloc(&e->ones, (size_t)D));
  TRY(launch_fill_f32(e->ones, 1.0f, (size_t)D, nullptr));

  e->weights.add("scale_shift_table", 2 * D, TK_F32, e->head_table);
  e->weights.add("pos_embed.proj.weight", (int64_t)D * e->KPE, TK_F32_TRANSPOSE, e->pe_wt, D, e->KPE);
  e->weights.add("pos_embed.proj.bias", D, TK_F32, e->pe_b);
  e->weights.add("adaln_single.emb.timestep_embedder.linear_1.weight", (int64_t)D * 256, TK_F32, e->t1_w);
  e->weights.add("adaln_single.emb.timestep_embedder.linear_1.bias", D, TK_F32, e->t1_b);
  e->weights.add("adaln_single.emb.timestep_embedder.linear_2.weight", (int64_t)D * D, TK_F32, e->t2_w);
  e->weights.add("adaln_single.emb.timestep_embedder.linear_2.bias", D, TK_F32, e->t2_b);
  e->weights.add("adaln_single.linear.weight", (int64_t)6 * D * D, TK_F32, e->ada_w);
  e->weights.add("adaln_single.linear.bias", 6 * D, TK_F32, e->ada_b);
  e->weights.add("caption_projection.linear_1.weight", (int64_t)D * e->Cc, TK_H16, e->cap1_w);
  e->weights.add("caption_projection.linear_1.bias", D, TK_F32, e->cap1_b);
  e->weights.add("caption_projection.linear_2.weight", (int64_t)D * D, TK_H16, e->cap2_w);
  e->weights.add("caption_projection.linear_2.bias", D, TK_F32, e->cap2_b);
  e->weights.add("caption_projection.y_embedding", (int64_t)120 * e->Cc, TK_F32, nullptr).optional = true;   // null-caption buffer, unused at inference
  e->weights.add("proj_out.weight", (int64_t)e->P * D, TK_F32_TRANSPOSE, e->fin_wt, e->P, D);
  e->weights.add("proj_out.bias", e->P, TK_F32, e->fin_b);

  e->blocks.resize(e->nblk);
  for (int i = 0; i < e->nblk; ++i) {
    T2VBlock& w = e->blocks[i];
    const bool spatial = (i % 2) == 0;
    const std::string p = std::string(spatial ? "transformer_blocks." : "temporal_transformer_blocks.") + std::to_string(i / 2) + ".";
    TRY(alloc_block_linears(e->arena, w, D, e->Hm));
    e->weights.add(p + "scale_shift_table", 6 * D, TK_F32, e->tables + (size_t)i * 6 * D);
    // to_q | to_k | to_v concatenated: one fused GEMM, columns ordered [3][heads][hd] like latte.py:50
    e->weights.add(p + "attn1.to_q.weight", (int64_t)D * D, TK_H16, w.qkv_w);
    e->weights.add(p + "attn1.to_k.weight", (int64_t)D * D, TK_H16, w.qkv_w + (size_t)D * D);
    e->weights.add(p + "attn1.to_v.weight", (int64_t)D * D, TK_H16, w.qkv_w + (size_t)2 * D * D);
    e->weights.add(p + "attn1.to_q.bias", D, TK_F32, w.qkv_b);
    e->weights.add(p + "attn1.to_k.bias", D, TK_F32, w.qkv_b + D);
    e->weights.add(p + "attn1.to_v.bias", D, TK_F32, w.qkv_b + 2 * D);
    e->weights.add(p + "attn1.to_out.0.weight", (int64_t)D * D, TK_H16, w.proj_w);
    e->weights.add(p + "attn1.to_out.0.bias", D, TK_F32, w.proj_b);
    if (spatial) {
      TRY(e->arena.alloc(&w.q2_w, (size_t)D * D));
      TRY(e->arena.alloc(&w.q2_b, (size_t)D));
      TRY(e->arena.alloc(&w.kv2_w, (size_t)2 * D * D));
      TRY(e->arena.alloc(&w.kv2_b, (size_t)2 * D));
      TRY(e->arena.alloc(&w.o2_w, (size_t)D * D));
      TRY(e->arena.alloc(&w.o2_b, (size_t)D));
      e->weights.add(p + "attn2.to_q.weight", (int64_t)D * D, TK_H16, w.q2_w);
      e->weights.add(p + "attn2.to_q.bias", D, TK_F32, w.q2_b);
      e->weights.add(p + "attn2.to_k.weight", (int64_t)D * D, TK_H16, w.kv2_w);
      e->weights.add(p + "attn2.to_v.weight", (int64_t)D * D, TK_H16, w.kv2_w + (size_t)D * D);
      e->weights.add(p + "attn2.to_k.bias", D, TK_F32, w.kv2_b);
      e->weights.add(p + "attn2.to_v.bias", D, TK_F32, w.kv2_b + D);
      e->weights.add(p + "attn2.to_out.0.weight", (int64_t)D * D, TK_H16, w.o2_w);
      e->weights.add(p + "attn2.to_out.0.bias", D, TK_F32, w.o2_b);
    }
    e->weights.add(p + "ff.net.0.proj.weight", (int64_t)e->Hm * D, TK_H16, w.fc1_w);
    e->weights.add(p + "ff.net.0.proj.bias", e->Hm, TK_F32, w.fc1_b);
    e->weights.add(p + "ff.net.2.weight", (int64_t)D * e->Hm, TK_H16, w.fc2_w);
    e->weights.add(p + "ff.net.2.bias", D, TK_F32, w.fc2_b);
  }

  // fixed tables (non-persistent buffers of the reference: PatchEmbed.pos_embed, temp_pos_embed, latte_t2v.py:571-581,670-671)
  {
    const int G = e->G;
    const double base_size = (double)(c.sample_size / c.patch_size), interp = (double)std::max(c.sample_size / 64, 1);
    std::vector<double> gw((size_t)G * G), gh((size_t)G * G), ew, eh;
    for (int i = 0; i < G; ++i)        // meshgrid(grid_w, grid_h): grid[0][i][j] = w_j, grid[1][i][j] = h_i (float32 positions)
      for (int j = 0; j < G; ++j) {
        gw[(size_t)i * G + j] = (double)((float)j / (float)((double)G / base_size) / (float)interp);
        gh[(size_t)i * G + j] = (double)((float)i / (float)((double)G / base_size) / (float)interp);
      }
    sincos_1d(D / 2, gw, ew);
    sincos_1d(D / 2, gh, eh);
    std::vector<float> pos((size_t)e->T * D);
    for (int t = 0; t < e->T; ++t)
      for (int d = 0; d < D / 2; ++d) {
        pos[(size_t)t * D + d] = (float)ew[(size_t)t * (D / 2) + d];
        pos[(size_t)t * D + D / 2 + d] = (float)eh[(size_t)t * (D / 2) + d];
      }
    LATTE_HIP(hipMemcpy(e->pos, pos.data(), pos.size() * sizeof(float), hipMemcpyHostToDevice));
    std::vector<double> fp(e->F), et;
    for (int f = 0; f < e->F; ++f) fp[f] = (double)f;
    sincos_1d(D, fp, et);
    std::vector<float> tf(et.begin(), et.end());
    LATTE_HIP(hipMemcpy(e->temp, tf.data(), tf.size() * sizeof(float), hipMemcpyHostToDevice));
  }

  const int64_t R = e->rows_pad, TR = e->trows_pad;
  TRY(e->weights.alloc_stage(e->arena, true));
  TRY(e->arena.alloc(&e->xin, (size_t)max_batch * e->F * c.in_channels * e->H * e->H));
  TRY(e->arena.alloc(&e->out_bf, (size_t)max_batch * e->F * c.out_channels * e->H * e->H));
  TRY(e->arena.alloc(&e->xres, (size_t)R * D));
  TRY(e->arena.alloc(&e->xn, (size_t)R * D));
  TRY(e->arena.alloc(&e->qkv, (size_t)R * 3 * D));
  TRY(e->arena.alloc(&e->hbuf, (size_t)R * e->Hm));
  TRY(e->arena.alloc(&e->ctx_in, (size_t)TR * e->Cc));
  TRY(e->arena.alloc(&e->ctx1, (size_t)TR * D));
  TRY(e->arena.alloc(&e->ctx, (size_t)TR * D));
  TRY(e->arena.alloc(&e->kv, (size_t)TR * 2 * D));
  TRY(e->arena.alloc(&e->kv_all, (size_t)c.num_layers * TR * 2 * D));
  TRY(e->arena.alloc(&e->tsteps, (size_t)1024));
  e->tsteps_cap = 1024;
  const size_t chain_latents = (size_t)(max_batch / 2) * e->F * c.in_channels * e->H * e->H;
  for (int j = 0; j < 3; ++j) TRY(e->arena.alloc(&e->hist[j], chain_latents));
  TRY(e->arena.alloc(&e->x_scaled, chain_latents));
  TRY(e->arena.alloc(&e->kbias, (size_t)max_batch * e->maxk));
  TRY(e->arena.alloc(&e->temb0, (size_t)max_batch * D));
  TRY(e->arena.alloc(&e->temb, (size_t)max_batch * D));
  TRY(e->arena.alloc(&e->t6, (size_t)max_batch * 6 * D));
  TRY(e->arena.alloc(&e->mod, (size_t)max_batch * (6 * e->nblk + 2) * D));
#undef TRY
  LATTE_HIP(hipDeviceSynchronize());
  *out = e;
  return LATTE_OK;
}

void latte_t2v_destroy(latte_t2v_t* e) {
  delete e;   // the arena frees every device block
}

int latte_t2v_num_keys(const latte_t2v_t* e) { return e ? e->weights.size() : 0; }
const char* latte_t2v_key(const latte_t2v_t* e, int i) { return e ? e->weights.key(i) : nullptr; }

int latte_t2v_load_tensor(latte_t2v_t* e, const char* key, const float* data, int64_t numel, int on_device, void* stream) {
  if (!e || !key || !data) return fail(LATTE_ERR_INVALID, "t2v_load_tensor: null argument");
  hipStream_t st = (hipStream_t)stream;
  WeightSlot* slot = nullptr;
  const float* src = nullptr;
  int rc = e->weights.begin_load("t2v_load_tensor", key, data, numel, on_device, st, &slot, &src);
  if (rc || slot->optional) return rc;
  WeightSlot& s = *slot;
  switch (s.kind) {
    case TK_F32: LATTE_HIP(hipMemcpyAsync(s.dst, src, sizeof(float) * numel, hipMemcpyDeviceToDevice, st)); break;
    case TK_F32_TRANSPOSE: rc = launch_transpose_f32(src, (float*)s.dst, s.rows, s.cols, st); break;
    case TK_H16: rc = launch_convert_f32_to_h16(src, (half_t*)s.dst, numel, e->cfg.compute_dtype, st); break;
  }
  if (rc || (rc = e->weights.end_load(s, on_device, st))) return rc;
  e->txt_batch = 0;   // an installed text context was projected with the old weights
  return LATTE_OK;
}

int latte_t2v_set_option(latte_t2v_t* e, const char* name, int64_t value) {
  if (!e || !name) return fail(LATTE_ERR_INVALID, "t2v_set_option: null argument");
  if (std::string(name) == "fuse_qkv_attn") {
    if (value < 0 || value > 31) return fail(LATTE_ERR_INVALID, "fuse_qkv_attn: bit 0 = spatial blocks, bit 1 = temporal blocks, bits 2-3 = schedule variant");
    e->fuse_qkv_attn = (int)value;
    return LATTE_OK;
  }
  return fail(LATTE_ERR_INVALID, std::string("t2v_set_option: unknown option '") + name + "'");
}

int latte_t2v_check_weights(latte_t2v_t* e) {
  if (!e) return fail(LATTE_ERR_INVALID, "t2v_check_weights: null engine");
  return e->weights.check_loaded();
}

// Text context: caption projection (latte_t2v.py:781-793: Linear -> GELU(tanh) -> Linear on [B * Lk, caption_channels]),
// the k|v projection of every spatial block's cross-attention on it, and the additive score bias of the padded tokens
// ((1 - mask) * -10000, :746-749).  All of it depends on the text only.
static int t2v_text_context(latte_t2v* e, const float* enc, const float* mask, int B, int Lk, hipStream_t st) {
  const auto& c = e->cfg;
  const int D = e->D, dt = c.compute_dtype, MT = B * Lk;
  int rc;
  GemmArgs g{};
  g.rows_per_sample = MT; g.gate_stride = 0;
  if ((rc = launch_convert_f32_to_h16(enc, e->ctx_in, (int64_t)MT * e->Cc, dt, st))) return rc;
  g.M = MT; g.A = e->ctx_in; g.W = e->cap1_w; g.bias = e->cap1_b; g.out = e->ctx1; g.N = D; g.K = e->Cc;
  if ((rc = launch_gemm(g, EPI_BIAS_GELU_H16, dt, 0, st))) return rc;
  g.A = e->ctx1; g.W = e->cap2_w; g.bias = e->cap2_b; g.out = e->ctx; g.K = D;
  if ((rc = launch_gemm(g, EPI_BIAS_H16, dt, 0, st))) return rc;
  for (int l = 0; l < e->L; ++l) {
    const T2VBlock& w = e->blocks[2 * l];
    GemmArgs gk{};
    gk.M = MT; gk.rows_per_sample = MT; gk.A = e->ctx; gk.W = w.kv2_w; gk.bias = w.kv2_b;
    gk.out = e->kv_all + (size_t)l * e->trows_pad * 2 * D; gk.N = 2 * D; gk.K = D;
    if ((rc = launch_gemm(gk, EPI_BIAS_H16, dt, 0, st))) return rc;
  }
  e->txt_has_mask = mask != nullptr;
  if (mask && (rc = launch_mask_bias(mask, e->kbias, (size_t)MT, st))) return rc;
  e->txt_batch = B;
  e->txt_nk = Lk;
  return LATTE_OK;
}

// The denoiser on an installed text context.  x: [xb, C, F, H, W] with xb = B, or B / 2 when `dup` (guidance pair: both
// halves of the batch see the same latents, pipeline_latte.py:725); t: device int64, one per sample or ONE shared by all
// (t_shared: the adaLN-single rows are then computed once, row stride 0).  Result: e->out_bf, frame layout [B * F, Cout, H, W].
static int t2v_core(latte_t2v* e, const float* x, const int64_t* t, bool t_shared, int B, bool dup, int enable_temporal,
                    hipStream_t st) {
  const auto& c = e->cfg;
  const int D = e->D, T = e->T, F = e->F, dt = c.compute_dtype, Lk = e->txt_nk;
  const int M = B * F * T, rps = F * T;
  const int nt = t_shared ? 1 : B;
  const int mstride = t_shared ? 0 : (6 * e->nblk + 2) * D;
  const float* kbias = e->txt_has_mask ? e->kbias : nullptr;
  int rc;
  // ---- conditioning: embedded timestep, its 6D projection, all adaLN-single rows (latte_t2v.py:398-428,775-779)
  if ((rc = launch_small_linear(IN_TFREQ, nullptr, t, e->t1_w, e->t1_b, nullptr, nullptr, e->temb0, nt, D, 256, D, st))) return rc;
  if ((rc = launch_small_linear(IN_SILU, e->temb0, nullptr, e->t2_w, e->t2_b, nullptr, nullptr, e->temb, nt, D, D, D, st))) return rc;
  if ((rc = launch_small_linear(IN_SILU, e->temb, nullptr, e->ada_w, e->ada_b, nullptr, nullptr, e->t6, nt, 6 * D, D, 6 * D, st))) return rc;
  if ((rc = launch_adaln_single(e->tables, e->head_table, e->t6, e->temb, e->mod, nt, e->nblk, D, st))) return rc;
  // ---- [xb, C, F, H, W] -> frames, patch embed + positions (twice for the guidance pair)
  const int xb = dup ? B / 2 : B;
  if ((rc = launch_permute_cf(x, e->xin, xb, c.in_channels, F, e->H * e->H, 1, st))) return rc;
  if ((rc = launch_patch_embed(e->xin, e->pe_wt, e->pe_b, e->pos, e->xres, xb * F, c.in_channels, e->H, c.patch_size, D, st))) return rc;
  if (dup && (rc = launch_patch_embed(e->xin, e->pe_wt, e->pe_b, e->pos, e->xres + (size_t)xb * rps * D, xb * F, c.in_channels,
                                      e->H, c.patch_size, D, st))) return rc;

  BlockCtx bc{};   // zero: no split-K workspace, no guided-split operands
  bc.B = B; bc.F = F; bc.T = T; bc.D = D; bc.heads = e->heads; bc.hd = e->hd; bc.Hm = e->Hm; bc.dt = dt;
  bc.xres = e->xres; bc.xn = e->xn; bc.qkv = e->qkv; bc.hbuf = e->hbuf;
  bc.mod_stride = mstride;
  bc.temp = F > 1 ? e->temp : nullptr;   // latte_t2v.py:889-890
  bc.te_in_fc2 = T2V_TEMP_EMBED_IN_FC2;
  bc.fuse_qkv_attn = e->fuse_qkv_attn;
  for (int k = 0; k < 4; ++k) bc.gemm_variant_of[k] = T2V_GEMM_VARIANT;
  bc.gated_split_k = T2V_GATED_SPLIT_K; bc.rmw_mode = T2V_RMW_MODE; bc.stream_policy = T2V_STREAM_POLICY;
  bc.gsplit = T2V_GUIDED_SPLIT;
  bc.prof = T2V_PROFILE;
  for (int i = 0; i < e->nblk; ++i) {
    const bool spatial = (i % 2) == 0;
    if (!spatial && !enable_temporal) continue;
    const T2VBlock& w = e->blocks[i];
    const float* mb = e->mod + (size_t)i * 6 * D;   // shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
    if ((rc = block_attention(bc, w, i, mb, st))) return rc;
    if (spatial) {
      // cross-attention on the UN-normalised stream (PixArt: no norm before attn2, no gate after it)
      if ((rc = launch_convert_f32_to_h16(e->xres, e->xn, (int64_t)M * D, dt, st))) return rc;
      GemmArgs g{};
      g.M = M; g.rows_per_sample = rps; g.gate_stride = mstride; g.rmw_mode = T2V_RMW_MODE; g.stream_policy = T2V_STREAM_POLICY;
      g.A = e->xn; g.W = w.q2_w; g.bias = w.q2_b; g.out = e->qkv; g.N = D; g.K = D;
      if ((rc = launch_gemm(g, EPI_BIAS_H16, dt, T2V_GEMM_VARIANT, st))) return rc;
      AttnArgs x2{};
      x2.qkv = e->qkv; x2.q_ld = D; x2.kv = e->kv_all + (size_t)(i / 2) * e->trows_pad * 2 * D; x2.kbias = kbias; x2.Lk = Lk;
      x2.out = e->xn;
      x2.heads = e->heads; x2.hd = e->hd; x2.D = D; x2.sample_stride = rps; x2.scale = 1.0f / std::sqrt((float)e->hd);
      seq_layout(x2, true, B, F, T);
      if ((rc = launch_cross_attention(x2, dt, st))) return rc;
      g.A = e->xn; g.W = w.o2_w; g.bias = w.o2_b; g.out = e->xres; g.gate = e->ones; g.gate_stride = 0;
      if ((rc = launch_gemm(g, EPI_GATE_RES_F32, dt, T2V_GEMM_VARIANT, st))) return rc;
    }
    if ((rc = block_mlp(bc, w, i, mb, st))) return rc;
  }
  // ---- output head (latte_t2v.py:913-931), frame layout
  const float* hm = e->mod + (size_t)e->nblk * 6 * D;   // chunk(2): shift, scale
  return launch_final_layer(e->xres, hm, hm + D, mstride, e->fin_wt, e->fin_b, e->out_bf, M, D, rps, T, c.patch_size,
                            c.out_channels, e->H, st);
}

int latte_t2v_set_text(latte_t2v_t* e, const float* encoder_hidden_states, const float* encoder_attention_mask, int batch,
                       int n_text, void* stream) {
  if (!e) return fail(LATTE_ERR_INVALID, "t2v_set_text: null engine");
  if (!encoder_hidden_states) {   // uninstall
    e->txt_batch = 0;
    return LATTE_OK;
  }
  int rc = latte_t2v_check_weights(e);
  if (rc) return rc;
  if (batch <= 0 || batch > e->max_batch) return fail(LATTE_ERR_STATE, "t2v_set_text: batch exceeds max_batch of the engine");
  if (n_text <= 0 || n_text > e->maxk) return fail(LATTE_ERR_STATE, "t2v_set_text: more text tokens than max_text_tokens");
  return t2v_text_context(e, encoder_hidden_states, encoder_attention_mask, batch, n_text, (hipStream_t)stream);
}

int latte_t2v_forward(latte_t2v_t* e, const float* x, const int64_t* t, const float* encoder_hidden_states,
                      const float* encoder_attention_mask, int batch, int n_text, int enable_temporal_attentions, float* out,
                      void* stream) {
  if (!e || !x || !t || !out) return fail(LATTE_ERR_INVALID, "t2v_forward: null argument");
  int rc = latte_t2v_check_weights(e);
  if (rc) return rc;
  if (batch <= 0 || batch > e->max_batch) return fail(LATTE_ERR_STATE, "t2v_forward: batch exceeds max_batch of the engine");
  hipStream_t st = (hipStream_t)stream;
  if (encoder_hidden_states) {
    if (n_text <= 0 || n_text > e->maxk) return fail(LATTE_ERR_STATE, "t2v_forward: more text tokens than max_text_tokens");
    if ((rc = t2v_text_context(e, encoder_hidden_states, encoder_attention_mask, batch, n_text, st))) return rc;
  } else if (e->txt_batch != batch) {
    return fail(LATTE_ERR_STATE, "t2v_forward: no encoder_hidden_states and no installed text context for this batch (latte_t2v_set_text)");
  }
  if ((rc = t2v_core(e, x, t, false, batch, false, enable_temporal_attentions, st))) return rc;
  const auto& c = e->cfg;
  return launch_permute_cf(e->out_bf, out, batch, c.out_channels, e->F, e->H * e->H, 0, st);   // back to [B, C, F, H, W]
}

// The argument block the guided loops share: loaded weights, the guidance pair within max_batch, its text context, C or 2C outputs.
// With windows (`ws`) the window set is checked behind the weights, and the pair is 2 * samples * W clips.
static int t2v_chain_check(const std::string& who, latte_t2v* e, int samples, const WindowSet* ws = nullptr) {
  int rc = latte_t2v_check_weights(e);
  if (rc) return rc;
  if (ws && (rc = window_check(who, *ws, e->H * e->H))) return rc;
  const int64_t B = 2 * (int64_t)samples * (ws ? ws->count() : 1);
  if (B > e->max_batch)
    return fail(LATTE_ERR_STATE, who + (ws ? ": the clips of the guidance pair (2 * samples * windows) exceed max_batch of the engine"
                                           : ": the guidance pair exceeds max_batch of the engine"));
  if (e->txt_batch != B)
    return fail(LATTE_ERR_STATE, who + ": install the text context of the guidance pair first "
                                 "(latte_t2v_set_text with [negative | prompt] embeddings, 2 * samples rows" + (ws ? " per window)" : ")"));
  const auto& c = e->cfg;
  if (c.out_channels != c.in_channels && c.out_channels != 2 * c.in_channels)
    return fail(LATTE_ERR_INVALID, who + ": out_channels must be C or 2C (learned sigma)");
  return LATTE_OK;
}

// n host timesteps (n <= tsteps_cap, checked by the caller) into e->tsteps
static int t2v_upload_timesteps(latte_t2v* e, const int64_t* ts, int n, hipStream_t st) {
  LATTE_HIP(hipMemcpyAsync(e->tsteps, ts, sizeof(int64_t) * n, hipMemcpyHostToDevice, st));
  LATTE_HIP(hipStreamSynchronize(st));   // the caller's host array may go away
  return LATTE_OK;
}

// One evaluation of the guidance pair of a chain on x_in [samples, C, frames, HW], *out = where its output lies
// ([2 * samples, frames, Cout, HW]): t2v_core itself, or with windows gather -> t2v_core on the 2 * samples * W clips -> merge.  The
// window buffers come from the arena on first use.
static int t2v_chain_forward(latte_t2v* e, const WindowSet* ws, const float* x_in, const int64_t* t, int samples, int enable_temporal,
                             hipStream_t st, const float** out) {
  const auto& c = e->cfg;
  const int HW = e->H * e->H;
  int rc;
  if (ws) {
    const size_t frame = (size_t)e->F * HW;
    if (!e->win_clips && (rc = e->arena.alloc(&e->win_clips, (size_t)(e->max_batch / 2) * frame * c.in_channels, false))) return rc;
    if (!e->win_merged && (rc = e->arena.alloc(&e->win_merged, (size_t)e->max_batch * frame * c.out_channels, false))) return rc;
    if ((rc = launch_window_gather(x_in, e->win_clips, samples, *ws, c.in_channels, HW, 1, st))) return rc;
    x_in = e->win_clips;
  }
  const int B = 2 * samples * (ws ? ws->count() : 1);
  if ((rc = t2v_core(e, x_in, t, true, B, true, enable_temporal, st))) return rc;
  *out = e->out_bf;
  if (!ws) return LATTE_OK;
  *out = e->win_merged;
  return launch_window_merge(e->out_bf, e->win_merged, 2 * samples, *ws, c.out_channels, HW, 0, st);
}

// The guided DDIM loop (diffusers DDIMScheduler.step, eta = 0, no clipping).  With `known`, the known part of x is replaced at the level
// each step reaches: noise slab 0 for the blend at alpha_t[0] before step 0, slab k + 1 for the blend at alpha_prev[k] after step k; the
// last step blends with (1, 0).  known == NULL: no blends, no noise read.
static int t2v_ddim_chain(const std::string& who, latte_t2v* e, float* x, int samples, int n_steps, const int64_t* timesteps,
                          const double* alpha_t, const double* alpha_prev, float guidance_scale, const float* known, const float* mask,
                          const float* noise, int enable_temporal_attentions, hipStream_t st, const WindowSet* ws = nullptr) {
  int rc = t2v_chain_check(who, e, samples, ws);
  if (rc) return rc;
  const auto& c = e->cfg;
  const int HW = e->H * e->H, frames = ws ? ws->L : e->F;
  if (known && HW % 4) return fail(LATTE_ERR_INVALID, who + ": H * W must be a multiple of 4 (16-byte accesses of the blend kernel)");
  if (n_steps > e->tsteps_cap) return fail(LATTE_ERR_INVALID, who + ": more than 1024 steps");
  for (int k = 0; k < n_steps; ++k)
    if (!(alpha_t[k] > 0.0 && alpha_t[k] < 1.0) || !(alpha_prev[k] > 0.0 && alpha_prev[k] <= 1.0))
      return fail(LATTE_ERR_INVALID, who + ": alpha out of range");
  if ((rc = t2v_upload_timesteps(e, timesteps, n_steps, st))) return rc;
  const size_t numel = (size_t)samples * c.in_channels * e->F * HW;
  auto blend = [&](double abar, const float* nz) {
    const bool clean = nz == nullptr;
    return launch_known_blend(x, known, mask, nz, 0, 0, clean ? 1.0f : (float)std::sqrt(abar), clean ? 0.0f : (float)std::sqrt(1.0 - abar),
                              samples, e->F, c.in_channels, HW, 1, st);
  };
  if (known && (rc = blend(alpha_t[0], noise))) return rc;
  for (int k = 0; k < n_steps; ++k) {
    const float* mo;
    if ((rc = t2v_chain_forward(e, ws, x, e->tsteps + k, samples, enable_temporal_attentions, st, &mo))) return rc;
    // Python-float coefficients times fp32 tensors
    const double at = alpha_t[k], ap = alpha_prev[k];
    if ((rc = launch_t2v_guided_ddim(x, mo, samples, c.in_channels, c.out_channels, frames, HW, guidance_scale,
                                     (float)std::sqrt(1.0 - at), (float)std::sqrt(at), (float)std::sqrt(ap),
                                     (float)std::sqrt(1.0 - ap), st))) return rc;
    if (known && (rc = blend(ap, k + 1 < n_steps ? noise + (size_t)(k + 1) * numel : nullptr))) return rc;
  }
  return LATTE_OK;
}

int latte_t2v_guided_ddim_loop(latte_t2v_t* e, float* x, int samples, int n_steps, const int64_t* timesteps,
                               const double* alpha_t, const double* alpha_prev, float guidance_scale,
                               int enable_temporal_attentions, void* stream) {
  if (!e || !x || !timesteps || !alpha_t || !alpha_prev || samples <= 0 || n_steps <= 0)
    return fail(LATTE_ERR_INVALID, "t2v_guided_ddim_loop: bad arguments");
  return t2v_ddim_chain("t2v_guided_ddim_loop", e, x, samples, n_steps, timesteps, alpha_t, alpha_prev, guidance_scale, nullptr, nullptr,
                        nullptr, enable_temporal_attentions, (hipStream_t)stream);
}

// The guided DDIM loop with the known part of x replaced at the level each step reaches (include/latte_amd.h)
int latte_t2v_guided_ddim_loop_known(latte_t2v_t* e, float* x, int samples, int n_steps, const int64_t* timesteps,
                                     const double* alpha_t, const double* alpha_prev, float guidance_scale, const float* known,
                                     const float* mask, const float* noise, int enable_temporal_attentions, void* stream) {
  const std::string who = "t2v_guided_ddim_loop_known";
  if (!e || !x || !timesteps || !alpha_t || !alpha_prev || samples <= 0 || n_steps <= 0) return fail(LATTE_ERR_INVALID, who + ": bad arguments");
  if (!known || !mask || !noise)
    return fail(LATTE_ERR_INVALID, who + ": known, mask and noise [n_steps, ...] are required (this engine draws no noise)");
  return t2v_ddim_chain(who, e, x, samples, n_steps, timesteps, alpha_t, alpha_prev, guidance_scale, known, mask, noise,
                        enable_temporal_attentions, (hipStream_t)stream);
}

// latte_t2v_guided_linear_loop, and latte_t2v_guided_linear_loop_windows (`ws`: x and the noise rows have ws->L frames)
static int t2v_linear_chain(const std::string& who, latte_t2v* e, float* x, int samples, int n_evals, const double* plan, const float* noise,
                            float guidance_scale, int enable_temporal_attentions, hipStream_t st, const WindowSet* ws) {
  if (!e || !x || !plan || samples <= 0 || n_evals <= 0) return fail(LATTE_ERR_INVALID, who + ": bad arguments");
  int rc = t2v_chain_check(who, e, samples, ws);
  if (rc) return rc;
  const auto& c = e->cfg;
  PlanInfo info;   // no trained-range bound, and this engine draws no noise of its own
  if ((rc = plan_check(who.c_str(), plan, n_evals, e->tsteps_cap, 0, noise != nullptr, false, &info))) return rc;
  if ((rc = t2v_upload_timesteps(e, info.ts.data(), n_evals, st))) return rc;
  const int HW = e->H * e->H, frames = ws ? ws->L : e->F;
  const size_t per_chain = (size_t)samples * c.in_channels * frames * HW;   // <= max_batch / 2 latents: the ring and x_scaled hold it
  // what the denoiser reads: x itself when every in_scale is 1, else in_scale * x kept beside it by the step kernel
  float* x_in = info.scaled ? e->x_scaled : x;
  if (info.scaled) {
    LATTE_HIP(hipMemcpyAsync(x_in, x, sizeof(float) * per_chain, hipMemcpyDeviceToDevice, st));
    if ((rc = launch_scale_f32(x_in, (float)plan[P_IN], per_chain, st))) return rc;
  }
  HistRing ring{{e->hist[0], e->hist[1], e->hist[2]}};
  for (int k = 0; k < n_evals; ++k) {
    const float* mo;
    if ((rc = t2v_chain_forward(e, ws, x_in, e->tsteps + k, samples, enable_temporal_attentions, st, &mo))) return rc;
    const LinearStep s = plan_step(plan, k, n_evals, guidance_scale);
    if ((rc = launch_t2v_guided_linear_step(x, k + 1 == n_evals ? x : x_in, mo, ring.h1(), ring.h2(), ring.h3(),
                                            noise ? noise + (size_t)k * per_chain : nullptr, ring.write(), samples, c.in_channels,
                                            c.out_channels, frames, HW, s, st))) return rc;
    if (s.push) ring.push();
  }
  return LATTE_OK;
}

int latte_t2v_guided_linear_loop(latte_t2v_t* e, float* x, int samples, int n_evals, const double* plan, const float* noise,
                                 float guidance_scale, int enable_temporal_attentions, void* stream) {
  return t2v_linear_chain("t2v_guided_linear_loop", e, x, samples, n_evals, plan, noise, guidance_scale, enable_temporal_attentions,
                          (hipStream_t)stream, nullptr);
}

// ---- overlapping temporal windows: the two guided loops on x [samples, C, total_frames, H, W] (include/latte_amd.h)
int latte_t2v_guided_ddim_loop_windows(latte_t2v_t* e, float* x, int samples, int n_steps, const int64_t* timesteps, const double* alpha_t,
                                       const double* alpha_prev, float guidance_scale, int enable_temporal_attentions, int total_frames,
                                       int stride, void* stream) {
  if (!e || !x || !timesteps || !alpha_t || !alpha_prev || samples <= 0 || n_steps <= 0)
    return fail(LATTE_ERR_INVALID, "t2v_guided_ddim_loop_windows: bad arguments");
  const WindowSet ws{total_frames, e->F, stride};
  return t2v_ddim_chain("t2v_guided_ddim_loop_windows", e, x, samples, n_steps, timesteps, alpha_t, alpha_prev, guidance_scale, nullptr,
                        nullptr, nullptr, enable_temporal_attentions, (hipStream_t)stream, &ws);
}

int latte_t2v_guided_linear_loop_windows(latte_t2v_t* e, float* x, int samples, int n_evals, const double* plan, const float* noise,
                                         float guidance_scale, int enable_temporal_attentions, int total_frames, int stride, void* stream) {
  if (!e) return fail(LATTE_ERR_INVALID, "t2v_guided_linear_loop_windows: bad arguments");
  const WindowSet ws{total_frames, e->F, stride};
  return t2v_linear_chain("t2v_guided_linear_loop_windows", e, x, samples, n_evals, plan, noise, guidance_scale,
                          enable_temporal_attentions, (hipStream_t)stream, &ws);
}

}  // extern "C"
