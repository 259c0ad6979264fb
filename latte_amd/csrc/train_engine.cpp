// Training step on the engine (round 2): forward with saved activations, backward, AdamW + EMA.
//
//   train.py:197-236       x_t = q_sample(x_0, t), loss = training_losses(model, x_0, t)["loss"].mean(); loss.backward();
//                          clip_grad_norm_; opt.step(); update_ema
//   gaussian_diffusion.py:719-795   MSE on the mean head, variational bound on the variance head (mean detached)
//   latte.py:177-181,314-377        the block and the forward whose backward this is
//
// Layout: the same canonical token order as the inference engine (row = (b F + f) T + t); parameters, gradients and the
// optimiser state live in caller-owned FLAT fp32 buffers (reference named_parameters() order without the two frozen sin-cos
// tables; the host shim makes the nn.Parameters views of the parameter buffer and all-reduces the gradient buffer over RCCL).
// MFMA operands are half copies of the masters ([N, K] for the forward / weight-gradient GEMMs, [K, N] for the
// input-gradient GEMMs), re-packed after every optimiser step.  Saved per block: the two fp32 residual inputs of its LayerNorms
// and the half tensors xn1, qkv, attention output, y1, xn2, u (pre-GELU), h, y2.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "weight_store.h"

using namespace latte;

namespace {
struct ParamInfo {
  std::string key;
  int64_t offset, numel;
};
// Offsets of the trained tensors inside the flat buffers, resolved once while latte_trainer_create_joint adds the keys
struct BlockParams { int64_t qkv_w, qkv_b, proj_w, proj_b, fc1_w, fc1_b, fc2_w, fc2_b, ada_w, ada_b; };
struct RestParams { int64_t pe_w, pe_b, t0_w, t0_b, t2_w, t2_b, y_table /* -1: no label table */, fin_w, fin_b, fin_ada_w, fin_ada_b; };
struct BlockBuf {
  half_t *xn1, *qkv, *att, *y1, *xn2, *u, *h, *y2;
  half_t *qkv_w, *qkv_wt, *proj_w, *proj_wt, *fc1_w, *fc1_wt, *fc2_w, *fc2_wt;
};
// A flat table of trained tensors and the caller-owned fp32 buffers it lays out: the base (reference named_parameters() order) or the
// LoRA adapters.  block_begin[i]: where block i's tensors begin, block_begin[depth]: where the tensors behind the blocks do -- the
// boundaries of the backward stages' gradient slices (latte_trainer_stage_range).
struct TrainedSet {
  std::vector<ParamInfo> table;
  std::vector<int64_t> block_begin;
  int64_t total = 0;
  float *p = nullptr, *g = nullptr, *m1 = nullptr, *v2 = nullptr, *ema = nullptr;
  // -> the offset the tensor got
  int64_t add(const std::string& key, int64_t numel) {
    const int64_t off = total;
    table.push_back(ParamInfo{key, off, numel});
    total += (numel + 3) / 4 * 4;   // 16-byte aligned tensors inside the flat buffers
    return off;
  }
  void bind(float* p_, float* g_, float* m1_, float* v2_, float* ema_) { p = p_; g = g_; m1 = m1_; v2 = v2_; ema = ema_; }
  const ParamInfo* entry(int i) const { return i >= 0 && i < (int)table.size() ? &table[i] : nullptr; }
};
// LoRA: where a block's adapters lie in the flat adapter buffers (-1: the linear is not targeted), linear j = qkv, proj, fc1, fc2
struct LoraOffsets { int64_t a[4], b[4]; };
const char* const LORA_LINEAR[4] = {"attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2"};
// a gradient writer of the frozen base was reached in LoRA mode (G() below): the stage ends with LATTE_ERR_STATE before its launch
struct FrozenBaseWrite {};
}  // namespace

struct latte_trainer {
  latte_model_config_t cfg;
  int max_batch = 0;
  int D = 0, T = 0, F = 0, G = 0, Cin = 0, Cout = 0, H = 0, P = 0, KPE = 0, Hm = 0, hd = 0, nmod = 0, dt = 0;
  int64_t rows_max = 0, rows_pad = 0, ld = 0;
  // Loss scaling (f16 operands): d loss / d model_output is multiplied by loss_scale before the backward and every finished slice
  // of the gradient buffer by 1 / loss_scale -- the backward is linear in that seed, the scale is a power of two, so the result is
  // the unscaled gradient exactly unless something leaves f16's range.  Per-token gradients of this model are 1e-7 ... 1e-4
  // (Latte-B/2, batch 5): x 2^14 puts them at 1.6e-3 ... 1.6, inside f16's normal range (6e-5 ... 65504).  bf16: 1 (fp32's range).
  // Round 4: the scale lives in DEVICE memory (`scaler`, float[8], layout at gradnorm_finalize_kernel in train.hip) so that the
  // optimiser step can react to an overflow without a host round trip: a non-finite gradient norm SKIPS the update (parameters,
  // AdamW moments, EMA untouched) and, with dynamic scaling (the f16 default), halves the scale; 2000 applied updates in a row double
  // it again (cap 2^16 -- the largest of the three scales validated bit-exact in tests/test_training_step.py).  The same array
  // counts the APPLIED updates: AdamW's bias-correction step is that count (a fresh optimiser state starts at 1 whatever the
  // training-step counter of a continued run says; torch.optim.AdamW keeps its own count too).
  float loss_scale = 1.0f;       // initial / static value (host copy; the live value is scaler[0])
  int dynamic_scale = 0;
  int fuse_gelu = 1;        // the MLP's GELU passes inside the fc1 forward / fc2 input-gradient GEMMs (round 6; "fuse_gelu" option, A/B tests)
  // round 6b ("fuse_small" option, default 1; train_fin.hip): one finalize launch per block stage instead of ~25 tiny ones -- the
  // row-run / column partials of a stage stay in their own buffers until its end, the adaLN linear's input gradient is one batched
  // product at the last stage, the loss-scale pass of the block slices rides on the kernels that write them, one weight-pack launch
  int fuse_small = 1;
  // Gradient accumulation ("grad_accumulate" / "loss_divisor" options).  grad_accumulate = 1: every kernel that writes into the bound
  // gradient buffer ADDS to what is there, in its own store -- no second pass, no scratch copy.  Loss scaling needs nothing new: each
  // micro-batch is unscaled by the CURRENT scale as it is written (in accumulate mode by the writing kernels themselves -- the
  // per-stage scale pass of the assign mode would rescale the earlier micro-batches' sum -- x 1 / scale, a power of two: the same
  // bits), the scale changes only inside the optimiser step, and a non-finite value of any micro-batch survives the sum, so the
  // existing rule applies unchanged: a non-finite gradient norm skips the update and halves the scale.
  int grad_accumulate = 0;
  float loss_divisor = 1.0f;     // d loss.mean() / loss_divisor (train.py:222 `loss / gradient_accumulation_steps`); terms stay undivided
  float *pg1 = nullptr, *pl1 = nullptr, *pg2 = nullptr, *pg2b = nullptr, *pl2 = nullptr, *pc_fc1 = nullptr, *pc_qkv = nullptr, *dc_ws = nullptr, *no_ws = nullptr;
  PackDesc* pack_descs = nullptr;
  std::vector<PackDesc> pack_host;   // [block][qkv, proj, fc1, fc2]: the host copy of pack_descs (latte_trainer_bind)
  PackPlan pack_plan{};
  float growth_interval = 2000.0f;
  float* scaler = nullptr;
  // The model's own tensors and, under LoRA, the adapters; the optimiser trains ONE of them (trained() below).  A third kind of
  // trained tensor is a third set here: its table built through add(), its buffers bound, trained() told when it is the one
  TrainedSet base, adapters;
  std::vector<BlockParams> bp;   // + rp: where every tensor of the base lies in its flat buffers
  RestParams rp{};
  float *pos = nullptr, *temp = nullptr, *pe_wt = nullptr, *fin_wt = nullptr;
  std::vector<float*> xs;        // 2 depth + 1 residual-stream snapshots, fp32 [rows_pad, D]
  std::vector<BlockBuf> blk;
  // conditioning
  float *tfreq = nullptr, *temb_pre = nullptr, *temb_act = nullptr, *cvec = nullptr, *csilu = nullptr, *mod = nullptr, *dmod = nullptr,
        *dc = nullptr, *dtmp = nullptr, *dtmp2 = nullptr;
  int64_t* t_orig = nullptr;
  int64_t* tmap_dev = nullptr;
  int tmap_n = 0;
  const latte_schedule_t* tmap_of = nullptr;
  // scratch
  float *x_t = nullptr, *model_out = nullptr, *dmodel_out = nullptr, *dtok = nullptr, *f32a = nullptr, *f32b = nullptr, *dx = nullptr,
        *pix = nullptr, *ones = nullptr, *zeros = nullptr, *part_rows = nullptr, *part_cols = nullptr, *wg_ws = nullptr, *ng_ws = nullptr,
        *attn_stats = nullptr, *loss_ws = nullptr, *stats = nullptr;
  double* sumsq = nullptr;
  half_t *dyD = nullptr, *dhH = nullptr, *dxnH = nullptr, *dqkvH = nullptr, *xnh = nullptr;
  int64_t wg_ws_floats = 0, ng_ws_floats = 0, loss_ws_floats = 0;
  bool weights_synced = false;
  // Joint image-video micro-batch (latte_trainer_begin_joint; train_with_img.py:214-241, latte_img.py:361-399).  The image frames of a
  // sample never meet its video frames (spatial blocks treat every frame alone, temporal blocks see x[:, :F] only) and mean_flat runs
  // over all F + N frames, so loss.mean() = F / (F + N) mean_b(loss_video_b) + N / (F + N) mean_{b,n}(loss_image_{b,n}): the step is the
  // video pass below plus an image pass over B N one-frame pseudo-samples in spatial-only mode.  The RUN MODE of a pass: frames per
  // sample (run_F), temporal blocks on / off (off: odd blocks skipped in the forward and in their backward stage, no temp_embed,
  // the xs[] / xn1 chain follows the even blocks), and the pass's loss weight (multiplies loss_divisor).
  int max_image = 0;
  int run_F = 0, run_temporal = 1;
  float run_weight = 1.0f;
  int joint_saved_acc = -1;      // >= 0: an image pass is in flight (always in accumulate mode); the caller's grad_accumulate, restored after its last stage
  float *jx_v = nullptr, *jn_v = nullptr, *jx_i = nullptr, *jn_i = nullptr, *jmo = nullptr, *jterms = nullptr;
  int64_t* jt_i = nullptr;
  int cur_batch = 0, next_stage = 1 << 30;   // step in flight: batch, labels (caller keeps them alive), next backward stage
  const int64_t* cur_y = nullptr;
  // Custom loss (latte_trainer_forward / _seed / _input_grad): 0 = no custom pass, 1 = forward done, awaiting the caller's seed,
  // 2 = seeded (its stages run, or have run: the token gradient e->dx of the last one is what latte_trainer_input_grad reads)
  int custom = 0, fwd_batch = 0;
  const int64_t* fwd_y = nullptr;
  // LoRA (latte_trainer_lora_enable; train_lora.hip): the base buffer is frozen -- no base gradient, moment or EMA buffer
  // is bound, every base-gradient writer is skipped -- and rank-r adapters on the targeted block linears train instead.  The half operand
  // copies hold W + s B A (the pack adds it), so the forward and the input-gradient GEMMs are the plain trainer's launches; linear_bwd
  // replaces the weight-gradient GEMM by the adapter gradients.  The `adapters` set lays them out; lo: per block, per linear.
  int lora_rank = 0, lora_mask = 0;
  float lora_s = 0.f;
  std::vector<LoraOffsets> lo;
  std::vector<LoraPackDesc> lora_host;   // [block][qkv, proj, fc1, fc2]
  LoraPackDesc *lora_descs = nullptr, *lora_merge_descs = nullptr;
  half_t *lora_h = nullptr, *lora_g = nullptr;   // [rows_pad, 2 R16]: s x A^T and s dY B of the linear in hand, as split pairs hi | lo
  DeviceArena arena;
};

namespace {

int64_t add_param(latte_trainer* e, const std::string& key, int64_t numel) { return e->base.add(key, numel); }
// the set the optimiser trains: the adapters under LoRA (the base is frozen), the base otherwise
const TrainedSet& trained(const latte_trainer* e) { return e->lora_rank ? e->adapters : e->base; }
// the bodies of the two accessor families (latte_trainer_param_* / latte_trainer_lora_param_*): s = the family's set, NULL without a trainer
int set_size(const TrainedSet* s) { return s ? (int)s->table.size() : 0; }
const char* set_key(const TrainedSet* s, int i) { return s && s->entry(i) ? s->entry(i)->key.c_str() : nullptr; }
int64_t set_offset(const TrainedSet* s, int i) { return s && s->entry(i) ? s->entry(i)->offset : -1; }
int64_t set_numel(const TrainedSet* s, int i) { return s && s->entry(i) ? s->entry(i)->numel : -1; }
int64_t set_total(const TrainedSet* s) { return s ? s->total : 0; }
const TrainedSet* base_of(const latte_trainer* e) { return e ? &e->base : nullptr; }
const TrainedSet* adapters_of(const latte_trainer* e) { return e ? &e->adapters : nullptr; }

// ---- LoRA: what latte_trainer_lora_enable accepts, and the adapter table (host logic: latte_debug_lora_table reads it without a device)
int lora_validate(int rank, float alpha, int target_mask) {
  // rank 64: the kernels take it (train_lora.hip, tested per element), the trainer does not -- at Latte-B/2, batch 5 its step measured
  // slower than the full step it replaces (18.41 against 17.93 ms, profiles/train_lora.json); it comes back with the fused dY pass
  if (rank == 64)
    return fail(LATTE_ERR_INVALID, "lora_enable: rank 64 is not offered: its step is slower than full fine-tuning at Latte-B/2 (DESIGN 4.4); rank must be one of 4, 8, 16, 32");
  if (rank != 4 && rank != 8 && rank != 16 && rank != 32)
    return fail(LATTE_ERR_INVALID, "lora_enable: rank must be one of 4, 8, 16, 32");
  if (target_mask < 1 || target_mask > 15)
    return fail(LATTE_ERR_INVALID, "lora_enable: target_mask must be a non-empty subset of qkv = 1, proj = 2, fc1 = 4, fc2 = 8");
  if (!(alpha > 0.0f) || !std::isfinite(alpha)) return fail(LATTE_ERR_INVALID, "lora_enable: alpha must be positive and finite");
  return LATTE_OK;
}
void lora_shape(int D, int Hm, int j, int* N, int* K) {   // W [N, K] of linear j
  const int shp[4][2] = {{3 * D, D}, {D, D}, {Hm, D}, {D, Hm}};
  *N = shp[j][0]; *K = shp[j][1];
}
// block-major, per block qkv, proj, fc1, fc2 (the targeted ones), per linear lora_A [rank, K] then lora_B [N, rank]
void lora_table(int D, int Hm, int depth, int rank, int target_mask, TrainedSet& set, std::vector<LoraOffsets>& lo) {
  lo.assign((size_t)depth, LoraOffsets{});
  for (int i = 0; i < depth; ++i) {
    set.block_begin.push_back(set.total);
    for (int j = 0; j < 4; ++j) {
      lo[i].a[j] = lo[i].b[j] = -1;
      if (!(target_mask >> j & 1)) continue;
      int N, K;
      lora_shape(D, Hm, j, &N, &K);
      const std::string p = "blocks." + std::to_string(i) + "." + LORA_LINEAR[j];
      lo[i].a[j] = set.add(p + ".lora_A", (int64_t)rank * K);
      lo[i].b[j] = set.add(p + ".lora_B", (int64_t)N * rank);
    }
  }
  set.block_begin.push_back(set.total);   // nothing lies behind the blocks
}

float* P(const latte_trainer* e, int64_t off) { return e->base.p + off; }
float* G(const latte_trainer* e, int64_t off) {
  if (e->lora_rank || !e->base.g) throw FrozenBaseWrite{};   // LoRA: there is no base gradient buffer (latte_trainer_backward_stage catches)
  return e->base.g + off;
}
// a step is in flight: begin / seed ran and a backward stage is still due
bool step_in_flight(const latte_trainer* e) { return e->next_stage <= e->cfg.depth + 1; }
bool pow2_in(double v, double lo, double hi) {
  int ex = 0;
  return v >= lo && v <= hi && std::frexp(v, &ex) == 0.5;
}
int gemm_half(latte_trainer* e, const half_t* A, const half_t* W, const float* bias, half_t* out, int M, int N, int K, hipStream_t st) {
  GemmArgs g{};
  g.A = A; g.W = W; g.bias = bias; g.out = out; g.M = M; g.N = N; g.K = K; g.rows_per_sample = M; g.gate_stride = 0;
  return launch_gemm(g, EPI_BIAS_H16, e->dt, 0, st);
}

// The rolling 12-wave kernel's training epilogues (gemm_pw.hip: EPI_BIAS_GELU_DUAL_H16 / EPI_DGELU_H16) take the shape
bool gelu_fusable(const latte_trainer* e, int M, int N, int K) {
  return e->fuse_gelu && N % 192 == 0 && K % 64 == 0 && K >= 128 && (uint64_t)((M + 255) / 256 * 256) * K * 2 < (1ull << 32) &&
         (uint64_t)N * K * 2 < (1ull << 32);
}
// out = A W^T + bias with the GELU pass fused: epi EPI_BIAS_GELU_DUAL_H16 (out = u, aux = gelu(u)) or EPI_DGELU_H16 (out = (A W^T) gelu'(aux))
int gemm_gelu(latte_trainer* e, int epi, const half_t* A, const half_t* W, const float* bias, half_t* out, half_t* aux, int M, int N, int K,
              hipStream_t st) {
  GemmArgs g{};
  g.A = A; g.W = W; g.bias = bias; g.out = out; g.aux = aux; g.M = M; g.N = N; g.K = K; g.rows_per_sample = M; g.gate_stride = 0;
  return launch_gemm_pw(g, epi, e->dt, 1, st);
}

bool scaling_active(const latte_trainer* e) { return e->loss_scale != 1.0f || e->dynamic_scale; }
// accumulate mode: the gradient writers unscale what they add themselves (device loss scale), nullptr otherwise
const float* acc_scale(const latte_trainer* e) { return e->grad_accumulate && scaling_active(e) ? e->scaler : nullptr; }
// dW[N, K] = dY[M, N]^T X[M, K] on the transposed-operand GEMM (gemm_tn.hip: no transposed copies), the contraction split so
// that about four workgroups per CU are in flight; the partial products are reduced in a fixed order; result ASSIGNED to dW
// ("grad_accumulate": ADDED by the reduction's own store, unscaled there)
// (unscale: the reduction also takes the result out of the loss-scaled domain, x 1 / scaler[0])
// cs_partial / cs_rows: the column sums of dY per split ([*cs_rows][N]: the bias gradient's partial rows) ride on the launch
int wgrad(latte_trainer* e, const half_t* dY, const half_t* X, int M, int N, int K, float* dW, hipStream_t st, bool unscale = false,
          float* cs_partial = nullptr, int* cs_rows = nullptr) {
  int rc, chunk = 0;
  const int splits = gemm_tn_plan(M, N, K, &chunk);
  if ((int64_t)splits * N * K > e->wg_ws_floats) return fail(LATTE_ERR_STATE, "wgrad: workspace too small");
  if (cs_rows) *cs_rows = splits;
  if ((rc = launch_gemm_tn(dY, X, e->wg_ws, M, N, K, chunk, e->dt, st, cs_partial))) return rc;
  return launch_split_reduce(e->wg_ws, splits, (size_t)N * K, (size_t)N * K, dW, e->grad_accumulate, st,
                             unscale ? e->scaler : acc_scale(e));
}

// loss-scale state -> device.  what: 0 = everything incl. the counters (create), 1 = a new scale (restarts the growth count),
// 2 = the policy fields only (dynamic on / off, growth interval): the live scale and the counters stay.  Synchronous (an option
// call, not on the step path).
int upload_scaler(latte_trainer* e, int what) {
  float h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (what != 0) {
    LATTE_HIP(hipDeviceSynchronize());
    LATTE_HIP(hipMemcpy(h, e->scaler, sizeof(h), hipMemcpyDeviceToHost));
  }
  if (what != 2) {
    h[0] = e->loss_scale;
    h[1] = 0.0f;
  }
  h[5] = (float)e->dynamic_scale;
  h[6] = e->growth_interval;
  h[7] = std::max(std::max(e->loss_scale, h[0]), 65536.0f);
  LATTE_HIP(hipMemcpy(e->scaler, h, sizeof(h), hipMemcpyHostToDevice));
  return LATTE_OK;
}

}  // namespace

extern "C" {

int latte_trainer_create(const latte_model_config_t* cfg, int max_batch, latte_trainer_t** out) {
  return latte_trainer_create_joint(cfg, max_batch, 0, out);
}

// max_image_num > 0: the per-sample buffers hold max_batch * max_image_num pseudo-samples of the image pass (the row buffers already
// do: B N T <= B F T), plus the packed regions of the joint micro-batch
int latte_trainer_create_joint(const latte_model_config_t* cfg, int max_batch, int max_image_num, latte_trainer_t** out) {
  if (!cfg || !out || max_batch <= 0 || max_image_num < 0) return fail(LATTE_ERR_INVALID, "trainer_create: bad arguments");
  if (max_image_num > cfg->num_frames)
    return fail(LATTE_ERR_INVALID, "trainer: use_image_num must not exceed num_frames (the image pass runs in the video pass's row buffers)");
  const auto& c = *cfg;
  if (c.extras != 1 && c.extras != 2) return fail(LATTE_ERR_INVALID, "trainer: extras must be 1 or 2 (train.py:213-218 refuses text-to-video training)");
  if (c.hidden_size % 128 || c.hidden_size > 1280 || c.depth < 2 || c.depth % 2 || c.hidden_size % c.num_heads)   // (bp[0], bp[1] exist)
    return fail(LATTE_ERR_INVALID, "trainer: hidden_size must be a multiple of 128 (<= 1280), depth even");
  const int hd = c.hidden_size / c.num_heads;
  if (hd != 64 && hd != 72) return fail(LATTE_ERR_INVALID, "trainer: head dim must be 64 or 72");
  if (c.mlp_hidden % 128) return fail(LATTE_ERR_INVALID, "trainer: mlp_hidden must be a multiple of 128");
  if (c.input_size % c.patch_size) return fail(LATTE_ERR_INVALID, "trainer: input_size % patch_size != 0");
  auto* e = new latte_trainer();
  e->cfg = c;
  e->max_batch = max_batch;
  e->max_image = max_image_num;
  e->run_F = c.num_frames;
  e->D = c.hidden_size; e->F = c.num_frames; e->G = c.input_size / c.patch_size; e->T = e->G * e->G;
  e->Cin = c.in_channels; e->Cout = c.learn_sigma ? 2 * c.in_channels : c.in_channels; e->H = c.input_size;
  e->P = c.patch_size * c.patch_size * e->Cout; e->KPE = c.in_channels * c.patch_size * c.patch_size;
  e->Hm = c.mlp_hidden; e->hd = hd; e->dt = c.compute_dtype;
  e->loss_scale = c.compute_dtype == LATTE_DTYPE_F16 ? 16384.0f : 1.0f;
  e->dynamic_scale = c.compute_dtype == LATTE_DTYPE_F16 ? 1 : 0;
  e->nmod = c.depth * 6 * e->D + 2 * e->D;
  if ((e->F * e->T) % 64) { delete e; return fail(LATTE_ERR_INVALID, "trainer: frames * tokens per sample must be a multiple of 64"); }
  if (max_image_num > 0 && e->T % 64) {
    delete e;
    return fail(LATTE_ERR_INVALID, "trainer: joint image-video training needs tokens per frame to be a multiple of 64 (an image is a sample of one frame)");
  }
  e->rows_max = (int64_t)max_batch * e->F * e->T;
  e->rows_pad = (e->rows_max + 255) / 256 * 256;
  e->ld = (e->rows_max + 63) / 64 * 64;
  const int D = e->D, Hm = e->Hm;
  // ---- parameter table: reference named_parameters() order (latte.py:226-255), frozen tables excluded
  RestParams& r = e->rp;
  r.pe_w = add_param(e, "x_embedder.proj.weight", (int64_t)D * e->KPE);
  r.pe_b = add_param(e, "x_embedder.proj.bias", D);
  r.t0_w = add_param(e, "t_embedder.mlp.0.weight", (int64_t)D * 256);
  r.t0_b = add_param(e, "t_embedder.mlp.0.bias", D);
  r.t2_w = add_param(e, "t_embedder.mlp.2.weight", (int64_t)D * D);
  r.t2_b = add_param(e, "t_embedder.mlp.2.bias", D);
  r.y_table = c.extras == 2 ? add_param(e, "y_embedder.embedding_table.weight", (int64_t)(c.num_classes + 1) * D) : -1;
  e->bp.resize(c.depth);
  for (int i = 0; i < c.depth; ++i) {
    const std::string p = "blocks." + std::to_string(i) + ".";
    BlockParams& w = e->bp[i];
    e->base.block_begin.push_back(e->base.total);
    w.qkv_w = add_param(e, p + "attn.qkv.weight", (int64_t)3 * D * D);
    w.qkv_b = add_param(e, p + "attn.qkv.bias", 3 * D);
    w.proj_w = add_param(e, p + "attn.proj.weight", (int64_t)D * D);
    w.proj_b = add_param(e, p + "attn.proj.bias", D);
    w.fc1_w = add_param(e, p + "mlp.fc1.weight", (int64_t)Hm * D);
    w.fc1_b = add_param(e, p + "mlp.fc1.bias", Hm);
    w.fc2_w = add_param(e, p + "mlp.fc2.weight", (int64_t)D * Hm);
    w.fc2_b = add_param(e, p + "mlp.fc2.bias", D);
    w.ada_w = add_param(e, p + "adaLN_modulation.1.weight", (int64_t)6 * D * D);
    w.ada_b = add_param(e, p + "adaLN_modulation.1.bias", 6 * D);
  }
  e->base.block_begin.push_back(e->base.total);   // the final layer lies behind the blocks
  r.fin_w = add_param(e, "final_layer.linear.weight", (int64_t)e->P * D);
  r.fin_b = add_param(e, "final_layer.linear.bias", e->P);
  r.fin_ada_w = add_param(e, "final_layer.adaLN_modulation.1.weight", (int64_t)2 * D * D);
  r.fin_ada_b = add_param(e, "final_layer.adaLN_modulation.1.bias", 2 * D);

  int rc = LATTE_OK;
  const size_t R = (size_t)e->rows_pad;
  auto A = [&](auto** p, size_t n) { if (!rc) rc = e->arena.alloc(p, n); };
  A(&e->pos, (size_t)e->T * D); A(&e->temp, (size_t)e->F * D); A(&e->pe_wt, (size_t)e->KPE * D); A(&e->fin_wt, (size_t)D * e->P);
  e->xs.resize(2 * c.depth + 1);
  for (auto& x : e->xs) A(&x, R * D);
  e->blk.resize(c.depth);
  for (auto& b : e->blk) {
    A(&b.xn1, R * D); A(&b.qkv, R * 3 * D); A(&b.att, R * D); A(&b.y1, R * D); A(&b.xn2, R * D); A(&b.u, R * Hm); A(&b.h, R * Hm);
    A(&b.y2, R * D);
    A(&b.qkv_w, (size_t)3 * D * D); A(&b.qkv_wt, (size_t)3 * D * D); A(&b.proj_w, (size_t)D * D); A(&b.proj_wt, (size_t)D * D);
    A(&b.fc1_w, (size_t)Hm * D); A(&b.fc1_wt, (size_t)Hm * D); A(&b.fc2_w, (size_t)Hm * D); A(&b.fc2_wt, (size_t)Hm * D);
  }
  const size_t Bm = (size_t)max_batch * std::max(1, max_image_num);   // samples of a pass: the image pass has batch * use_image_num
  A(&e->tfreq, Bm * 256); A(&e->temb_pre, Bm * D); A(&e->temb_act, Bm * D); A(&e->cvec, Bm * D); A(&e->csilu, Bm * D);
  A(&e->mod, Bm * e->nmod); A(&e->dmod, Bm * e->nmod); A(&e->dc, Bm * D); A(&e->dtmp, Bm * D); A(&e->dtmp2, Bm * D);
  A(&e->t_orig, Bm);
  const size_t lat = Bm * e->F * e->H * e->H;
  A(&e->x_t, lat * e->Cin); A(&e->model_out, lat * e->Cout); A(&e->dmodel_out, lat * e->Cout);
  A(&e->dtok, R * e->P); A(&e->f32a, R * D); A(&e->f32b, R * D); A(&e->dx, R * D); A(&e->pix, R * e->KPE);
  A(&e->ones, R); A(&e->zeros, (size_t)std::max(Hm, 3 * D) + 256);
  const int Rr = train_rows_per_run(e->F * e->T);
  A(&e->part_rows, (size_t)(e->rows_max / Rr + 4) * 2 * D);
  A(&e->part_cols, (size_t)(colsum_chunks((int)e->rows_max) + 1) * std::max(Hm, 3 * D));
  {
    const size_t pr = (size_t)(e->rows_max / Rr / 4 + 1) * 2 * D;   // one block of 4 runs -> 2 partial rows
    A(&e->pg1, pr); A(&e->pl1, pr); A(&e->pg2, pr); A(&e->pg2b, pr); A(&e->pl2, pr);
    const size_t pcr = (size_t)std::max(colsum_chunks((int)e->rows_max) + 1, 260);   // column-sum chunks or weight-gradient splits (<= 256)
    A(&e->pc_fc1, pcr * Hm);
    A(&e->pc_qkv, pcr * 3 * D);
    A(&e->dc_ws, (size_t)adaln_dc_splits(e->nmod) * Bm * D);
    A(&e->no_ws, (size_t)narrow_blocks((int)e->rows_max) * ((size_t)32 * D + 32 + D));
    A(&e->pack_descs, (size_t)c.depth * 4);
    const int shp[4][2] = {{3 * D, D}, {D, D}, {Hm, D}, {D, Hm}};
    int t0 = 0;
    for (int j = 0; j < 4; ++j) {
      e->pack_plan.tile0[j] = t0;
      t0 += ((shp[j][0] + 31) / 32) * ((shp[j][1] + 31) / 32);
    }
    e->pack_plan.tiles_per_block = t0;
  }
  {
    // split-K partial products: splits * N * K with splits <= ceil(1024 / tiles) (+1), tiles = ceil(N / 128) (K / 128)
    int64_t worst = 0;
    const int shapes[4][2] = {{3 * D, D}, {D, D}, {Hm, D}, {D, Hm}};
    for (auto& s : shapes) {
      const int tiles = ((s[0] + 255) / 256) * (s[1] / 128);
      const int64_t splits = std::min<int64_t>(e->ld / 64 + 1, (768 + tiles - 1) / tiles) + 1;
      worst = std::max<int64_t>(worst, splits * s[0] * s[1]);
    }
    e->wg_ws_floats = worst;
    A(&e->wg_ws, (size_t)worst);
  }
  e->ng_ws_floats = 64LL * std::max<int64_t>((int64_t)e->P * D, (int64_t)Bm * D) + 64LL * D * e->KPE + 64LL * D;
  A(&e->ng_ws, (size_t)e->ng_ws_floats);
  A(&e->attn_stats, (size_t)e->rows_max * c.num_heads * 3 + 16);
  e->loss_ws_floats = std::max(latte_training_workspace_floats(max_batch, (int64_t)e->F * e->Cin * e->H * e->H),
                               latte_training_workspace_floats((int)Bm, (int64_t)e->Cin * e->H * e->H)) + 3 * max_batch;
  A(&e->loss_ws, (size_t)e->loss_ws_floats);
  if (max_image_num > 0) {
    const size_t per = (size_t)e->Cin * e->H * e->H, mb = (size_t)max_batch;
    A(&e->jx_v, mb * e->F * per); A(&e->jn_v, mb * e->F * per); A(&e->jx_i, Bm * per); A(&e->jn_i, Bm * per);
    A(&e->jmo, mb * e->F * e->Cout * e->H * e->H); A(&e->jterms, 3 * mb + 3 * Bm); A(&e->jt_i, Bm);
  }
  A(&e->stats, 4);
  A(&e->scaler, 8);
  A(&e->sumsq, (size_t)sumsq_blocks());
  A(&e->dyD, R * D); A(&e->dhH, R * Hm); A(&e->dxnH, R * D); A(&e->dqkvH, R * 3 * D); A(&e->xnh, R * D);
  if (!rc) rc = launch_fill_f32(e->ones, 1.0f, R, nullptr);
  if (!rc) rc = upload_scaler(e, 0);
  if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(LATTE_ERR_HIP, "trainer_create: device error");
  if (rc) { latte_trainer_destroy(e); return rc; }
  *out = e;
  return LATTE_OK;
}

void latte_trainer_destroy(latte_trainer_t* e) {
  delete e;   // the arena frees every device block
}

int latte_trainer_num_params(const latte_trainer_t* e) { return set_size(base_of(e)); }
const char* latte_trainer_param_key(const latte_trainer_t* e, int i) { return set_key(base_of(e), i); }
int64_t latte_trainer_param_offset(const latte_trainer_t* e, int i) { return set_offset(base_of(e), i); }
int64_t latte_trainer_param_numel(const latte_trainer_t* e, int i) { return set_numel(base_of(e), i); }
int64_t latte_trainer_total_numel(const latte_trainer_t* e) { return set_total(base_of(e)); }
int latte_trainer_lora_num_params(const latte_trainer_t* e) { return set_size(adapters_of(e)); }
const char* latte_trainer_lora_param_key(const latte_trainer_t* e, int i) { return set_key(adapters_of(e), i); }
int64_t latte_trainer_lora_param_offset(const latte_trainer_t* e, int i) { return set_offset(adapters_of(e), i); }
int64_t latte_trainer_lora_param_numel(const latte_trainer_t* e, int i) { return set_numel(adapters_of(e), i); }
int64_t latte_trainer_lora_total_numel(const latte_trainer_t* e) { return set_total(adapters_of(e)); }

int latte_trainer_bind(latte_trainer_t* e, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* ema) {
  if (!e || !params || !grads || !exp_avg || !exp_avg_sq) return fail(LATTE_ERR_INVALID, "trainer_bind: null buffer");
  if (e->lora_rank) return fail(LATTE_ERR_STATE, "trainer_bind: LoRA is enabled, bind with latte_trainer_bind_lora");
  e->base.bind(params, grads, exp_avg, exp_avg_sq, ema);
  e->weights_synced = false;
  {   // pointer table of the one-launch weight pack (train_fin.hip): [block][qkv, proj, fc1, fc2]
    const int D = e->D, Hm = e->Hm;
    std::vector<PackDesc>& h = e->pack_host;
    h.resize((size_t)e->cfg.depth * 4);
    for (int i = 0; i < e->cfg.depth; ++i) {
      const BlockParams& w = e->bp[i];
      BlockBuf& b = e->blk[i];
      h[i * 4 + 0] = PackDesc{P(e, w.qkv_w), b.qkv_w, b.qkv_wt, 3 * D, D};
      h[i * 4 + 1] = PackDesc{P(e, w.proj_w), b.proj_w, b.proj_wt, D, D};
      h[i * 4 + 2] = PackDesc{P(e, w.fc1_w), b.fc1_w, b.fc1_wt, Hm, D};
      h[i * 4 + 3] = PackDesc{P(e, w.fc2_w), b.fc2_w, b.fc2_wt, D, Hm};
    }
    LATTE_HIP(hipDeviceSynchronize());
    LATTE_HIP(hipMemcpy(e->pack_descs, h.data(), h.size() * sizeof(PackDesc), hipMemcpyHostToDevice));
  }
  return LATTE_OK;
}

// ---- LoRA: enable (before bind), the adapter table, bind, merge
int latte_trainer_lora_enable(latte_trainer_t* e, int rank, float alpha, int target_mask) {
  if (!e) return fail(LATTE_ERR_INVALID, "lora_enable: null trainer");
  if (step_in_flight(e) || e->custom == 1) return fail(LATTE_ERR_STATE, "lora_enable: a step is in flight");
  if (e->base.p || e->lora_rank) return fail(LATTE_ERR_STATE, "lora_enable: legal once, before the buffers are bound");
  int rc;
  if ((rc = lora_validate(rank, alpha, target_mask))) return rc;
  const int D = e->D, Hm = e->Hm, depth = e->cfg.depth, R16 = (rank + 15) / 16 * 16;
  TrainedSet set;
  std::vector<LoraOffsets> lo;
  lora_table(D, Hm, depth, rank, target_mask, set, lo);
  std::vector<LoraPackDesc> host((size_t)depth * 4);
  auto A = [&](auto** p, size_t n) { if (!rc) rc = e->arena.alloc(p, n); };
  for (int i = 0; i < depth; ++i)
    for (int j = 0; j < 4; ++j) {
      LoraPackDesc& d = host[(size_t)i * 4 + j];
      d = LoraPackDesc{};
      lora_shape(D, Hm, j, &d.N, &d.K);
      if (lo[i].a[j] < 0) continue;
      A(&d.a_h, (size_t)R16 * d.K);
      A(&d.bt_h, (size_t)R16 * d.N);
    }
  A(&e->lora_h, (size_t)e->rows_pad * 2 * R16);   // split pairs [hi | lo]
  A(&e->lora_g, (size_t)e->rows_pad * 2 * R16);
  A(&e->lora_descs, (size_t)depth * 4);
  A(&e->lora_merge_descs, (size_t)depth * 4);
  if (rc) return rc;
  e->adapters = std::move(set);
  e->lo = std::move(lo);
  e->lora_host = std::move(host);
  e->lora_mask = target_mask;
  e->lora_s = alpha / (float)rank;
  e->lora_rank = rank;
  return LATTE_OK;
}

// Host logic only (include/latte_amd_debug.h): entry `index` of the adapter table a trainer of `cfg` would get
int latte_debug_lora_table(const latte_model_config_t* cfg, int rank, float alpha, int target_mask, int index, char* key_out, int key_cap,
                           int64_t* offset, int64_t* numel, int* num_params, int64_t* total) {
  if (!cfg || cfg->depth < 1 || cfg->hidden_size < 1 || cfg->mlp_hidden < 1) return fail(LATTE_ERR_INVALID, "lora_table: bad config");
  if (int rc = lora_validate(rank, alpha, target_mask)) return rc;
  TrainedSet set;
  std::vector<LoraOffsets> lo;
  lora_table(cfg->hidden_size, cfg->mlp_hidden, cfg->depth, rank, target_mask, set, lo);
  if (num_params) *num_params = set_size(&set);
  if (total) *total = set.total;
  if (index < 0) return LATTE_OK;   // the counts only
  const ParamInfo* p = set.entry(index);
  if (!p || !key_out || key_cap <= (int)p->key.size()) return fail(LATTE_ERR_INVALID, "lora_table: bad index or key buffer");
  std::copy(p->key.begin(), p->key.end(), key_out);
  key_out[p->key.size()] = 0;
  if (offset) *offset = p->offset;
  if (numel) *numel = p->numel;
  return LATTE_OK;
}

int latte_trainer_bind_lora(latte_trainer_t* e, float* base_params, float* lora_params, float* lora_grads, float* lora_exp_avg,
                            float* lora_exp_avg_sq, float* lora_ema) {
  if (!e || !base_params || !lora_params || !lora_grads || !lora_exp_avg || !lora_exp_avg_sq) return fail(LATTE_ERR_INVALID, "trainer_bind_lora: null buffer");
  if (!e->lora_rank) return fail(LATTE_ERR_STATE, "trainer_bind_lora: call latte_trainer_lora_enable first");
  if (step_in_flight(e) || e->custom == 1) return fail(LATTE_ERR_STATE, "trainer_bind_lora: a step is in flight");
  e->base.bind(base_params, nullptr, nullptr, nullptr, nullptr);
  e->adapters.bind(lora_params, lora_grads, lora_exp_avg, lora_exp_avg_sq, lora_ema);
  e->weights_synced = false;
  for (int i = 0; i < e->cfg.depth; ++i) {
    const BlockParams& w = e->bp[i];
    BlockBuf& b = e->blk[i];
    const int64_t wo[4] = {w.qkv_w, w.proj_w, w.fc1_w, w.fc2_w};
    half_t* const wn[4] = {b.qkv_w, b.proj_w, b.fc1_w, b.fc2_w};
    half_t* const wt[4] = {b.qkv_wt, b.proj_wt, b.fc1_wt, b.fc2_wt};
    for (int j = 0; j < 4; ++j) {
      LoraPackDesc& d = e->lora_host[(size_t)i * 4 + j];
      d.w = P(e, wo[j]); d.wn = wn[j]; d.wt = wt[j]; d.wf = nullptr;
      d.A = e->lo[i].a[j] >= 0 ? lora_params + e->lo[i].a[j] : nullptr;
      d.B = e->lo[i].b[j] >= 0 ? lora_params + e->lo[i].b[j] : nullptr;
    }
  }
  LATTE_HIP(hipDeviceSynchronize());
  LATTE_HIP(hipMemcpy(e->lora_descs, e->lora_host.data(), e->lora_host.size() * sizeof(LoraPackDesc), hipMemcpyHostToDevice));
  return LATTE_OK;
}

// params_out: a caller's copy of the flat base buffer (or the bound buffer itself: every element is read before it is written);
// lora_params: the adapters to merge (NULL: the bound ones; the EMA buffer merges the EMA adapters).  Synchronises.
int latte_trainer_lora_merge(latte_trainer_t* e, const float* lora_params, float* params_out, void* stream) {
  if (!e || !params_out) return fail(LATTE_ERR_INVALID, "lora_merge: null argument");
  if (!e->lora_rank || !e->base.p) return fail(LATTE_ERR_STATE, "lora_merge: bind the LoRA buffers first");
  if (step_in_flight(e)) return fail(LATTE_ERR_STATE, "lora_merge: a step is in flight");
  const float* lp = lora_params ? lora_params : e->adapters.p;
  std::vector<LoraPackDesc> h = e->lora_host;
  for (size_t li = 0; li < h.size(); ++li) {   // li = block * 4 + linear
    LoraPackDesc& d = h[li];
    const LoraOffsets& o = e->lo[li / 4];
    d.wf = params_out + (d.w - e->base.p);   // the same offset in the caller's copy of the base buffer
    d.wn = d.wt = nullptr;
    if (d.A) { d.A = lp + o.a[li % 4]; d.B = lp + o.b[li % 4]; }
  }
  LATTE_HIP(hipDeviceSynchronize());
  LATTE_HIP(hipMemcpy(e->lora_merge_descs, h.data(), h.size() * sizeof(LoraPackDesc), hipMemcpyHostToDevice));
  if (int rc = launch_pack_weights_lora(e->lora_merge_descs, e->cfg.depth, e->pack_plan, e->lora_rank, e->lora_s, e->dt, (hipStream_t)stream)) return rc;
  LATTE_HIP(hipStreamSynchronize((hipStream_t)stream));
  return LATTE_OK;
}

int latte_trainer_set_frozen(latte_trainer_t* e, const float* pos_embed, const float* temp_embed, int on_device, void* stream) {
  if (!e || !pos_embed || !temp_embed) return fail(LATTE_ERR_INVALID, "trainer_set_frozen: null");
  const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  LATTE_HIP(hipMemcpyAsync(e->pos, pos_embed, sizeof(float) * e->T * e->D, k, (hipStream_t)stream));
  LATTE_HIP(hipMemcpyAsync(e->temp, temp_embed, sizeof(float) * e->F * e->D, k, (hipStream_t)stream));
  LATTE_HIP(hipStreamSynchronize((hipStream_t)stream));
  return LATTE_OK;
}

int latte_trainer_sync_weights(latte_trainer_t* e, void* stream) {
  if (!e || !e->base.p) return fail(LATTE_ERR_STATE, "trainer_sync_weights: bind the parameter buffers first");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (e->lora_rank) {   // half(W + s B A) into the same operand copies, and the adapters' own padded half copies
    if ((rc = launch_pack_weights_lora(e->lora_descs, e->cfg.depth, e->pack_plan, e->lora_rank, e->lora_s, e->dt, st))) return rc;
    if ((rc = launch_lora_operands(e->lora_descs, e->cfg.depth * 4, e->lora_rank, e->dt, st))) return rc;
  } else if (e->fuse_small) {
    if ((rc = launch_pack_weights(e->pack_descs, e->cfg.depth, e->pack_plan, e->dt, st))) return rc;
  } else {   // the same table, one launch per entry
    for (const PackDesc& d : e->pack_host)
      if ((rc = launch_pack_weight(d.w, d.wn, d.wt, d.N, d.K, e->dt, st))) return rc;
  }
  if ((rc = launch_transpose_f32(P(e, e->rp.pe_w), e->pe_wt, e->D, e->KPE, st))) return rc;
  if ((rc = launch_transpose_f32(P(e, e->rp.fin_w), e->fin_wt, e->P, e->D, st))) return rc;
  e->weights_synced = true;
  return LATTE_OK;
}

// Forward with saved activations + loss terms + d loss / d model_output; the backward follows in stages (below).
// terms_out: device float [3][batch] = loss, mse, vb;  model_out_copy: optional device copy of the model output
}  // extern "C"

namespace {
// The three parts of a pass in the trainer's current run mode (run_F frames per sample, temporal blocks on / off, loss weight):
// q_sample + timestep gather, the forward with saved activations, the loss terms + seed.  begin_impl runs them in a row; the custom
// loss entry points (latte_trainer_forward / _seed) run the middle one and take the seed from the caller.

// ---- x_t = q_sample(x_start, t, noise), original timesteps of the respaced t
int qsample_part(latte_trainer_t* e, const latte_schedule_t* s, const float* tab, const float* x_start, const float* noise, const int64_t* t,
                 int B, hipStream_t st) {
  int rc;
  const int hw = e->H * e->H;
  if ((rc = launch_q_sample(tab, s->num_timesteps, x_start, noise, t, B, (size_t)e->run_F * e->Cin * hw, e->x_t, st))) return rc;
  if (e->tmap_of != s || e->tmap_n != s->num_timesteps) {
    if (e->tmap_n < s->num_timesteps) { if ((rc = e->arena.alloc(&e->tmap_dev, (size_t)s->num_timesteps, false))) return rc; }
    LATTE_HIP(hipMemcpyAsync(e->tmap_dev, s->timestep_map.data(), sizeof(int64_t) * s->num_timesteps, hipMemcpyHostToDevice, st));
    LATTE_HIP(hipStreamSynchronize(st));
    e->tmap_n = s->num_timesteps;
    e->tmap_of = s;
  }
  return launch_gather_i64(e->tmap_dev, t, e->t_orig, B, st);
}

// ---- forward of model(e->x_t, e->t_orig, y) with saved activations -> e->model_out (and model_out_copy)
int forward_part(latte_trainer_t* e, const int64_t* y, int batch, float* model_out_copy, hipStream_t st) {
  const auto& c = e->cfg;
  const RestParams& r = e->rp;
  int rc;
  const int D = e->D, T = e->T, F = e->run_F, Hm = e->Hm, B = batch, dt = e->dt, nmod = e->nmod;
  const bool temporal = e->run_temporal != 0;
  const int M = B * F * T, rps = F * T;
  const int hw = e->H * e->H;
  // ================================================================ forward
  // conditioning (latte.py:119-123,332-348): temb_pre = W0 freq(t) + b0; c = W2 SiLU(temb_pre) + b2 (+ y_emb); mod = adaLN(SiLU(c))
  if ((rc = launch_tfreq(e->t_orig, e->tfreq, B, st))) return rc;
  if ((rc = launch_small_linear(IN_PLAIN, e->tfreq, nullptr, P(e, r.t0_w), P(e, r.t0_b), nullptr, nullptr, e->temb_pre, B, D, 256, D, st))) return rc;
  if ((rc = launch_silu_rows(e->temb_pre, e->temb_act, (size_t)B * D, st))) return rc;
  if ((rc = launch_small_linear(IN_PLAIN, e->temb_act, nullptr, P(e, r.t2_w), P(e, r.t2_b), c.extras == 2 ? P(e, r.y_table) : nullptr,
                                c.extras == 2 ? y : nullptr, e->cvec, B, D, D, D, st))) return rc;
  if ((rc = launch_silu_rows(e->cvec, e->csilu, (size_t)B * D, st))) return rc;
  for (int i = 0; i < c.depth; ++i) {
    if ((rc = launch_small_linear(IN_PLAIN, e->csilu, nullptr, P(e, e->bp[i].ada_w), P(e, e->bp[i].ada_b), nullptr, nullptr,
                                  e->mod + (size_t)i * 6 * D, B, 6 * D, D, nmod, st))) return rc;
  }
  if ((rc = launch_small_linear(IN_PLAIN, e->csilu, nullptr, P(e, r.fin_ada_w), P(e, r.fin_ada_b), nullptr, nullptr,
                                e->mod + (size_t)c.depth * 6 * D, B, 2 * D, D, nmod, st))) return rc;
  if ((rc = launch_patch_embed(e->x_t, e->pe_wt, P(e, r.pe_b), e->pos, e->xs[0], B * F, e->Cin, e->H, c.patch_size, D, st)))
    return rc;
  for (int i = 0; i < c.depth; ++i) {
    const bool spatial = (i % 2) == 0;
    if (!temporal && !spatial) continue;
    const int nx = temporal ? i + 1 : i + 2;   // the next block that runs: its input snapshot is xs[2 nx] (depth is even: nx <= depth)
    const BlockParams& w = e->bp[i];
    BlockBuf& b = e->blk[i];
    const float* mb = e->mod + (size_t)i * 6 * D;
    float* x0 = e->xs[2 * i];
    float* x1 = e->xs[2 * i + 1];
    float* x2 = e->xs[2 * nx];
    // (fuse_small: blocks 1 .. depth-1 got xn1 -- and the temporal embedding -- from the previous block's closing gated add)
    if ((!e->fuse_small || i == 0) &&
        (rc = launch_ln_modulate(x0, x0, b.xn1, mb, mb + D, nmod, M, D, rps, i == 1 ? e->temp : nullptr, T, F, dt, st))) return rc;
    if ((rc = gemm_half(e, b.xn1, b.qkv_w, P(e, w.qkv_b), b.qkv, M, 3 * D, D, st))) return rc;
    AttnArgs a{};
    a.qkv = b.qkv; a.out = b.att; a.heads = c.num_heads; a.hd = e->hd; a.D = D;
    a.sample_stride = rps; a.scale = 1.0f / std::sqrt((float)e->hd);
    seq_layout(a, spatial, B, F, T);
    if ((rc = launch_attention(a, dt, st))) return rc;
    if ((rc = gemm_half(e, b.att, b.proj_w, P(e, w.proj_b), b.y1, M, D, D, st))) return rc;
    if (e->fuse_small) {   // x1 = x0 + g1 y1 and xn2 = LN-modulate(x1) in one pass over the rows
      if ((rc = launch_gated_add_ln(x0, b.y1, mb + 2 * D, nmod, x1, b.xn2, mb + 3 * D, mb + 4 * D, nmod, M, D, rps, nullptr, T, F, dt, st)))
        return rc;
    } else {
      if ((rc = launch_gated_add(x0, b.y1, mb + 2 * D, nmod, x1, M, D, rps, dt, st))) return rc;
      if ((rc = launch_ln_modulate(x1, x1, b.xn2, mb + 3 * D, mb + 4 * D, nmod, M, D, rps, nullptr, T, F, dt, st))) return rc;
    }
    if (gelu_fusable(e, M, Hm, D)) {   // u and h = gelu(u) out of one launch (bit-identical to the separate pass)
      if ((rc = gemm_gelu(e, EPI_BIAS_GELU_DUAL_H16, b.xn2, b.fc1_w, P(e, w.fc1_b), b.u, b.h, M, Hm, D, st))) return rc;
    } else {
      if ((rc = gemm_half(e, b.xn2, b.fc1_w, P(e, w.fc1_b), b.u, M, Hm, D, st))) return rc;
      if ((rc = launch_gelu_fwd(b.u, b.h, (size_t)M * Hm, dt, st))) return rc;
    }
    if ((rc = gemm_half(e, b.h, b.fc2_w, P(e, w.fc2_b), b.y2, M, D, Hm, st))) return rc;
    if (e->fuse_small && nx < c.depth) {   // x2 = x1 + g2 y2 (+ temp_embed in front of block 1) and the NEXT running block's xn1
      const float* nb = e->mod + (size_t)nx * 6 * D;
      if ((rc = launch_gated_add_ln(x1, b.y2, mb + 5 * D, nmod, x2, e->blk[nx].xn1, nb, nb + D, nmod, M, D, rps,
                                    nx == 1 ? e->temp : nullptr, T, F, dt, st))) return rc;
    } else if ((rc = launch_gated_add(x1, b.y2, mb + 5 * D, nmod, x2, M, D, rps, dt, st))) return rc;
  }
  float* xl = e->xs[2 * c.depth];
  const float* fm = e->mod + (size_t)c.depth * 6 * D;
  if ((rc = launch_final_layer(xl, fm, fm + D, nmod, e->fin_wt, P(e, r.fin_b), e->model_out, M, D, rps, T, c.patch_size,
                               e->Cout, e->H, st))) return rc;
  if (model_out_copy)
    LATTE_HIP(hipMemcpyAsync(model_out_copy, e->model_out, sizeof(float) * (size_t)B * F * e->Cout * hw, hipMemcpyDeviceToDevice, st));
  return LATTE_OK;
}

// ---- the backward's start state behind a seed in e->dmodel_out
int arm_backward(latte_trainer_t* e, const int64_t* y, int B, hipStream_t st) {
  LATTE_HIP(hipMemsetAsync(e->dc, 0, sizeof(float) * (size_t)B * e->D, st));   // d SiLU(c), summed over the adaLN linears by the stages
  // temporal blocks off: their stages write no dmod rows, and the last stage contracts ALL rows with the adaLN weights -- what the
  // previous pass left there must not reach the t / y embedders' gradients
  if (!e->run_temporal) LATTE_HIP(hipMemsetAsync(e->dmod, 0, sizeof(float) * (size_t)B * e->nmod, st));
  e->cur_batch = B;
  e->cur_y = y;
  e->next_stage = 0;
  return LATTE_OK;
}

// one pass; batch_cap: samples the per-sample buffers hold in the current run mode
int begin_impl(latte_trainer_t* e, const latte_schedule_t* s, int loss_type, const float* x_start, const float* noise, const int64_t* t,
               const int64_t* y, int batch, int batch_cap, float* terms_out, float* model_out_copy, void* stream) {
  if (!e || !s || !x_start || !noise || !t || !terms_out) return fail(LATTE_ERR_INVALID, "train step: null argument");
  if (!e->base.p) return fail(LATTE_ERR_STATE, "train step: bind the parameter buffers first");
  if (batch <= 0 || batch > batch_cap) return fail(LATTE_ERR_STATE, "train step: batch exceeds max_batch");
  if (loss_type != 0 && loss_type != 1) return fail(LATTE_ERR_INVALID, "train step: loss_type must be 0 (MSE) or 1 (RESCALED_MSE); the KL losses train no mean head (gaussian_diffusion.py:741-752)");
  if (s->mean_type != 0) return fail(LATTE_ERR_INVALID, "train step: only the epsilon-prediction models of train.py:92 are supported");
  if ((s->var_type == 0) != (e->cfg.learn_sigma != 0)) return fail(LATTE_ERR_INVALID, "train step: schedule / model disagree on learn_sigma");
  const auto& c = e->cfg;
  if (c.extras == 2 && !y) return fail(LATTE_ERR_INVALID, "train step: class-conditional model needs y");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (!e->weights_synced && (rc = latte_trainer_sync_weights(e, stream))) return rc;
  const int F = e->run_F, B = batch;
  const int hw = e->H * e->H;
  e->custom = 0;
  const float* tab = nullptr;
  if ((rc = schedule_device_tables(s, &tab, st))) return rc;
  if ((rc = qsample_part(e, s, tab, x_start, noise, t, B, st))) return rc;
  if ((rc = forward_part(e, y, B, model_out_copy, st))) return rc;

  // ================================================================ loss values and d loss / d model_output
  float vb_scale = 1.0f;
  if (loss_type == 1) vb_scale = (float)(s->num_timesteps / 1000.0);
  if ((rc = latte_training_losses(s, loss_type, x_start, e->x_t, noise, e->model_out, t, B, F, e->Cin, hw, e->loss_ws,
                                  e->loss_ws_floats - 3 * e->max_batch, terms_out + B, terms_out + 2 * B, terms_out, stream))) return rc;
  if ((rc = launch_loss_grad(tab, s->num_timesteps, s->mean_type, s->var_type, x_start, e->x_t, noise, e->model_out, t, B, F, e->Cin, hw,
                             vb_scale, e->dmodel_out, st, e->loss_divisor * e->run_weight))) return rc;
  if (scaling_active(e) && (rc = launch_scale_f32_dev(e->dmodel_out, e->scaler, 0, (size_t)B * F * e->Cout * hw, st))) return rc;
  return arm_backward(e, y, B, st);
}

// the trainer back in the plain run mode (an image pass that was abandoned half way included)
void plain_mode(latte_trainer_t* e) {
  if (e->joint_saved_acc >= 0) e->grad_accumulate = e->joint_saved_acc;
  e->joint_saved_acc = -1;
  e->run_F = e->F;
  e->run_temporal = 1;
  e->run_weight = 1.0f;
}
}  // namespace

extern "C" {

int latte_trainer_begin(latte_trainer_t* e, const latte_schedule_t* s, int loss_type, const float* x_start, const float* noise,
                        const int64_t* t, const int64_t* y, int batch, float* terms_out, float* model_out_copy, void* stream) {
  if (!e) return fail(LATTE_ERR_INVALID, "train step: null argument");
  plain_mode(e);
  return begin_impl(e, s, loss_type, x_start, noise, t, y, batch, e->max_batch, terms_out, model_out_copy, stream);
}

// One joint micro-batch: x_start / noise / model_out_copy [batch, F + N, C, H, W], y_image int64 [batch, N] after label dropout.
// The video pass runs here completely (forward and every stage, in the caller's assign / accumulate mode), then the image pass's
// forward in accumulate mode; ITS stages are the caller's (latte_trainer_backward_stage: after stage k the slice is final).
int latte_trainer_begin_joint(latte_trainer_t* e, const latte_schedule_t* s, int loss_type, const float* x_start, const float* noise,
                              const int64_t* t, const int64_t* y, const int64_t* y_image, int batch, int use_image_num, float* terms_out,
                              float* model_out_copy, void* stream) {
  if (!e || !s || !x_start || !noise || !t || !terms_out) return fail(LATTE_ERR_INVALID, "joint train step: null argument");
  if (use_image_num < 1 || use_image_num > e->max_image)
    return fail(LATTE_ERR_INVALID, "joint train step: use_image_num must be in [1, max_image_num of latte_trainer_create_joint]");
  if (batch <= 0 || batch > e->max_batch) return fail(LATTE_ERR_STATE, "train step: batch exceeds max_batch");
  if (e->cfg.extras == 2 && (!y || !y_image)) return fail(LATTE_ERR_INVALID, "joint train step: class-conditional model needs y and y_image");
  hipStream_t st = (hipStream_t)stream;
  const int B = batch, F = e->F, N = use_image_num;
  const size_t per = (size_t)e->Cin * e->H * e->H, per_out = (size_t)e->Cout * e->H * e->H;
  float* tv = e->jterms;
  float* ti = e->jterms + 3 * (size_t)e->max_batch;
  int rc;
  plain_mode(e);
  if ((rc = launch_joint_split(x_start, noise, t, e->jx_v, e->jn_v, e->jx_i, e->jn_i, e->jt_i, B, F, N, per, st))) return rc;
  // ---- video pass: the plain step with the weight F / (F + N) on its loss
  e->run_weight = (float)(F + N) / (float)F;
  rc = begin_impl(e, s, loss_type, e->jx_v, e->jn_v, t, y, B, e->max_batch, tv, model_out_copy ? e->jmo : nullptr, stream);
  for (int k = 0; !rc && k < latte_trainer_num_stages(e); ++k) rc = latte_trainer_backward_stage(e, k, stream);
  if (rc) { plain_mode(e); return rc; }
  // ---- image pass: B N one-frame samples, spatial blocks only, gradients ADDED (unscaled by their writers)
  e->joint_saved_acc = e->grad_accumulate;
  e->grad_accumulate = 1;
  e->run_F = 1;
  e->run_temporal = 0;
  e->run_weight = (float)(F + N) / (float)N;
  rc = begin_impl(e, s, loss_type, e->jx_i, e->jn_i, e->jt_i, e->cfg.extras == 2 ? y_image : nullptr, B * N, e->max_batch * e->max_image, ti,
                  nullptr, stream);
  if (!rc) rc = launch_joint_merge(tv, ti, terms_out, e->jmo, e->model_out, model_out_copy, B, F, N, per_out, st);
  if (rc) { plain_mode(e); e->next_stage = 1 << 30; }
  return rc;
}

// adaLN linear of block i (i == depth: the final layer's): bias / weight gradients from the finished dmod rows, and its
// contribution to d SiLU(c)
static int adaln_bwd(latte_trainer_t* e, int i, hipStream_t st) {
  const int D = e->D, B = e->cur_batch, nmod = e->nmod;
  const bool fin = i == e->cfg.depth;
  const int64_t w = fin ? e->rp.fin_ada_w : e->bp[i].ada_w, bias = fin ? e->rp.fin_ada_b : e->bp[i].ada_b;
  const int N = fin ? 2 * D : 6 * D;
  const float* dm = e->dmod + (size_t)i * 6 * D;
  int rc;
  const int acc = e->grad_accumulate;
  const float* gs = acc_scale(e);
  if ((rc = launch_rows_sum(dm, B, nmod, N, G(e, bias), acc, st, gs))) return rc;
  if ((rc = launch_naive_gemm(dm, 1, nmod, e->csilu, D, 1, G(e, w), D, 1, N, D, B, 1.0f, acc, st, 1, nullptr, gs))) return rc;   // dW[n, k]
  if ((rc = launch_naive_gemm(dm, nmod, 1, P(e, w), D, 1, e->dtmp, D, 1, B, D, N, 1.0f, 0, st, 48, e->ng_ws))) return rc;  // d csilu
  return launch_add_rows(e->dc, e->dtmp, (size_t)B * D, st);
}

// the MLP gate's partial rows of block i wait in one of two buffers for its stage's finalize launch, which follows the pass that
// fills the NEXT running block's: consecutive running blocks alternate (temporal off: blocks 0, 2, 4, ...)
static float* pg2_of(const latte_trainer_t* e, int i) { return ((e->run_temporal ? i : i >> 1) & 1) ? e->pg2b : e->pg2; }

// The adapter gradients of targeted linear li behind dY [M, N] (x [M, K]): h = s x A^T and g = s dY B by the row-local product (kept as
// split half pairs, train_lora.hip), then
// dB = dY^T h and dA = g^T x as chunked outer products whose partials launch_split_reduce sums in chunk order, takes out of the
// loss-scaled domain and assigns -- or, in accumulate mode, adds -- to the adapter gradient buffer.  Four launches + two reductions.
static int lora_grads(latte_trainer_t* e, int li, const half_t* dY, const half_t* x, int M, int N, int K, hipStream_t st) {
  const LoraPackDesc& d = e->lora_host[li];
  const LoraOffsets& o = e->lo[li / 4];
  if (o.a[li % 4] < 0) return LATTE_OK;
  const int r = e->lora_rank, dt = e->dt;
  const float* us = scaling_active(e) ? e->scaler : nullptr;
  float* dA = e->adapters.g + o.a[li % 4];
  float* dB = e->adapters.g + o.b[li % 4];
  int rc, chunk = 0;
  if ((rc = launch_lora_down(x, d.a_h, e->lora_h, M, K, r, e->lora_s, dt, st))) return rc;
  if ((rc = launch_lora_down(dY, d.bt_h, e->lora_g, M, N, r, e->lora_s, dt, st))) return rc;
  int splits = lora_outer_plan(M, N, &chunk);
  if ((int64_t)splits * r * N > e->wg_ws_floats) return fail(LATTE_ERR_STATE, "lora: workspace too small");
  if ((rc = launch_lora_outer(e->lora_h, dY, e->wg_ws, M, N, r, chunk, 1, dt, st))) return rc;
  if ((rc = launch_split_reduce(e->wg_ws, splits, (size_t)r * N, (size_t)r * N, dB, e->grad_accumulate, st, us))) return rc;
  splits = lora_outer_plan(M, K, &chunk);
  if ((int64_t)splits * r * K > e->wg_ws_floats) return fail(LATTE_ERR_STATE, "lora: workspace too small");
  if ((rc = launch_lora_outer(e->lora_g, x, e->wg_ws, M, K, r, chunk, 0, dt, st))) return rc;
  return launch_split_reduce(e->wg_ws, splits, (size_t)r * K, (size_t)r * K, dA, e->grad_accumulate, st, us);
}

// The backward of one linear y = x W^T + b behind dY [M, N] (x [M, K]; wt: the [K, N] operand copy of W): the bias gradient in the
// form the mode asks for, dW, then dX = dY W -- through gelu'(u) where the linear's input was gelu(u).
// fuse_small: the bias gradient is column-sum partial rows that wait for launch_stage_finalize -- pc [*pc_rows][N], filled here (on
// the weight-gradient launch where the 8-wave kernel takes the shape), or pc == nullptr where the LayerNorm backward that produced dY
// left them beside the gate's -- and wgrad unscales what it writes.  Otherwise launch_colsum_half sums straight into the gradient.
// LoRA (li = block * 4 + linear): W and b are frozen -- no bias sums, no weight gradient; a targeted linear gets its adapter gradients.
static int linear_bwd(latte_trainer_t* e, const half_t* dY, const half_t* x, const half_t* wt, int M, int N, int K, int64_t w, int64_t bias,
                      int li, float* pc, int* pc_rows, half_t* dX, half_t* u, hipStream_t st) {
  int rc;
  if (e->lora_rank) {
    if ((rc = lora_grads(e, li, dY, x, M, N, K, st))) return rc;
  } else if (e->fuse_small) {
    const bool ride = pc && gemm_tn8_ok(M, N, K);
    if (pc && !ride && (rc = launch_colsum_half(dY, M, N, pc, nullptr, 0, e->dt, st))) return rc;
    if ((rc = wgrad(e, dY, x, M, N, K, G(e, w), st, scaling_active(e), ride ? pc : nullptr, ride ? pc_rows : nullptr))) return rc;
  } else {
    if ((rc = launch_colsum_half(dY, M, N, e->part_cols, G(e, bias), e->grad_accumulate, e->dt, st, acc_scale(e)))) return rc;
    if ((rc = wgrad(e, dY, x, M, N, K, G(e, w), st))) return rc;
  }
  // du = (dy W) gelu'(u) in the GEMM's epilogue where it takes the shape (the product is not rounded to half in between)
  if (u && gelu_fusable(e, M, K, N)) return gemm_gelu(e, EPI_DGELU_H16, dY, wt, e->zeros, dX, u, M, K, N, st);
  if ((rc = gemm_half(e, dY, wt, e->zeros, dX, M, K, N, st))) return rc;
  return u ? launch_gelu_bwd(u, dX, dX, (size_t)M * K, e->dt, st) : LATTE_OK;
}

// ---- stage 0, the final layer: out = unpatchify(Linear(LN-mod(x)))
static int backward_final(latte_trainer_t* e, hipStream_t st) {
  const auto& c = e->cfg;
  const RestParams& r = e->rp;
  int rc;
  const int D = e->D, T = e->T, F = e->run_F, B = e->cur_batch, dt = e->dt, nmod = e->nmod;
  const int M = B * F * T, rps = F * T;
  const int acc = e->grad_accumulate;
  const float* gs = acc_scale(e);
  float* xl = e->xs[2 * c.depth];
  const float* fm = e->mod + (size_t)c.depth * 6 * D;
  const bool lora = e->lora_rank != 0;   // the base is frozen: only the input gradients of the stage are due
  if ((rc = launch_unpatchify_bwd(e->dmodel_out, e->dtok, B * F, e->G, c.patch_size, e->Cout, st))) return rc;
  if (e->fuse_small && e->P <= 32) {
    // the linear's weight / bias gradients (exact fp32 products of dtok with the half LN output, as below) in one launch + its
    // reductions, and its input gradient straight to half (train_fin.hip)
    if ((rc = launch_ln_modulate(xl, xl, e->xnh, fm, fm + D, nmod, M, D, rps, nullptr, T, F, dt, st))) return rc;
    if (!lora && (rc = launch_narrow_outer(e->dtok, e->P, e->xnh, 1, D, M, G(e, r.fin_w), D, 1, G(e, r.fin_b), nullptr, e->no_ws, dt, gs, st, acc)))
      return rc;
    if ((rc = launch_narrow_dx(e->dtok, e->P, P(e, r.fin_w), D, M, e->dxnH, dt, st))) return rc;
  } else {
    if (!lora && (rc = launch_naive_gemm(e->ones, 0, 1, e->dtok, e->P, 1, G(e, r.fin_b), e->P, 1, 1, e->P, M, 1.0f, acc, st, 64, e->ng_ws, gs))) return rc;
    if ((rc = launch_ln_modulate(xl, xl, e->xnh, fm, fm + D, nmod, M, D, rps, nullptr, T, F, dt, st))) return rc;
    if (!lora) {
      if ((rc = launch_convert_h16_to_f32(e->xnh, e->f32a, (int64_t)M * D, dt, st))) return rc;
      if ((rc = launch_naive_gemm(e->dtok, 1, e->P, e->f32a, D, 1, G(e, r.fin_w), D, 1, e->P, D, M, 1.0f, acc, st, 64, e->ng_ws, gs))) return rc;
    }
    if ((rc = launch_naive_gemm(e->dtok, e->P, 1, P(e, r.fin_w), D, 1, e->f32b, D, 1, M, D, e->P, 1.0f, 0, st))) return rc;
    if ((rc = launch_convert_f32_to_h16(e->f32b, e->dxnH, (int64_t)M * D, dt, st))) return rc;
  }
  float* dm = e->dmod + (size_t)c.depth * 6 * D;
  if (!e->fuse_small) {
    if ((rc = launch_ln_bwd(e->dxnH, xl, fm + D, nmod, nullptr, e->dx, e->part_rows, dm, dm + D, nmod, M, D, rps, dt, st))) return rc;
    return lora ? LATTE_OK : adaln_bwd(e, c.depth, st);
  }
  // fuse_small: shift / scale gradients of the final modulation and its adaLN linear's bias / weight gradients in one launch ... and the
  // gated residual's backward of the last block's MLP branch on the same pass over dx (its stage starts at the wgrad)
  const int il = e->run_temporal ? c.depth - 1 : c.depth - 2;   // the last block that ran
  if ((rc = launch_ln_bwd(e->dxnH, xl, fm + D, nmod, nullptr, e->dx, e->pl1, nullptr, nullptr, nmod, M, D, rps, dt, st, e->blk[il].y2,
                          e->mod + (size_t)il * 6 * D + 5 * D, nmod, e->dyD, pg2_of(e, il)))) return rc;
  if (lora) return LATTE_OK;   // the finalize launch writes base gradients only
  StageFinArgs a{};
  a.mod_src[0] = a.mod_src[1] = e->pl1; a.mod_nsum[0] = a.mod_nsum[1] = 2; a.mod_which[0] = 0; a.mod_which[1] = 1;
  a.n_mod = 2; a.rows_per_sample = rps / (4 * train_rows_per_run(rps)); a.B = B; a.D = D;
  a.dmod = dm; a.dmod_stride = nmod; a.csilu = e->csilu;
  a.dW = G(e, r.fin_ada_w); a.db = G(e, r.fin_ada_b);
  a.n_bias = 0; a.scaler = gs;   // assign mode: this stage's slice is unscaled by the pass behind the stage
  a.accumulate = acc;
  return launch_stage_finalize(a, st);
}

// ---- stages 1 .. depth, block i = depth - stage: x1 = x0 + g1 * proj(attn(qkv(xn1))), x2 = x1 + g2 * fc2(gelu(fc1(xn2)))
static int backward_block(latte_trainer_t* e, int i, hipStream_t st) {
  int rc;
  const int D = e->D, T = e->T, F = e->run_F, Hm = e->Hm, B = e->cur_batch, dt = e->dt, nmod = e->nmod;
  const bool temporal = e->run_temporal != 0, spatial = (i % 2) == 0, fs = e->fuse_small != 0;
  const int M = B * F * T, rps = F * T;
  if (!temporal && !spatial) return LATTE_OK;   // the block did not run: its gradient slice, dx and the waiting partial rows stay
  const int ip = temporal ? i - 1 : i - 2;      // the running block in front of this one
  const BlockParams& w = e->bp[i];
  BlockBuf& b = e->blk[i];
  const float* mb = e->mod + (size_t)i * 6 * D;
  float* dm = e->dmod + (size_t)i * 6 * D;
  float* pg2 = pg2_of(e, i);
  // bias gradients of fc1 / qkv under fuse_small: partial rows per column-sum chunk, or per split of the weight-gradient launch
  int fc1_rows = colsum_chunks(M), qkv_rows = colsum_chunks(M);
  // ---- MLP branch.  fuse_small: dy = g2 dx and the gate / bias partial rows were left by the LayerNorm backward that produced dx
  // (the previous stage's last pass); the partial rows wait for this stage's finalize launch
  if (!fs && (rc = launch_gate_bwd(e->dx, b.y2, mb + 5 * D, nmod, e->dyD, e->part_rows, dm + 5 * D, nmod, M, D, rps, dt, st))) return rc;
  if ((rc = linear_bwd(e, e->dyD, b.h, b.fc2_wt, M, D, Hm, w.fc2_w, w.fc2_b, i * 4 + 3, nullptr, nullptr, e->dhH, b.u, st))) return rc;
  if ((rc = linear_bwd(e, e->dhH, b.xn2, b.fc1_wt, M, Hm, D, w.fc1_w, w.fc1_b, i * 4 + 2, e->pc_fc1, &fc1_rows, e->dxnH, nullptr, st))) return rc;
  // ---- attention branch.  fuse_small: its gate backward rides on LN2's backward
  if (fs) {
    if ((rc = launch_ln_bwd(e->dxnH, e->xs[2 * i + 1], mb + 4 * D, nmod, e->dx, e->dx, e->pl2, nullptr, nullptr, nmod, M, D, rps, dt, st, b.y1,
                            mb + 2 * D, nmod, e->dyD, e->pg1))) return rc;
  } else {
    if ((rc = launch_ln_bwd(e->dxnH, e->xs[2 * i + 1], mb + 4 * D, nmod, e->dx, e->dx, e->part_rows, dm + 3 * D, dm + 4 * D, nmod, M, D, rps, dt,
                            st))) return rc;
    if ((rc = launch_gate_bwd(e->dx, b.y1, mb + 2 * D, nmod, e->dyD, e->part_rows, dm + 2 * D, nmod, M, D, rps, dt, st))) return rc;
  }
  if ((rc = linear_bwd(e, e->dyD, b.att, b.proj_wt, M, D, D, w.proj_w, w.proj_b, i * 4 + 1, nullptr, nullptr, e->dxnH, nullptr, st))) return rc;   // d(attention output)
  AttnArgs sl{};
  seq_layout(sl, spatial, B, F, T);
  if ((rc = launch_attention_bwd(b.qkv, b.att, e->dxnH, e->dqkvH, e->attn_stats, sl.num_seq, sl.L, e->cfg.num_heads, e->hd, sl.U, rps,
                                 sl.seq_stride, sl.row_stride, dt, st))) return rc;
  if ((rc = linear_bwd(e, e->dqkvH, b.xn1, b.qkv_wt, M, 3 * D, D, w.qkv_w, w.qkv_b, i * 4 + 0, e->pc_qkv, &qkv_rows, e->dxnH, nullptr, st))) return rc;
  // ---- LN1's backward, and the stage's tail
  if (!fs) {
    if ((rc = launch_ln_bwd(e->dxnH, e->xs[2 * i], mb + D, nmod, e->dx, e->dx, e->part_rows, dm, dm + D, nmod, M, D, rps, dt, st))) return rc;
    return e->lora_rank ? LATTE_OK : adaln_bwd(e, i, st);
  }
  if (ip >= 0) {   // + the gate backward of the previous running block's MLP branch (the next stage's first step)
    if ((rc = launch_ln_bwd(e->dxnH, e->xs[2 * i], mb + D, nmod, e->dx, e->dx, e->pl1, nullptr, nullptr, nmod, M, D, rps, dt, st, e->blk[ip].y2,
                            e->mod + (size_t)ip * 6 * D + 5 * D, nmod, e->dyD, pg2_of(e, ip)))) return rc;
  } else if ((rc = launch_ln_bwd(e->dxnH, e->xs[2 * i], mb + D, nmod, e->dx, e->dx, e->pl1, nullptr, nullptr, nmod, M, D, rps, dt, st)))
    return rc;
  if (e->lora_rank) return LATTE_OK;   // modulation, adaLN and bias gradients: all of the frozen base
  // one launch: the six modulation gradients, the adaLN linear's bias / weight gradients, the four linears' bias gradients
  StageFinArgs a{};
  const float* msrc[6] = {e->pl1, e->pl1, e->pg1, e->pl2, e->pl2, pg2};
  const int mwhich[6] = {0, 1, 0, 0, 1, 0};
  for (int k = 0; k < 6; ++k) { a.mod_src[k] = msrc[k]; a.mod_nsum[k] = 2; a.mod_which[k] = mwhich[k]; }
  const int rb = rps / (4 * train_rows_per_run(rps));   // partial rows (blocks of 4 runs) per sample
  a.n_mod = 6; a.rows_per_sample = rb; a.B = B; a.D = D;
  a.dmod = dm; a.dmod_stride = nmod; a.csilu = e->csilu;
  a.dW = G(e, w.ada_w); a.db = G(e, w.ada_b);
  a.n_bias = 4;
  a.bias_src[0] = e->pc_qkv;  a.bias_rows[0] = qkv_rows; a.bias_stride[0] = 3 * D; a.bias_cols[0] = 3 * D; a.bias_out[0] = G(e, w.qkv_b);
  a.bias_src[1] = e->pg1 + D; a.bias_rows[1] = B * rb;   a.bias_stride[1] = 2 * D; a.bias_cols[1] = D;     a.bias_out[1] = G(e, w.proj_b);
  a.bias_src[2] = e->pc_fc1;  a.bias_rows[2] = fc1_rows; a.bias_stride[2] = Hm;    a.bias_cols[2] = Hm;    a.bias_out[2] = G(e, w.fc1_b);
  a.bias_src[3] = pg2 + D;    a.bias_rows[3] = B * rb;   a.bias_stride[3] = 2 * D; a.bias_cols[3] = D;     a.bias_out[3] = G(e, w.fc2_b);
  a.scaler = scaling_active(e) ? e->scaler : nullptr;
  a.accumulate = e->grad_accumulate;
  return launch_stage_finalize(a, st);
}

// ---- stage depth + 1: patch embed (latte.py:233,330-331: tokens = pix W^T + b + pos) and the conditioning tail
static int backward_embed(latte_trainer_t* e, hipStream_t st) {
  const auto& c = e->cfg;
  const RestParams& r = e->rp;
  int rc;
  const int D = e->D, T = e->T, F = e->run_F, B = e->cur_batch, dt = e->dt, nmod = e->nmod;
  const int M = B * F * T;
  const int acc = e->grad_accumulate;
  const float* gs = acc_scale(e);
  if (e->lora_rank) return LATTE_OK;   // the whole stage writes base gradients; e->dx stays for latte_trainer_input_grad
  if (e->fuse_small && e->KPE <= 32) {   // dW[k][j] = sum_m dx[m][k] pix[m][j], db[k] = sum_m dx[m][k]: one launch + reductions
    if ((rc = launch_im2col_patch(e->x_t, e->pix, B * F, e->G, c.patch_size, e->Cin, st))) return rc;
    if ((rc = launch_narrow_outer(e->pix, e->KPE, e->dx, 0, D, M, G(e, r.pe_w), 1, e->KPE, nullptr, G(e, r.pe_b), e->no_ws, dt, gs, st, acc)))
      return rc;
  } else {
    if ((rc = launch_naive_gemm(e->ones, 0, 1, e->dx, D, 1, G(e, r.pe_b), D, 1, 1, D, M, 1.0f, acc, st, 64, e->ng_ws, gs))) return rc;
    if ((rc = launch_im2col_patch(e->x_t, e->pix, B * F, e->G, c.patch_size, e->Cin, st))) return rc;
    if ((rc = launch_naive_gemm(e->dx, 1, D, e->pix, e->KPE, 1, G(e, r.pe_w), e->KPE, 1, D, e->KPE, M, 1.0f, acc, st, 64, e->ng_ws, gs))) return rc;
  }
  // ---- conditioning tail: d SiLU(c) (summed by the stages) -> c = temb (+ y_emb) -> t_embedder MLP
  if (e->fuse_small) {   // d SiLU(c) = dmod W over every adaLN linear of the model at once (the stages left their dmod rows)
    const int64_t stride = e->bp[1].ada_w - e->bp[0].ada_w;   // depth is even: block 1 exists
    if ((rc = launch_adaln_dc(e->dmod, nmod, B, P(e, e->bp[0].ada_w), (long)stride, c.depth, 6 * D, P(e, r.fin_ada_w), D, e->dc_ws, e->dc, st)))
      return rc;
  }
  if ((rc = launch_silu_bwd(e->dc, e->cvec, e->dtmp, (size_t)B * D, 0, st))) return rc;     // dtmp = dc (gradient of c = temb + y_emb)
  if (c.extras == 2) {
    // the scatter accumulates (a label may repeat inside the batch): clear the slice first, so that forward_backward ASSIGNS this
    // gradient like every other one (two calls without an optimiser step in between must not double it).  Accumulate mode: no
    // clear -- the scatter's own add IS the accumulation (rows of labels this micro-batch does not hold keep their sum)
    float* gy = G(e, r.y_table);
    if (!acc) LATTE_HIP(hipMemsetAsync(gy, 0, (size_t)(c.num_classes + 1) * D * sizeof(float), st));
    if ((rc = launch_embedding_bwd(e->dtmp, e->cur_y, gy, B, D, st, gs))) return rc;
  }
  // temb = W2 SiLU(temb_pre) + b2
  if ((rc = launch_rows_sum(e->dtmp, B, D, D, G(e, r.t2_b), acc, st, gs))) return rc;
  if ((rc = launch_naive_gemm(e->dtmp, 1, D, e->temb_act, D, 1, G(e, r.t2_w), D, 1, D, D, B, 1.0f, acc, st, 1, nullptr, gs))) return rc;
  if ((rc = launch_naive_gemm(e->dtmp, D, 1, P(e, r.t2_w), D, 1, e->dtmp2, D, 1, B, D, D, 1.0f, 0, st))) return rc;
  if ((rc = launch_silu_bwd(e->dtmp2, e->temb_pre, e->dtmp2, (size_t)B * D, 0, st))) return rc;
  // temb_pre = W0 freq(t) + b0
  if ((rc = launch_rows_sum(e->dtmp2, B, D, D, G(e, r.t0_b), acc, st, gs))) return rc;
  return launch_naive_gemm(e->dtmp2, 1, D, e->tfreq, 256, 1, G(e, r.t0_w), 256, 1, D, 256, B, 1.0f, acc, st, 1, nullptr, gs);
}

int latte_trainer_num_stages(const latte_trainer_t* e) { return e ? e->cfg.depth + 2 : 0; }

// the slice of the flat gradient buffer that stage `stage` finalises: 0 = final layer, 1 .. depth = blocks depth-1 .. 0,
// depth + 1 = patch embed + t / y embedders (the head of the buffer) -- of the TRAINED set: the adapters have nothing in front of
// or behind their blocks, so their stages 0 and depth + 1 finish the empty slices at the buffer's end and head
int latte_trainer_stage_range(const latte_trainer_t* e, int stage, int64_t* offset, int64_t* numel) {
  if (!e || !offset || !numel || stage < 0 || stage > e->cfg.depth + 1) return fail(LATTE_ERR_INVALID, "stage_range: bad stage");
  const TrainedSet& s = trained(e);
  const int depth = e->cfg.depth, i = depth - stage;   // block i, or: -1 = in front of the blocks, depth = behind them
  *offset = i < 0 ? 0 : s.block_begin[i];
  *numel = (i < depth ? s.block_begin[i + 1] : s.total) - *offset;
  return LATTE_OK;
}

// Backward of one stage (in order 0, 1, ..., depth + 1 after latte_trainer_begin).  After stage k the gradient slice
// latte_trainer_stage_range(k) is final: the data-parallel driver starts its all-reduce while the next stages run.
int latte_trainer_backward_stage(latte_trainer_t* e, int stage, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (!e || !e->base.p) rc = fail(LATTE_ERR_STATE, "backward_stage: no step in flight");
  else if (stage != e->next_stage || stage > e->cfg.depth + 1) rc = fail(LATTE_ERR_STATE, "backward_stage: stages run in order after latte_trainer_begin");
  else {
    e->next_stage = stage + 1;
    try {
      rc = stage == 0 ? backward_final(e, st) : stage <= e->cfg.depth ? backward_block(e, e->cfg.depth - stage, st) : backward_embed(e, st);
    } catch (const FrozenBaseWrite&) {
      rc = fail(LATTE_ERR_STATE, "backward_stage: a writer of a base gradient was reached, but no base gradient buffer is bound (LoRA)");
    }
  }
  // (fuse_small: the block stages' slices were unscaled by the kernels that wrote them; accumulate mode: every slice was)
  // (LoRA: the adapter gradients' reductions unscale in every mode)
  if (!rc && !e->lora_rank && scaling_active(e) && !e->grad_accumulate && !(e->fuse_small && stage >= 1 && stage <= e->cfg.depth)) {   // the slice this stage finalised leaves the loss-scaled domain
    int64_t off = 0, n = 0;
    if ((rc = latte_trainer_stage_range(e, stage, &off, &n))) return rc;
    rc = launch_scale_f32_dev(trained(e).g + off, e->scaler, 1, (size_t)n, st);
  }
  if (e && e->joint_saved_acc >= 0 && (rc || stage == e->cfg.depth + 1)) {   // the image pass of a joint micro-batch is over
    plain_mode(e);
    if (rc) e->next_stage = 1 << 30;
  }
  return rc;
}

int latte_trainer_set_option(latte_trainer_t* e, const char* name, double value) {
  if (!e || !name) return fail(LATTE_ERR_INVALID, "trainer_set_option: null argument");
  const std::string n(name);
  if (n == "loss_scale") {
    if (!pow2_in(value, 1.0, 16777216.0)) return fail(LATTE_ERR_INVALID, "loss_scale must be a power of two in [1, 2^24]");
    e->loss_scale = (float)value;
    return upload_scaler(e, 1);
  }
  if (n == "dynamic_loss_scale") {   // 0: the scale stays what "loss_scale" set (overflowing steps are still skipped)
    e->dynamic_scale = value != 0.0 ? 1 : 0;
    return upload_scaler(e, 2);
  }
  if (n == "loss_scale_growth_interval") {
    if (!(value >= 1.0) || value > 1e7) return fail(LATTE_ERR_INVALID, "loss_scale_growth_interval must be in [1, 1e7]");
    e->growth_interval = (float)value;
    return upload_scaler(e, 2);
  }
  if (n == "fuse_small") {   // 0: the separate finalize / column-sum / adaLN launches of rounds 2 - 6, 1: train_fin.hip (default)
    if (step_in_flight(e) || e->custom == 1) return fail(LATTE_ERR_STATE, "fuse_small: a step is in flight");
    e->fuse_small = value != 0.0 ? 1 : 0;
    return LATTE_OK;
  }
  if (n == "grad_accumulate") {   // 0: the gradient writers assign (default), 1: they add (struct latte_trainer)
    if (step_in_flight(e)) return fail(LATTE_ERR_STATE, "grad_accumulate: a step is in flight");
    e->grad_accumulate = value != 0.0 ? 1 : 0;
    return LATTE_OK;
  }
  if (n == "loss_divisor") {
    if (step_in_flight(e)) return fail(LATTE_ERR_STATE, "loss_divisor: a step is in flight");
    if (!(value >= 1.0) || value > 65536.0) return fail(LATTE_ERR_INVALID, "loss_divisor must be in [1, 65536]");
    e->loss_divisor = (float)value;
    return LATTE_OK;
  }
  if (n == "fuse_gelu") {   // 0: separate GELU passes (rounds 2 - 5), 1: inside the GEMM epilogues (default)
    e->fuse_gelu = value != 0.0 ? 1 : 0;
    return LATTE_OK;
  }
  return fail(LATTE_ERR_INVALID, std::string("trainer_set_option: unknown option '") + name + "'");
}

// begin + every stage: one micro-batch, gradients of terms["loss"].mean() in the bound gradient buffer
int latte_trainer_forward_backward(latte_trainer_t* e, const latte_schedule_t* s, int loss_type, const float* x_start, const float* noise,
                                   const int64_t* t, const int64_t* y, int batch, float* terms_out, float* model_out_copy, void* stream) {
  int rc = latte_trainer_begin(e, s, loss_type, x_start, noise, t, y, batch, terms_out, model_out_copy, stream);
  for (int k = 0; !rc && k < latte_trainer_num_stages(e); ++k) rc = latte_trainer_backward_stage(e, k, stream);
  return rc;
}

int latte_trainer_forward_backward_joint(latte_trainer_t* e, const latte_schedule_t* s, int loss_type, const float* x_start, const float* noise,
                                         const int64_t* t, const int64_t* y, const int64_t* y_image, int batch, int use_image_num,
                                         float* terms_out, float* model_out_copy, void* stream) {
  int rc = latte_trainer_begin_joint(e, s, loss_type, x_start, noise, t, y, y_image, batch, use_image_num, terms_out, model_out_copy, stream);
  for (int k = 0; !rc && k < latte_trainer_num_stages(e); ++k) rc = latte_trainer_backward_stage(e, k, stream);
  return rc;
}

// ---- custom losses: the forward alone, the caller's seed, the input gradient (include/latte_amd.h)
int latte_trainer_forward(latte_trainer_t* e, const float* x, const int64_t* t_model, const int64_t* y, int batch, float* model_out,
                          void* stream) {
  if (!e || !x || !t_model || !model_out) return fail(LATTE_ERR_INVALID, "trainer_forward: null argument");
  if (!e->base.p) return fail(LATTE_ERR_STATE, "trainer_forward: bind the parameter buffers first");
  if (e->joint_saved_acc >= 0) return fail(LATTE_ERR_STATE, "trainer_forward: the image pass of a joint micro-batch is in flight");
  if (step_in_flight(e)) return fail(LATTE_ERR_STATE, "trainer_forward: a step is in flight");
  if (batch <= 0 || batch > e->max_batch) return fail(LATTE_ERR_STATE, "trainer_forward: batch exceeds max_batch");
  if (e->cfg.extras == 2 && !y) return fail(LATTE_ERR_INVALID, "trainer_forward: class-conditional model needs y");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (!e->weights_synced && (rc = latte_trainer_sync_weights(e, stream))) return rc;
  plain_mode(e);
  e->custom = 0;
  // the patch embed's weight gradient reads x from e->x_t at the last stage, the forward its timesteps from e->t_orig
  LATTE_HIP(hipMemcpyAsync(e->x_t, x, sizeof(float) * (size_t)batch * e->F * e->Cin * e->H * e->H, hipMemcpyDeviceToDevice, st));
  LATTE_HIP(hipMemcpyAsync(e->t_orig, t_model, sizeof(int64_t) * (size_t)batch, hipMemcpyDeviceToDevice, st));
  if ((rc = forward_part(e, y, batch, model_out, st))) return rc;
  e->fwd_batch = batch;
  e->fwd_y = y;
  e->custom = 1;
  return LATTE_OK;
}

int latte_trainer_seed(latte_trainer_t* e, const float* d_model_out, void* stream) {
  if (!e || !d_model_out) return fail(LATTE_ERR_INVALID, "trainer_seed: null argument");
  if (e->custom != 1) return fail(LATTE_ERR_STATE, "trainer_seed: one seed per latte_trainer_forward (none is awaiting its seed)");
  hipStream_t st = (hipStream_t)stream;
  const int B = e->fwd_batch;
  int rc;
  // what launch_loss_grad + the scale pass leave for the built-in loss: the gradient of the sum / loss_divisor, in the loss-scaled domain
  if ((rc = launch_seed_scale(d_model_out, e->dmodel_out, e->loss_divisor, scaling_active(e) ? e->scaler : nullptr,
                              (size_t)B * e->F * e->Cout * e->H * e->H, st))) return rc;
  e->custom = 2;
  return arm_backward(e, e->fwd_y, B, st);
}

int latte_trainer_input_grad(latte_trainer_t* e, float* dx_out, void* stream) {
  if (!e || !dx_out) return fail(LATTE_ERR_INVALID, "trainer_input_grad: null argument");
  if (e->custom != 2 || e->next_stage != e->cfg.depth + 2)
    return fail(LATTE_ERR_STATE, "trainer_input_grad: valid after the last backward stage of a pass that latte_trainer_seed started");
  // e->dx is the gradient of the patch embed's output (block 0's LayerNorm backward left it), e->pix is free after the last stage
  return launch_patch_embed_dgrad(e->dx, P(e, e->rp.pe_w), dx_out, e->cur_batch * e->F, e->G, e->cfg.patch_size, e->Cin, e->D,
                                  e->pix, scaling_active(e) ? e->scaler : nullptr, (hipStream_t)stream);
}

// clip_grad_norm_ (utils.py:72-117) + AdamW (train.py:127) + update_ema (utils.py:191-200) on the bound flat buffers, then the
// half operand copies are re-packed.  norm_out: optional device float[2] = {total gradient norm, applied clip coefficient}.
int latte_trainer_optimizer_step(latte_trainer_t* e, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                 float clip_max_norm, int clip, float ema_decay, float* norm_out, void* stream) {
  if (!e || !e->base.p) return fail(LATTE_ERR_STATE, "optimizer_step: bind the parameter buffers first");
  if (step < 0) return fail(LATTE_ERR_INVALID, "optimizer_step: step counts from 1 (0: the trainer's own count of applied updates)");
  e->custom = 0;   // the weights and perhaps the loss scale change: a forward awaiting its seed is abandoned, the input gradient's time is over
  hipStream_t st = (hipStream_t)stream;
  int rc;
  const TrainedSet& s = trained(e);
  const size_t n = (size_t)s.total;
  if ((rc = launch_grad_norm(s.g, n, e->sumsq, clip_max_norm, clip, e->stats, e->scaler, st))) return rc;
  if (norm_out) LATTE_HIP(hipMemcpyAsync(norm_out, e->stats, sizeof(float) * 2, hipMemcpyDeviceToDevice, st));
  if ((rc = launch_adamw_ema(s.p, s.g, s.m1, s.v2, s.ema, n, lr, beta1, beta2, eps, weight_decay, step, ema_decay,
                             e->stats, e->scaler + 2, st))) return rc;
  return latte_trainer_sync_weights(e, stream);
}

// {loss scale, applied steps since it changed, applied optimiser updates, skipped updates, last call skipped, dynamic, growth interval,
// largest scale} -> host doubles (synchronises the device: logging / tests, not the step path)
int latte_trainer_scaler_state(latte_trainer_t* e, double* out8) {
  if (!e || !out8) return fail(LATTE_ERR_INVALID, "trainer_scaler_state: null argument");
  float h[8];
  LATTE_HIP(hipDeviceSynchronize());
  LATTE_HIP(hipMemcpy(h, e->scaler, sizeof(h), hipMemcpyDeviceToHost));
  for (int i = 0; i < 8; ++i) out8[i] = h[i];
  return LATTE_OK;
}

// The inverse of latte_trainer_scaler_state: the same eight fields back to the device (a resumed run: the live loss scale, its growth
// count, AdamW's bias-correction count = applied updates, the skip counters, the policy).  Not while a step is in flight.
int latte_trainer_set_scaler_state(latte_trainer_t* e, const double* in8) {
  if (!e || !in8) return fail(LATTE_ERR_INVALID, "trainer_set_scaler_state: null argument");
  if (step_in_flight(e)) return fail(LATTE_ERR_STATE, "trainer_set_scaler_state: a step is in flight");
  if (!pow2_in(in8[0], 1.0, 16777216.0) || !pow2_in(in8[7], in8[0], 16777216.0))
    return fail(LATTE_ERR_INVALID, "trainer_set_scaler_state: loss scale and largest scale must be powers of two in [1, 2^24], scale <= largest");
  for (int i = 1; i <= 4; ++i)
    if (!(in8[i] >= 0.0) || in8[i] > 16777216.0 || in8[i] != std::floor(in8[i]))
      return fail(LATTE_ERR_INVALID, "trainer_set_scaler_state: counters must be integers in [0, 2^24] (what a float counts exactly)");
  if (!(in8[6] >= 1.0) || in8[6] > 1e7) return fail(LATTE_ERR_INVALID, "trainer_set_scaler_state: growth interval must be in [1, 1e7]");
  float h[8];
  for (int i = 0; i < 8; ++i) h[i] = (float)in8[i];
  h[5] = in8[5] != 0.0 ? 1.0f : 0.0f;
  e->loss_scale = h[0];
  e->dynamic_scale = (int)h[5];
  e->growth_interval = h[6];
  LATTE_HIP(hipDeviceSynchronize());
  LATTE_HIP(hipMemcpy(e->scaler, h, sizeof(h), hipMemcpyHostToDevice));
  return LATTE_OK;
}

}  // extern "C"
