/*
 * latte_amd.h — C-ABI of the MI355X-native Latte denoising engine (liblatte_amd.so).
 *
 * The reference (Vchitect/Latte) exposes its hot path through Python protocols, not a native
 * plugin ABI; each entry point below names the reference interface it stands
 * in for.  Conventions:
 *   - plain C symbols, plain pointers and sizes, no torch / C++ types;
 *   - tensors are CALLER-OWNED DEVICE pointers in the reference layouts (contiguous);
 *     the engine owns only its packed weights and workspace;
 *   - every compute call takes a hipStream_t (as void*), is stream-ordered, never synchronises;
 *   - return value 0 = ok, non-zero = error; latte_last_error() gives the thread-local message
 *     (the reference raises Python exceptions / asserts: latte.py:38, gaussian_diffusion.py:278,290);
 *   - one engine per (device, host thread); no internal threads.
 */
#ifndef LATTE_AMD_H_
#define LATTE_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LATTE_OK 0
#define LATTE_ERR_INVALID 1   /* bad argument / unsupported configuration */
#define LATTE_ERR_HIP 2       /* a HIP runtime call failed                 */
#define LATTE_ERR_STATE 3     /* e.g. weights missing, batch > max_batch   */

/* compute dtype of the MFMA operands (accumulation, residual stream, LN/softmax statistics and the
 * sampler update are always fp32) */
#define LATTE_DTYPE_BF16 0
#define LATTE_DTYPE_F16 1

const char* latte_last_error(void);
/* "latte_amd <version> gfx950 ..." build identification */
const char* latte_version(void);

/* ------------------------------------------------------------------ schedule (host, fp64)
 * Replaces diffusion/__init__.py:10-47 create_diffusion -> respace.py:12-62 space_timesteps,
 * respace.py:73-87 SpacedDiffusion.__init__, gaussian_diffusion.py:153-201 table construction.
 * Integer outputs are bit-exact with the reference; fp64 tables are computed in the same order
 * of operations. */
typedef struct latte_schedule latte_schedule_t;

int latte_schedule_create(int diffusion_steps, const char* timestep_respacing /* "", "250", "ddim50", "10,15,20" */,
                          const char* noise_schedule /* "linear" | "squaredcos_cap_v2" */,
                          latte_schedule_t** out);
/* What the model predicts, as create_diffusion derives it (diffusion/__init__.py:32-45): predict_xstart -> START_X
 * instead of EPSILON; learn_sigma -> LEARNED_RANGE (model output 2C channels), else FIXED_LARGE / FIXED_SMALL
 * (sigma_small) with C output channels (gaussian_diffusion.py:289-313,323-328).  Default: 0, 1, 0. */
int latte_schedule_set_model_types(latte_schedule_t* s, int predict_xstart, int learn_sigma, int sigma_small);
void latte_schedule_destroy(latte_schedule_t* s);
int latte_schedule_num_timesteps(const latte_schedule_t* s);
/* SpacedDiffusion.timestep_map (respace.py:75,86): respaced index -> original timestep */
int latte_schedule_timestep_map(const latte_schedule_t* s, int64_t* out, int n);
/* name in {betas, alphas_cumprod, alphas_cumprod_prev, alphas_cumprod_next, sqrt_recip_alphas_cumprod,
 * sqrt_recipm1_alphas_cumprod, posterior_variance, posterior_log_variance_clipped,
 * posterior_mean_coef1, posterior_mean_coef2, log_betas, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod} */
int latte_schedule_table(const latte_schedule_t* s, const char* name, double* out, int n);

/* ------------------------------------------------------------------ engine
 * Replaces models/latte.py:204-255 Latte.__init__ (one of the Latte_models presets, :464-506). */
typedef struct latte_engine latte_engine_t;

typedef struct latte_model_config {
  int input_size;    /* latent H = W (image_size / 8)          latte.py:210 */
  int patch_size;    /* 2 | 4 | 8                                latte.py:211 */
  int in_channels;   /* 4                                        latte.py:212 */
  int hidden_size;   /* multiple of 128                          latte.py:213 */
  int depth;         /* even: spatial/temporal alternate         latte.py:214,345 */
  int num_heads;     /* head_dim = hidden/heads in {64, 72}      latte.py:215 */
  int mlp_hidden;    /* int(hidden * mlp_ratio)                  latte.py:169 */
  int num_frames;    /*                                          latte.py:217 */
  int num_classes;   /* label table has num_classes+1 rows       latte.py:131 */
  int learn_sigma;   /* out_channels = 2*in_channels if set      latte.py:226 */
  int extras;        /* 1 = unconditional, 2 = class-conditional, 78 = text embedding (latte.py:221,235-242) */
  int compute_dtype; /* LATTE_DTYPE_* for the MFMA operands */
} latte_model_config_t;

int latte_engine_create(const latte_model_config_t* cfg, int max_batch, latte_engine_t** out);
void latte_engine_destroy(latte_engine_t* e);

/* Engine options: "gemm_variant" (0 auto; 1-3 simple kernel 128x128 / 256x128 / 256x256; 4-6 ping-pong kernel
 * 256x128 / 256x192 / 256x256 tiles; 7-9 the persistent ping-pong kernel, same tiles; 10 / 11 the 12-wave
 * producer / consumer kernel, 256x192, two-segment / rolling schedule; 12 / 13 the small-M kernel, 128x144 tile with a
 * four-stage ring, DMA by the twelve MFMA waves / by four extra waves -- what the gated GEMMs of a 4096-row batch run on),
 * "gemm_variant_qkv" / "_proj" / "_fc1" / "_fc2" (the same, for one of the four GEMMs of the block only; tuning hook),
 * "gated_split_k" (small batches: 0 = the rule -- a gated GEMM with >= 64 K tiles whose tiles fill at most half of the
 * CUs, and which the 128x144 tile does not take, runs as 2..4 partial products + one reduction into the residual stream; 1 = never; 2..4 = force that many),
 * "gated_rmw_shape" (how the rolling 12-wave kernel requests the fp32 residual of a gated GEMM: 0 = one 16 x 16 accumulator
 * fragment, 16 rows x 64 B, per instruction; 1 = the default: the whole 128-byte line of a wave's span as 8 rows x 128 B; same bits),
 * "stream_policy" (bit mask, default 3: which once-used streams of a block are issued with the `nt` cache-policy hint so that they do not
 * displace the fp32 residual from the Infinity Cache -- bit 0 = fc1's hidden-activation stores, bit 1 = fc2's activation operand, bit 2 = the
 * fused attention kernel's output stores, bit 3 = the out-projection's activation operand; the large-batch kernels of unguided calls only,
 * every other kernel ignores it; the library's default applies only where the hidden activations and the residual together exceed the
 * 256 MiB cache, a value set here applies at every batch; same bits),
 * "fc2_temp_embed" (1 = the default: x + temp_embed of latte.py:357-358 is added by the first block's fc2 epilogue where fc2 runs on the
 * rolling 12-wave kernel; 0 = by the second block's first LayerNorm pass, as for every other fc2 kernel; same bits),
 * "fuse_qkv_attn" (bit 0: spatial blocks, bit 1: temporal blocks run the QKV projection and the attention core of
 * latte.py:48-70 as ONE kernel with q / k / v held in LDS -- csrc/qkv_attn.hip -- wherever the shape allows it: 256 tokens per
 * frame / 16 frames, head_dim 64 | 72; default 3, 0 = the separate qkv GEMM + attention kernels; values 0..31: bits 2, 3, 4 switch
 * OFF one default schedule feature of the fused kernel each -- the next unit's first operand tile fetched under the attention
 * phase, the attention-phase issue priority of wave group 0, the four-heads-per-XCD unit order of 16-head models (A/B hooks);
 * every setting gives the same bits),
 * "guided_split" (bits; guided calls -- latte_forward_with_cfg and the guided sample loop -- only; default 20 on f16 engines, ignored
 * beyond bits 0 / 1 on bf16 ones: bit 0 = the attention output
 * that feeds the out-projection, bit 1 = the LayerNorm-modulate output that feeds fc1 are carried as SPLIT operand pairs [hi | lo] (two
 * halves per value) against weights stored [W | W], i.e. those two linears run on K' = 2 K without rounding their activation operand.
 * The guidance combination of latte.py:394-398 amplifies the operand rounding that differs between the two halves; with f16 operands
 * the XL/2 guided output at trained-scale gates sits AT 1e-3 of the fp32 reference (0.6 - 1.2e-3), with the split pairs at 0.4 - 0.8e-3
 * for +31 % of the guided step at XL/2.  Bits 2 / 3 (round 6) carry the same two operands as f16 + an FP8
 * remainder (e4m3 of lo * 2^12, one byte per value) whose product with an fp8 copy of the weight is collected by a block-scaled fp8
 * MFMA pass behind the f16 K loop of the SAME GEMM launch: the same parity margin at half the extra MFMA time and a quarter of the
 * extra operand bytes; a bit-2 / 3 setting wins over bit 0 / 1 for its operand.  Bit 4 (round 6) carries fc1's operand as f16 + an FP4
 * remainder (e2m1 codes, two per byte, ONE E8M0 scale per row) -- the block-scaled MFMA runs fp4 x fp4 at twice the fp8 rate; it wins
 * over bits 1 / 3.  12 = both remainders as fp8 (+15 % per guided forward), 20 = the default (+11 %), 3 = round 5's f16 pairs (+30 %), all
 * at the same parity.  0 = the plain f16 operands of the unguided path.
 * Operands whose shape has no split form stay plain: latte_engine_get_option("guided_split_active") reports the bits the last
 * guided forward really used),
 * "seed" (Philox seed of the engine's own noise stream, used by latte_sample_loop when no noise
 * pointer is supplied; the reference draws torch.randn_like, gaussian_diffusion.py:413,555),
 * "train_timesteps" (default 1000: the number of timesteps the model was trained on, diffusion_steps of create_diffusion;
 * latte_sample_plan_loop refuses a plan row at or above it -- nothing else reads it). */
int latte_engine_set_option(latte_engine_t* e, const char* name, int64_t value);
/* Reads an option back (same names), or one of the read-only facts "guided_split_active" (bits of "guided_split" the last guided
 * forward ran with) and "guided_split_failed" (1 after an allocation for the split operands failed: guided calls then run plain). */
int latte_engine_get_option(const latte_engine_t* e, const char* name, int64_t* value);

/* Replaces nn.Module.load_state_dict (sample.py:62-64) for ONE tensor named by its reference
 * state_dict key (SURVEY.md §8(b) lists them: "blocks.3.attn.qkv.weight", "pos_embed", ...).
 * `data` is fp32, contiguous, reference shape; host pointer if on_device == 0, else device pointer.
 * The engine converts / packs into its own storage (caller may free `data` on return). */
int latte_engine_load_tensor(latte_engine_t* e, const char* key, const float* data, int64_t numel,
                             int on_device, void* stream);
/* Returns 0 when every tensor the configuration needs has been loaded; otherwise LATTE_ERR_STATE
 * and latte_last_error() names the first missing key (load_state_dict strict=True behaviour). */
int latte_engine_check_weights(latte_engine_t* e);
/* number of reference keys expected / name of the i-th one (for enumeration by the host shim) */
int latte_engine_num_keys(const latte_engine_t* e);
const char* latte_engine_key(const latte_engine_t* e, int i);

/* Timestep-embedding table of a schedule: out[i, :] = t_embedder(timestep_map[i]) for every respaced step i
 * (TimestepEmbedder, latte.py:84-123, through respace.py:125-130) -- [num_timesteps, hidden] fp32, device.  It depends on
 * nothing but the schedule and the weights, so the multi-GPU driver lets rank 0 compute it and broadcasts it over RCCL
 * (250 x 1152 x 4 B = 1.15 MB, the only payload collective of the sampling path); latte_engine_set_temb_table installs
 * a received table (copied) together with the schedule's timestep_map; latte_sample_loop uses it only for a schedule with
 * exactly that map (create_diffusion("250") and ("ddim250") both have 250 steps but different maps) and falls back to
 * computing its own otherwise.  Loading any t_embedder.* tensor uninstalls it.  table == NULL or s == NULL uninstalls. */
int latte_engine_temb_table(latte_engine_t* e, const latte_schedule_t* s, float* out, void* stream);
int latte_engine_set_temb_table(latte_engine_t* e, const latte_schedule_t* s, const float* table, void* stream);

/* Text-conditioned variant (extras == 78; latte.py:238-242,340-363): project a batch of text embeddings once,
 * text_embedding:[batch, 77*768] fp32 (device), Linear(SiLU(.)) -> [batch, D] kept inside the engine.  Every later
 * latte_forward / latte_forward_with_cfg / latte_sample_loop with the same batch conditions the 28 blocks on
 * t_emb + projected text and the final layer on t_emb alone (latte.py:372-373); y is ignored.  For guidance pass the
 * doubled batch [text, null text] (forward_with_cfg forwards text_embedding unchanged, latte.py:388). */
int latte_engine_set_text_embedding(latte_engine_t* e, const float* text_embedding, int batch, void* stream);

/* Latte.forward (latte.py:314-377).  x:[B,F,C,H,W] fp32, t: int64[B] ORIGINAL timesteps (device),
 * y: int64[B] labels (device) or NULL when extras == 1, out:[B,F,Cout,H,W] fp32. */
int latte_forward(latte_engine_t* e, const float* x, const int64_t* t, const int64_t* y, int batch,
                  float* out, void* stream);
/* Latte.forward_with_cfg (latte.py:379-398): x is the doubled batch [2b,...] whose first half is
 * duplicated internally; guidance on the first 4 channels; out:[2b,F,Cout,H,W]. */
int latte_forward_with_cfg(latte_engine_t* e, const float* x, const int64_t* t, const int64_t* y,
                           int batch /* = 2b */, float cfg_scale, float* out, void* stream);

/* ------------------------------------------------------------------ sampler update
 * Replaces gaussian_diffusion.py:254-336 p_mean_variance (EPSILON + LEARNED_RANGE, as built by
 * create_diffusion) followed by :380-421 p_sample (method 0 = "ddpm") or :517-564 ddim_sample
 * (method 1 = "ddim") or :566-602 ddim_reverse_sample (method 2 = "ddim_reverse": the deterministic step from level
 * `index` UP to level index + 1 with alphas_cumprod_next, whose last entry is 0 -- index num_timesteps-1 returns the
 * re-derived eps itself; eta must be 0 (:580, LATTE_ERR_INVALID otherwise) and noise is ignored).  `index` is the
 * respaced step i.  model_out:[B,F,2C,H,W]; noise may be NULL when no noise term is needed (ddim eta == 0, or
 * index == 0).  Outputs may alias x. */
#define LATTE_METHOD_DDPM 0
#define LATTE_METHOD_DDIM 1
#define LATTE_METHOD_DDIM_REVERSE 2
int latte_sampler_step(const latte_schedule_t* s, int method, int index, float eta, int clip_denoised,
                       const float* x, const float* model_out, const float* noise,
                       int batch, int frames, int channels, int hw /* H*W */,
                       float* sample_out, float* pred_xstart_out /* may be NULL */, void* stream);
/* The same step with the two caller hooks of gaussian_diffusion.py:
 *   denoised_fn (process_xstart, :316-321): call once with predict_only = 1 to get the raw x_start prediction in
 *     pred_xstart_out, apply the function, and pass its result as pred_xstart_in (it replaces the prediction BEFORE the
 *     clamp);
 *   cond_fn (:345-375; the hook sees ORIGINAL timesteps, respace.py:100-104): pass cond_grad = cond_fn(x, t).  DDPM
 *     adds variance * gradient to the mean (condition_mean), DDIM and the reverse step shift eps by
 *     sqrt(1 - alpha_bar) * gradient and re-derive pred_xstart from it (condition_score, :589-590).
 * Either pointer may be NULL. */
int latte_sampler_step_ex(const latte_schedule_t* s, int method, int index, float eta, int clip_denoised,
                          const float* x, const float* model_out, const float* noise, const float* pred_xstart_in,
                          const float* cond_grad, int predict_only, int batch, int frames, int channels, int hw,
                          float* sample_out, float* pred_xstart_out, void* stream);

/* ------------------------------------------------------------------ fused sampling loop
 * Replaces gaussian_diffusion.py:423-515 p_sample_loop / :604-684 ddim_sample_loop driving the
 * model through respace.py:125-130 _WrappedModel (index -> original timestep), i.e. the body of
 * sample/sample.py:100-107.  Runs steps start_index .. end_index (inclusive, descending; the full
 * chain is num_timesteps-1 .. 0).  x:[B,F,C,H,W] fp32 updated in place.  cfg_scale > 1 selects
 * forward_with_cfg semantics (batch is then the doubled batch, sample.py:88-94).
 * noise: NULL, or [n_steps][B,F,C,H,W] with noise[k] consumed by the k-th executed step (parity
 * runs feed the reference's draws).  trail_sample / trail_x0: NULL or [n_steps][B,F,C,H,W] receiving
 * every step's {"sample","pred_xstart"} (the *_progressive generators, :468,:637). */
int latte_sample_loop(latte_engine_t* e, const latte_schedule_t* s, int method, float eta,
                      int clip_denoised, float cfg_scale, float* x, const int64_t* y, int batch,
                      int start_index, int end_index, const float* noise,
                      float* trail_sample, float* trail_x0, void* stream);
/* The same loop with the model callable named explicitly: guided != 0 drives Latte.forward_with_cfg (doubled batch, first
 * half duplicated, eps_u + cfg_scale * (eps_c - eps_u)) for ANY cfg_scale -- the reference's method has no threshold
 * (latte.py:379-398); sample.py:51 only decides which callable it passes.  latte_sample_loop = guided iff cfg_scale > 1. */
int latte_sample_loop_ex(latte_engine_t* e, const latte_schedule_t* s, int method, float eta, int clip_denoised, int guided,
                         float cfg_scale, float* x, const int64_t* y, int batch, int start_index, int end_index,
                         const float* noise, float* trail_sample, float* trail_x0, void* stream);

/* ------------------------------------------------------------------ DDIM inversion
 * GaussianDiffusion.ddim_reverse_sample (gaussian_diffusion.py:566-602) stepped over respaced indices start_index ... end_index
 * ASCENDING, 0 <= start_index <= end_index < num_timesteps; the full chain is 0 ... num_timesteps-1 (the reference has no loop of
 * its own: this is `for i in range(T)` around its step).  Index i evaluates the model on (x, timestep_map[i]) -- the level being
 * LEFT -- and carries x from level i to level i + 1; level num_timesteps is pure noise (alphas_cumprod_next ends in 0), one level
 * above where ddim_sample_loop starts.  x:[B,F,C,H,W] fp32 updated in place.  The forward runs on the chain conditioning of
 * latte_sample_loop_ex; guided != 0 drives Latte.forward_with_cfg on the doubled batch for any cfg_scale, combined inside the
 * update kernel as there.  trail_sample / trail_x0: NULL or [n_steps][B,F,C,H,W] receiving every step's {"sample","pred_xstart"}
 * in execution order.  Deterministic: no noise is read and the engine's Philox offset is not touched.  Same preconditions and
 * error codes as latte_sample_loop_ex; nothing is launched when one fails.  Stream-ordered, no synchronisation. */
int latte_invert_loop(latte_engine_t* e, const latte_schedule_t* s, int clip_denoised, int guided, float cfg_scale, float* x,
                      const int64_t* y, int batch, int start_index, int end_index, float* trail_sample, float* trail_x0, void* stream);

/* ------------------------------------------------------------------ known-region sampling (prediction, interpolation, inpainting)
 * The replacement scheme of Video Diffusion Models / RePaint on latte_sample_loop_ex's chain (not in the reference): part of the clip is
 * held fixed and the rest is generated.  known: [B,F,C,H,W] fp32 clean latents; mask: [B,F,H,W] fp32, shared by the channels, 1 = known,
 * 0 = generated, values between mix linearly.  One blend at level abar is
 *   kn = sqrt(abar) known + sqrt(1 - abar) z  (known itself at abar = 1);   x <- m == 1 ? kn : (m == 0 ? x : m kn + (1 - m) x)
 * blend_start != 0: one blend at alphas_cumprod[start_index] before the first evaluation (the first segment of a chain).  Then for every
 * index i = start_index ... end_index and every repetition u = 1 ... resample: the forward and the step of latte_sample_loop_ex, a blend
 * at alphas_cumprod_prev[i] (the level the step has just reached; (1, 0) at i == 0, so the known part of the result IS `known`), and,
 * when u < resample and i > 0, the forward jump x <- sqrt(1 - betas[i]) x + sqrt(betas[i]) z back to level i (RePaint's resampling).
 * trail_sample / trail_x0: NULL or [n_steps][...], one slot per INDEX: x after the blend of the last repetition, and its pred_xstart.
 * noise: NULL, or DEVICE slabs of B*F*C*H*W floats consumed in this order: the start blend; then per repetition the step's own noise
 * (DDPM at i > 0, DDIM where sigma != 0), the blend's (i > 0), the jump's.  latte_known_chain_slabs is the one definition of that count.
 * NULL: every slab comes from the engine's Philox stream (option "seed") in the same order, the offset advancing by B*F*C*H*W per slab;
 * the blend draws inside its kernel.  On a guided (doubled) batch known and mask have the batch of x: the caller doubles them as it
 * doubles z.  LATTE_ERR_INVALID for resample < 1, a method other than DDPM / DDIM, H * W % 4 != 0, a NULL known or mask, plus the checks
 * of latte_sample_loop_ex; every check runs before the first launch.  Stream-ordered, no synchronisation. */
int latte_sample_loop_known(latte_engine_t* e, const latte_schedule_t* s, int method, float eta, int clip_denoised, int guided,
                            float cfg_scale, float* x, const int64_t* y, int batch, int start_index, int end_index, const float* known,
                            const float* mask, int resample, int blend_start, const float* noise, float* trail_sample, float* trail_x0,
                            void* stream);
/* The number of noise slabs latte_sample_loop_known consumes for these arguments.  Host only. */
int latte_known_chain_slabs(const latte_schedule_t* s, int method, float eta, int start_index, int end_index, int resample,
                            int blend_start, int64_t* n_slabs);
/* One blend (formula above) with (a, b) = (sqrt(abar), sqrt(1 - abar)) given; b == 0 reads no noise.  x, known, noise:
 * [B,F,C,H*W] (frames_inner = 0, the class-conditional engine's layout) or [B,C,F,H*W] (frames_inner = 1, text-to-video); mask [B,F,H*W].
 * noise == NULL with b != 0: z is drawn in the kernel, bit for bit what the engine's generator writes for a slab at (seed, offset).
 * hw % 4 != 0 is refused (16-byte accesses). */
int latte_known_blend(float* x, const float* known, const float* mask, const float* noise, uint64_t seed, uint64_t offset, float a,
                      float b, int batch, int frames, int channels, int hw, int frames_inner, void* stream);

/* ------------------------------------------------------------------ linear samplers as a plan (Euler, Euler-ancestral, Heun, DPM-Solver++)
 * The class-conditional / unconditional / text-embedding engine's counterpart of latte_t2v_guided_linear_loop (below): a whole chain of
 * any sampler whose update is a linear combination of the latents, the newest eps, up to three remembered outputs and fresh noise, as
 * ONE call.  plan: HOST doubles [n_evals][LATTE_PLAN_COLS] (latte_amd/schedulers.py: engine_plan()), narrowed to fp32 at launch:
 *   timestep (integral, ORIGINAL -- no latte_schedule_t is involved), in_scale, m_x, m_eps, c_x, c0, c1, c2, c3, c_noise, push (0 / 1),
 *   reserved (0)
 * Per row: Latte.forward (guided != 0: Latte.forward_with_cfg on the doubled batch, first half duplicated, for ANY cfg_scale) on
 * in_scale * x at the row's timestep, eps = the first C output channels (guided: uncond + cfg_scale (cond - uncond), rows b and
 * b + batch / 2 alike; the learned-sigma channels are dropped), then
 *   m0 = m_x x + m_eps eps;   x = c_x x + c0 m0 + c1 h1 + c2 h2 + c3 h3 + c_noise noise[row];   push: (h1, h2, h3) <- (m0, h1, h2)
 * x: [batch, F, C, H, W] fp32 in place.  The conditioning of the chain (t_embedder of every row's timestep, then the adaLN outputs in
 * chunks of <= 256 rows) is computed as latte_sample_loop_ex computes it; timesteps may repeat (Heun).
 * noise: DEVICE [n_evals][batch * F * C * H * W] fp32 (only rows with c_noise != 0 are read), or NULL = those rows draw from the
 * engine's Philox stream (option "seed"), as latte_sample_loop_ex does.  trail_sample: NULL or [n_evals][...] receiving x after every row.
 * LATTE_ERR_INVALID for a non-finite entry, a non-integral or negative timestep, a timestep at or above the trained range (option
 * "train_timesteps", default 1000), push outside {0, 1} or a non-zero reserved column, a c_j (j >= 1) that is non-zero before j rows
 * with push have run, an odd guided batch, a class-conditional model without y, n_evals > LATTE_PLAN_MAX_EVALS and H * W % 4 != 0;
 * LATTE_ERR_STATE for batch > max_batch and for a text-embedding model without latte_engine_set_text_embedding of `batch` rows.  Every
 * check runs before the first launch: x is untouched when one fails.  The ring of remembered outputs and the scaled model input are
 * taken from the engine's arena by the first call only.  Stream-ordered; the plan is consumed before the call returns. */
#define LATTE_PLAN_COLS 12   /* the columns above; their one C++ definition and every check of the table: csrc/plan.h (PlanCol, plan_check) */
#define LATTE_PLAN_MAX_EVALS 4096
int latte_sample_plan_loop(latte_engine_t* e, int guided, float cfg_scale, float* x, const int64_t* y, int batch, int n_evals,
                           const double* plan, const float* noise, float* trail_sample, void* stream);

/* ------------------------------------------------------------------ clips longer than num_frames: overlapping temporal windows
 * Temporal co-denoising (Gen-L-Video, MultiDiffusion along time; not in the reference): a long latent of L = total_frames >= F frames
 * (F = the model's num_frames / video_length) is denoised as ONE chain.  With 1 <= stride <= F the windows are
 *   W = ceil((L - F) / stride) + 1,   s_w = min(w * stride, L - F)   (the last window is pulled back so that it ends at L)
 * and every denoiser evaluation of a chain is
 *   gather   clips[g W + w] = x[g, s_w : s_w + F]          g over the batch rows as the loop sees them (the doubled batch when guided)
 *   forward  once, on the G W clips (labels repeated per window; a text context is installed per clip)
 *   merge    merged[g, f] = (sum over the windows covering f, ascending w, of out[g W + w, f - s_w]) / count(f), fp32, every output
 *            channel (the learned-sigma ones included); a frame one window covers is copied exactly
 * followed by the loop's own update kernel with frames = L: guidance, clipping, noise, trails and the history ring are unchanged.
 * Uniform weights, the same windows at every step, every clip of a call in one forward: G W <= max_batch.
 *
 * latte_window_plan: host only.  Writes the W starts (starts_out, `cap` entries; NULL: skipped) and the per-frame window counts
 * (counts_out, total_frames entries; NULL: skipped) and returns W >= 1, or -LATTE_ERR_INVALID (latte_last_error) for
 * total_frames < frames, stride outside 1 ... frames, or cap < W. */
int latte_window_plan(int total_frames, int frames, int stride, int* starts_out, int* counts_out, int cap);
/* The two kernels on their own (device pointers, fp32).  frames_inner = 0: x / merged [G, L, C, H*W], clips / out [G W, F, C, H*W] (the
 * class-conditional engine's layout, and the layout of BOTH engines' model outputs); 1: [G, C, L, H*W] and [G W, C, F, H*W]
 * (text-to-video latents).  hw % 4 != 0 and a bad window set are refused (LATTE_ERR_INVALID). */
int latte_window_gather(const float* x, float* clips, int groups, int total_frames, int frames, int stride, int channels, int hw,
                        int frames_inner, void* stream);
int latte_window_merge(const float* out, float* merged, int groups, int total_frames, int frames, int stride, int channels, int hw,
                       int frames_inner, void* stream);
/* latte_sample_loop_ex / latte_sample_plan_loop on x [batch, total_frames, C, H, W]; the noise rows and the trails have that shape too
 * (row k of the caller's noise is read at step k, else one engine draw of that size per step).  The conditioning rows are per clip.
 * After the checks of the plain loop, in its order: LATTE_ERR_INVALID for total_frames < num_frames, stride < 1, stride > num_frames
 * and H * W % 4 != 0, then LATTE_ERR_STATE for batch * W > max_batch (a text-embedding model needs batch * W installed rows).  Every
 * check runs before the first launch: x is untouched when one fails.  The clip and merged-output buffers are taken from the engine's
 * arena by the first call.  total_frames == num_frames gives the bits of the plain loop. */
int latte_sample_loop_windows(latte_engine_t* e, const latte_schedule_t* s, int method, float eta, int clip_denoised, int guided,
                              float cfg_scale, float* x, const int64_t* y, int batch, int start_index, int end_index, const float* noise,
                              float* trail_sample, float* trail_x0, int total_frames, int stride, void* stream);
int latte_sample_plan_loop_windows(latte_engine_t* e, int guided, float cfg_scale, float* x, const int64_t* y, int batch, int n_evals,
                                   const double* plan, const float* noise, float* trail_sample, int total_frames, int stride,
                                   void* stream);

/* ------------------------------------------------------------------ training path, forward evaluation
 * SURVEY.md section 8(f) rank 3, first slice: the loss VALUES of GaussianDiffusion.training_losses
 * (gaussian_diffusion.py:719-795, through SpacedDiffusion.training_losses respace.py:95-98; called by train.py:224-226)
 * on device tensors, one timestep per sample -- no gradients yet (the backward kernels are the next slice).
 *   latte_q_sample          gaussian_diffusion.py:216-229   x_t = sqrt(ab[t]) x_0 + sqrt(1 - ab[t]) noise
 *   latte_training_losses   given x_0, x_t, noise and the model's output on (x_t, timestep_map[t]):
 *                           mse = mean_flat((target - prediction)^2) (target = noise | x_0, :776-785),
 *                           vb  = _vb_terms_bpd with the frozen mean (:686-717,:760-774; KL in bits, decoder NLL at t == 0),
 *                           loss by loss_type: 0 MSE (mse [+ vb when the variance is learned]), 1 RESCALED_MSE (vb *
 *                           num_timesteps / 1000), 2 KL (vb), 3 RESCALED_KL (vb * num_timesteps)  (diffusion/__init__.py:22-27)
 * t: int64[batch] RESPACED indices (device); tensors [batch, frames, channels, hw] fp32 (model_out with 2 * channels when the
 * schedule's variance is learned); mse_out / vb_out may be NULL; workspace: latte_training_workspace_floats() floats. */
int latte_q_sample(const latte_schedule_t* s, const float* x_start, const float* noise, const int64_t* t, int batch,
                   int64_t numel_per_sample, float* x_t, void* stream);
int64_t latte_training_workspace_floats(int batch, int64_t numel_per_sample);
int latte_training_losses(const latte_schedule_t* s, int loss_type, const float* x_start, const float* x_t, const float* noise,
                          const float* model_out, const int64_t* t, int batch, int frames, int channels, int hw, float* workspace,
                          int64_t workspace_floats, float* mse_out, float* vb_out, float* loss_out, void* stream);

/* ------------------------------------------------------------------ likelihood evaluation (bits per dimension)
 * GaussianDiffusion.calc_bpd_loop (gaussian_diffusion.py:813-866): the variational bound of a batch of clips, term by term.
 * One RESPACED index is shared by the batch (:836); tensors are [batch, frames, channels, hw] fp32 on the device, model_out with
 * 2 * channels when the schedule's variance is learned (the layout latte_sampler_step reads).
 *   latte_prior_bpd     _prior_bpd (:797-811): KL(q(x_T | x_0) || N(0, I)) / ln 2 per sample -> out[batch].
 *   latte_bpd_terms     one column of the loop from x_0, x_t, the noise that made x_t and the model's output on
 *                       (x_t, timestep_map[index]), per sample b, written at [b * out_stride]:
 *                         vb         _vb_terms_bpd (:686-717): p_mean_variance (:254-336) for the schedule's ModelMeanType /
 *                                    ModelVarType, pred_xstart clamped to [-1, 1] BEFORE the posterior mean when clip_denoised
 *                                    (:316-330), KL against the true posterior in bits; the discretized decoder NLL at index 0
 *                         xstart_mse mean_flat((pred_xstart - x_0)^2)                                              (:850)
 *                         mse        mean_flat((eps - noise)^2), eps = _predict_eps_from_xstart(x_t, pred_xstart)  (:345-348,:851-852)
 *                       pred_xstart_out (may be NULL) receives the [batch, frames, channels, hw] prediction.
 *                       workspace: latte_bpd_workspace_floats(batch, frames * channels * hw) floats.  The sums are taken in a fixed
 *                       order without atomics: equal inputs give equal bits, and a sample's numbers do not depend on the batch.
 *   latte_bpd_loop      the whole loop inside the engine for respaced steps start_index ... end_index DESCENDING (:835): per step
 *                       noise (:837), q_sample (:838), the unguided Latte.forward on (x_t, timestep_map[i]) with the chain
 *                       conditioning latte_sample_loop_ex uses, then the terms.  vb / xstart_mse / mse are [batch, n_steps] with
 *                       n_steps = start_index - end_index + 1; column k is the k-th executed step, so a full chain has the
 *                       reference's column order (t = T-1 first, :854).  noise: [n_steps][batch, frames, channels, hw] or NULL
 *                       = one draw per step from the engine's Philox stream (option "seed"), as the sampling loop draws.
 *                       Class-conditional (y: int64[batch]) and unconditional models.  Stream-ordered, no synchronisation. */
int latte_prior_bpd(const latte_schedule_t* s, const float* x_start, int batch, int64_t numel_per_sample, float* out, void* stream);
int64_t latte_bpd_workspace_floats(int batch, int64_t numel_per_sample);
int latte_bpd_terms(const latte_schedule_t* s, int index, int clip_denoised, const float* x_start, const float* x_t, const float* noise,
                    const float* model_out, int batch, int frames, int channels, int hw, float* workspace, int64_t workspace_floats,
                    float* vb_out, float* xstart_mse_out, float* mse_out, int64_t out_stride, float* pred_xstart_out, void* stream);
int latte_bpd_loop(latte_engine_t* e, const latte_schedule_t* s, int clip_denoised, const float* x_start, const int64_t* y, int batch,
                   int start_index, int end_index, const float* noise, float* vb, float* xstart_mse, float* mse, void* stream);

/* ------------------------------------------------------------------ training step
 * Replaces the body of the reference's optimisation loop, train.py:197-236, for the class-conditional / unconditional Latte
 * (train.py:213-218 refuses text-to-video training):
 *     x_t = q_sample(x_0, t); terms = diffusion.training_losses(model, x_0, t, dict(y=y)); loss = terms["loss"].mean()
 *     loss.backward(); clip_grad_norm_(...); opt.step() [torch.optim.AdamW(lr, weight_decay=0), train.py:127]; update_ema(...)
 * on device buffers.  Parameters, gradients, AdamW moments and the EMA live in caller-owned FLAT fp32 device buffers of
 * latte_trainer_total_numel() floats; tensor i (reference named_parameters() order, latte.py:226-255, without the frozen
 * pos_embed / temp_embed tables, which latte_trainer_set_frozen supplies) occupies [offset_i, offset_i + numel_i) in reference
 * shape.  The data-parallel driver (train.py:125 DDP) all-reduces the gradient buffer between latte_trainer_forward_backward
 * and latte_trainer_optimizer_step; nothing here communicates.  MFMA operands are half copies (cfg->compute_dtype) of the fp32
 * masters, fp32 accumulation, fp32 residual stream / LayerNorm / softmax statistics / loss. */
typedef struct latte_trainer latte_trainer_t;
int latte_trainer_create(const latte_model_config_t* cfg, int max_batch, latte_trainer_t** out);
void latte_trainer_destroy(latte_trainer_t* e);
int latte_trainer_num_params(const latte_trainer_t* e);
const char* latte_trainer_param_key(const latte_trainer_t* e, int i);
int64_t latte_trainer_param_offset(const latte_trainer_t* e, int i);
int64_t latte_trainer_param_numel(const latte_trainer_t* e, int i);
int64_t latte_trainer_total_numel(const latte_trainer_t* e);
/* device pointers; ema may be NULL (no EMA update) */
int latte_trainer_bind(latte_trainer_t* e, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* ema);
int latte_trainer_set_frozen(latte_trainer_t* e, const float* pos_embed, const float* temp_embed, int on_device, void* stream);
/* re-packs the half operand copies from the fp32 masters (after the caller changed the parameter buffer, e.g. load_state_dict) */
int latte_trainer_sync_weights(latte_trainer_t* e, void* stream);
/* One micro-batch: forward with saved activations, loss terms, backward; the gradient of terms["loss"].mean() is ASSIGNED to the
 * bound gradient buffer (label-table rows are accumulated: the optimiser step leaves the buffer zeroed).  x_start / noise
 * [batch, F, C, H, W] fp32, t int64[batch] RESPACED indices, y int64[batch] labels AFTER the caller's label dropout
 * (LabelEmbedder.token_drop, latte.py:138-153: dropped labels = num_classes) or NULL, loss_type 0 MSE | 1 RESCALED_MSE,
 * terms_out device float [3][batch] = loss, mse, vb; model_out_copy optional [batch, F, C_out, H, W]. */
int latte_trainer_forward_backward(latte_trainer_t* e, const latte_schedule_t* s, int loss_type, const float* x_start, const float* noise,
                                   const int64_t* t, const int64_t* y, int batch, float* terms_out, float* model_out_copy, void* stream);
/* The same micro-batch in pieces, for a data-parallel driver that overlaps its gradient all-reduce with the backward (what
 * DistributedDataParallel's buckets do for train.py:125): latte_trainer_begin = forward + loss terms + d loss / d model_output;
 * then latte_trainer_backward_stage(k) for k = 0 .. latte_trainer_num_stages() - 1 IN ORDER (0 = final layer, 1 .. depth =
 * blocks depth-1 .. 0, depth + 1 = patch embed and the t / y embedders).  After stage k the contiguous slice
 * latte_trainer_stage_range(k) of the gradient buffer is final: the driver enqueues its collective on that slice (28 MB per
 * Latte-B/2 block, 96 MB per XL/2 block: large buckets, as the per-link-bound xGMI ring wants) while the next stages run.
 * `y` must stay alive until the last stage. */
int latte_trainer_begin(latte_trainer_t* e, const latte_schedule_t* s, int loss_type, const float* x_start, const float* noise,
                        const int64_t* t, const int64_t* y, int batch, float* terms_out, float* model_out_copy, void* stream);
int latte_trainer_num_stages(const latte_trainer_t* e);
int latte_trainer_stage_range(const latte_trainer_t* e, int stage, int64_t* offset, int64_t* numel);
int latte_trainer_backward_stage(latte_trainer_t* e, int stage, void* stream);
/* Custom losses: the same forward and the same staged backward with the loss between them in the CALLER's hands (LatteTrainer.forward
 * hangs the pair on torch.autograd).  States of a custom pass: idle -> [forward] -> awaiting seed -> [seed] -> backward in flight ->
 * [stage 0 .. num_stages - 1] -> done (input gradient available) -> idle at the next forward / begin.
 * latte_trainer_forward: the plain-mode forward with saved activations of model(x, t_model, y).  x fp32 [batch, F, C, H, W], the model
 * input, ALREADY noised (copied into the trainer: the patch embed's weight gradient reads it at the last stage); t_model int64 [batch]
 * device, the ORIGINAL timesteps the model sees (timestep_map[t] of a respaced schedule), not respaced indices; y labels after dropout
 * or NULL (extras == 1), alive until the last stage; model_out fp32 [batch, F, C_out, H, W].  A forward that no seed follows is simply
 * abandoned: the next latte_trainer_forward / latte_trainer_begin starts over.  Refused (LATTE_ERR_STATE): while a step is in flight
 * (between a begin / seed and the last stage), on a joint trainer inside its image pass, batch > max_batch, buffers unbound.
 * latte_trainer_seed: d_model_out fp32, model_out's shape: the caller's gradient of the SUM it wants minimised (for a mean over the
 * batch: 1 / batch is the caller's).  The trainer divides it by "loss_divisor" and multiplies it by the live loss scale -- exactly
 * what it does to the built-in loss's gradient -- so accumulation and loss scaling work unchanged; the stages and
 * latte_trainer_stage_range then run as after latte_trainer_begin, in the current assign / accumulate mode.  One seed per forward:
 * a second one is refused.  f16 operands: an arbitrary seed is multiplied by 2^14 (the default scale) on its way into f16 operands;
 * a seed orders of magnitude away from the built-in loss's 2 (pred - target) / numel needs "loss_scale" set accordingly, or bf16.
 * latte_trainer_input_grad: after the LAST stage of a pass that latte_trainer_seed started and before the next forward / begin /
 * optimizer step (which re-packs the weights and may change the loss scale; it also abandons a forward that awaits its seed):
 * dx_out fp32 [batch, F, C, H, W] = d / d x of the seeded sum (divided by "loss_divisor" like every gradient), already out of the
 * loss-scaled domain.  One pass over the token gradient (csrc/train_fin.hip: patch_embed_dgrad_kernel). */
int latte_trainer_forward(latte_trainer_t* e, const float* x, const int64_t* t_model, const int64_t* y, int batch, float* model_out,
                          void* stream);
int latte_trainer_seed(latte_trainer_t* e, const float* d_model_out, void* stream);
int latte_trainer_input_grad(latte_trainer_t* e, float* dx_out, void* stream);
/* Joint image-video training (train_with_img.py:214-241, models/latte_img.py:361-399, `use_image_num: N` of the *_img_train.yaml
 * configs): every sample carries F video frames and N single image frames.  LatteIMG has exactly Latte's parameters, its image
 * frames never meet the video frames (spatial blocks treat every frame alone, temporal blocks see x[:, :F]) and mean_flat runs over
 * all F + N frames of a sample, whose t they share, so for loss, mse and vb
 *     terms_b = (F terms_video_b + sum_n terms_image_{b,n}) / (F + N)
 *     grad loss.mean() = F / (F + N) grad mean_b(loss_video_b) + N / (F + N) grad mean_{b,n}(loss_image_{b,n})
 * and a joint micro-batch is the plain step on the video frames plus an IMAGE PASS: the same network on batch * N one-frame
 * pseudo-samples (t_b, label y_image[b][n]) with the temporal blocks off -- only the even blocks and the final layer run, no
 * temp_embed, the odd blocks' gradient slices are not touched -- whose gradient writers add to what the video pass wrote.
 * latte_trainer_create_joint: a trainer whose per-sample buffers hold max_batch * max_image_num pseudo-samples; max_image_num = 0 is
 * latte_trainer_create; max_image_num > num_frames (the image pass runs in the video pass's row buffers) and tokens per frame % 64
 * != 0 are refused.  Through the plain entry points such a trainer computes what one of latte_trainer_create does, bit for bit.
 * latte_trainer_begin_joint: x_start / noise / model_out_copy [batch, F + N, C(_out), H, W], y_image int64 [batch, N] after label
 * dropout (ignored without a label table); runs the video pass completely (forward and every stage) in the current assign /
 * accumulate mode with loss weight F / (F + N) (it multiplies into "loss_divisor"), then the image pass's forward in accumulate
 * mode with weight N / (F + N), and writes the combined terms_out [3][batch] (undivided, as ever).  The image pass's stages are the
 * caller's: latte_trainer_backward_stage(k), k = 0 .. num_stages - 1; after stage k the slice latte_trainer_stage_range(k) is
 * final (the odd blocks' stages launch nothing).  `y` and `y_image` must stay alive until the last stage.
 * latte_trainer_forward_backward_joint = latte_trainer_begin_joint + every stage. */
int latte_trainer_create_joint(const latte_model_config_t* cfg, int max_batch, int max_image_num, latte_trainer_t** out);
int latte_trainer_begin_joint(latte_trainer_t* e, const latte_schedule_t* s, int loss_type, const float* x_start, const float* noise,
                              const int64_t* t, const int64_t* y, const int64_t* y_image, int batch, int use_image_num, float* terms_out,
                              float* model_out_copy, void* stream);
int latte_trainer_forward_backward_joint(latte_trainer_t* e, const latte_schedule_t* s, int loss_type, const float* x_start,
                                         const float* noise, const int64_t* t, const int64_t* y, const int64_t* y_image, int batch,
                                         int use_image_num, float* terms_out, float* model_out_copy, void* stream);
/* clip_grad_norm_ (utils.py:72-117: total 2-norm, g *= min(max_norm / (norm + 1e-6), 1) when clip != 0) + AdamW + update_ema
 * (utils.py:191-200) on the bound buffers.  `step` = 0 (what LatteTrainer passes): AdamW's bias correction uses the trainer's own count
 * of APPLIED updates (what torch.optim.AdamW does: a fresh optimiser state starts at 1 even when the training-step counter continues
 * from a checkpoint, train.py:195-196 -- the count that drives clipping and logging stays with the caller; a skipped update does not
 * advance it).  `step` >= 1: the caller supplies the bias-correction step -- valid only while NO update is ever skipped (the caller cannot
 * see a skip without latte_trainer_scaler_state; after one, a caller-side count runs ahead of the moments' age, which differs from
 * GradScaler + torch.optim.AdamW): with loss scaling on, pass 0.  A NON-FINITE gradient norm
 * (overflow of the loss-scaled f16 backward or of an f16 activation; impossible in the reference's fp32 range) skips the update:
 * parameters, moments and EMA stay untouched, the gradients are zeroed, norm_out reports the non-finite norm with coefficient 0.
 * norm_out: optional device float[2] = {norm, applied coefficient} */
/* "loss_scale" (a power of two in [1, 2^24]): d loss / d model_output is multiplied by it before the backward and every finished
 * gradient slice by its inverse, so that the half-precision gradient operands stay inside the operand type's range.  Default: 1 with
 * bf16 operands, 16384 with f16 operands -- f16's 10 mantissa bits are the precision class of the TF32 matmuls the reference trains
 * with (train.py:12-14 allow_tf32), bf16 has 7; the reference itself needs no scaling because it keeps fp32 ranges.
 * "dynamic_loss_scale" (0 / 1; default 1 with f16, 0 with bf16): a skipped update halves the scale (floor 1), and
 * "loss_scale_growth_interval" (default 2000) applied updates in a row double it (cap max(initial scale, 2^16)) -- all on the
 * device, no host round trip.  Setting "loss_scale" restarts from that value.
 * "fuse_gelu" (default 1): the MLP's GELU passes inside the fc1 forward / fc2 input-gradient GEMM epilogues.
 * "fuse_small" (default 1, round 6b): the step's tiny launches folded (csrc/train_fin.hip) -- one finalize launch per block
 * stage, the gated residual's backward on the LayerNorm backward's pass, gated add + next LayerNorm in one forward pass, fc1 / qkv
 * bias gradients on the weight-gradient launch, one weight-pack launch; 0 = the separate launches (A/B tests); refused while a
 * step is in flight (between latte_trainer_begin and the last backward stage).  Gradients agree with the separate path to 2e-4.
 * "grad_accumulate" (default 0): 1 makes every kernel that writes into the bound gradient buffer ADD to what is there, in its own
 * store (gradient accumulation, train.py:222-236: micro-batch 1 of a window runs with 0 -- no clear needed --, the others with 1;
 * each micro-batch leaves the loss-scaled domain by the current scale as it is written, and a non-finite value of any micro-batch
 * survives the sum, so the skip rule of latte_trainer_optimizer_step holds unchanged).  "loss_divisor" (default 1, in [1, 65536]):
 * d loss.mean() is divided by it (`loss / gradient_accumulation_steps`); the reported terms stay undivided.  Both are refused
 * while a step is in flight; with both at their defaults the step is bit-identical to a trainer that never heard of them. */
int latte_trainer_set_option(latte_trainer_t* e, const char* name, double value);
/* out8 (host) = {loss scale, applied updates since it changed, applied updates in total, skipped updates, last call skipped (0/1),
 * dynamic (0/1), growth interval, largest scale}.  Synchronises the device: for logging and tests, not for the step path. */
int latte_trainer_scaler_state(latte_trainer_t* e, double* out8);
/* The inverse: in8 (host, the same eight fields) goes back to the device -- what a resumed run needs besides the five flat buffers:
 * the live loss scale and its growth count, the count of applied updates (AdamW's bias-correction step), the skip counters and the
 * policy.  Scales must be powers of two in [1, 2^24], counters integers in [0, 2^24].  Synchronises; refused while a step is in flight. */
int latte_trainer_set_scaler_state(latte_trainer_t* e, const double* in8);
int latte_trainer_optimizer_step(latte_trainer_t* e, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                 float clip_max_norm, int clip, float ema_decay, float* norm_out, void* stream);
/* LoRA fine-tuning (DESIGN.md 4.4 "LoRA"; not part of the reference): every targeted block linear y = x W^T + b, W [N, K], runs with
 * W_eff = W + s B A -- A [rank, K], B [N, rank], s = alpha / rank.  The whole base (W, b and every other parameter) is frozen; only A
 * and B are trained.  The forward and the input gradients run on the merged half operand copies (the step-end pack writes
 * half(W + s B A), one rounding), the adapter gradients come from dY, x and the adapters themselves (csrc/train_lora.hip).
 * latte_trainer_lora_enable: rank in {4, 8, 16, 32} (64 is refused: its step measured slower than the full step), alpha > 0, target_mask a non-empty subset of qkv = 1 | proj = 2 | fc1 = 4 |
 * fc2 = 8.  Legal once, BEFORE the buffers are bound; refused (LATTE_ERR_STATE) afterwards or while a step is in flight.
 * The adapters are a trained set of their own -- five caller-owned flat fp32 buffers and the table that lays them out, exactly what
 * latte_trainer_param_* and latte_trainer_bind are for the base -- read through latte_trainer_lora_param_*: keys
 * blocks.{i}.attn.qkv.lora_A / .lora_B, blocks.{i}.attn.proj.*, blocks.{i}.mlp.fc1.*, blocks.{i}.mlp.fc2.* in block order, 16-byte
 * aligned tensors.  latte_trainer_bind_lora replaces latte_trainer_bind (which is then refused): base_params is the plain trainer's
 * parameter buffer, read only; there are no base gradient, moment or EMA buffers.  In LoRA mode every writer of a base gradient is
 * skipped (one that is reached anyway ends its stage with LATTE_ERR_STATE before any launch), latte_trainer_sync_weights packs the
 * merged weights, latte_trainer_optimizer_step runs norm / clip / AdamW / EMA over the adapter buffers, latte_trainer_stage_range
 * reports slices of the ADAPTER gradient buffer (block stages: the block's adapters; the two other stages: empty), and
 * latte_trainer_input_grad, gradient accumulation, joint steps and custom losses work as before.
 * latte_trainer_lora_merge: fp32 W + s B A of every targeted weight -- the pack's arithmetic in its order, so half() of it is the
 * operand the LoRA trainer ran with -- into params_out, a copy of the flat parameter buffer (or the bound buffer itself, which ends the
 * LoRA run: a later sync would add the adapters again); lora_params NULL = the bound adapters, else e.g. their EMA.  Synchronises. */
int latte_trainer_lora_enable(latte_trainer_t* e, int rank, float alpha, int target_mask);
int latte_trainer_lora_num_params(const latte_trainer_t* e);
const char* latte_trainer_lora_param_key(const latte_trainer_t* e, int i);
int64_t latte_trainer_lora_param_offset(const latte_trainer_t* e, int i);
int64_t latte_trainer_lora_param_numel(const latte_trainer_t* e, int i);
int64_t latte_trainer_lora_total_numel(const latte_trainer_t* e);
int latte_trainer_bind_lora(latte_trainer_t* e, float* base_params, float* lora_params, float* lora_grads, float* lora_exp_avg,
                            float* lora_exp_avg_sq, float* lora_ema);
int latte_trainer_lora_merge(latte_trainer_t* e, const float* lora_params, float* params_out, void* stream);

/* ------------------------------------------------------------------ VAE decoder
 * Replaces diffusers.AutoencoderKL (sample/sample.py:69 from_pretrained, :113-115 vae.decode(z / 0.18215).sample;
 * sample_ddp.py:90,165-168) for the stabilityai/sd-vae-ft-* architecture: latent_channels 4,
 * block_out_channels (128, 256, 512, 512), layers_per_block 2, norm_num_groups 32, SiLU.  diffusers is not vendored
 * in the reference: the restated algorithm and its parity status are in oracle/vae_oracle.py. */
typedef struct latte_vae latte_vae_t;
/* latent_size: H = W of the latent (multiple of 16); max_frames: largest N of one decode call; compute_dtype: LATTE_DTYPE_F16
 * only (MFMA operands f16 as in the reference's fp16 decode, residual stream fp32) */
int latte_vae_create(int latent_size, int max_frames, int compute_dtype, latte_vae_t** out);
/* diffusers.AutoencoderKLTemporalDecoder (sample/sample_t2x.py:31-32, pipeline_latte.py:779-798: vae.decode(z[i : i + 14],
 * num_frames=n).sample): the same handle type and entry points; every resnet is a SpatioTemporalResBlock (keys
 * "...resnets.N.spatial_res_block.*", "...temporal_res_block.*" with Conv3d weights [C, C, 3, 1, 1], "...time_mixer.mix_factor"),
 * there is no post_quant_conv, and "decoder.time_conv_out.*" follows conv_out.  ONE latte_vae_decode call decodes ONE chunk:
 * its n_frames frames are the temporal extent (max_frames >= the chunk length).  Restated from memory of diffusers 0.24.0:
 * parity unpinned (oracle/vae_temporal_oracle.py). */
int latte_vae_create_temporal(int latent_size, int max_frames, int compute_dtype, latte_vae_t** out);
void latte_vae_destroy(latte_vae_t* v);
/* load_state_dict for ONE tensor named by its diffusers key ("decoder.up_blocks.2.resnets.0.conv1.weight",
 * "post_quant_conv.bias", ...); fp32, reference shape; a decoder handle does not accept encoder.* / quant_conv.* keys (an encoder
 * handle accepts only those). */
int latte_vae_num_keys(const latte_vae_t* v);
const char* latte_vae_key(const latte_vae_t* v, int i);
int latte_vae_load_tensor(latte_vae_t* v, const char* key, const float* data, int64_t numel, int on_device,
                          void* stream);
int latte_vae_check_weights(latte_vae_t* v);
/* vae.decode(z * z_scale).sample: z [N,4,h,w] fp32 (device, the layout sample.py:112 produces), z_scale = 1/0.18215
 * folds the caller's division.  out_mode 0: fp32 [N,3,8h,8w] (the reference's `.sample`); out_mode 1: uint8
 * [N,8h,8w,3] = ((x*0.5+0.5)*255+0.5).clamp(0,255) of sample.py:122 fused into the last convolution. */
int latte_vae_decode(latte_vae_t* v, const float* z, int n_frames, float z_scale, int out_mode, void* out,
                     void* stream);
/* Measurement hook beside latte_profile_forward: ONE decode with a HIP event behind every launch.  ms_out[c] / launches_out[c]
 * (n >= 5 entries) per kernel class c: 0 = conv3x3 (implicit GEMM on the MFMA pipe), 1 = GroupNorm statistics, 2 = GroupNorm
 * apply (+ SiLU), 3 = mid-block attention and the 1x1 shortcut GEMMs, 4 = the small kernels (post_quant_conv, conv_in, conv_out,
 * fp32 -> half copies).  Synchronises the stream; bench.py's `vae_decode.roofline_table` is built from it. */
int latte_vae_profile_decode(latte_vae_t* v, const float* z, int n_frames, float z_scale, int out_mode, void* out, float* ms_out,
                             int* launches_out, int n, void* stream);

/* ------------------------------------------------------------------ VAE encoder
 * diffusers.AutoencoderKL.encode (the reference's training step, train.py:204-211: vae.encode(x).latent_dist.sample().mul_(0.18215))
 * for the same sd-vae-ft architecture: the same handle type, so latte_vae_num_keys / key / load_tensor / check_weights / destroy apply;
 * its slots are the diffusers keys "encoder.*" and "quant_conv.*".  image_size: H = W of the frames, a multiple of 128, at most 512
 * (latent h = image_size / 8); max_frames: largest N of one encode call; compute_dtype LATTE_DTYPE_F16 only.  latte_vae_decode on an
 * encoder handle, and latte_vae_encode on a decoder handle, return LATTE_ERR_INVALID.  Parity with diffusers unpinned
 * (tests/vae_encoder_reference.py restates it). */
int latte_vae_create_encoder(int image_size, int max_frames, int compute_dtype, latte_vae_t** out);
/* x: in_mode 0 fp32 NCHW [N, 3, H, W] in [-1, 1]; in_mode 1 uint8 NHWC [N, H, W, 3] read as x / 127.5 - 1.  out (fp32 NCHW):
 * out_mode 0 the moments [N, 8, h, w] (DiagonalGaussianDistribution.parameters: mean = channels 0..3, logvar = 4..7);
 * 1 mean * scale [N, 4, h, w] (.mode()); 2 (mean + exp(0.5 clamp(logvar, -30, 20)) noise) * scale [N, 4, h, w] (.sample() with the
 * caller's N(0, 1) noise [N, 4, h, w]; noise may be NULL otherwise). */
int latte_vae_encode(latte_vae_t* v, const void* x, int n_frames, int in_mode, const float* noise, float scale, int out_mode, float* out,
                     void* stream);
/* The posterior on moments [n, 8, hw] already encoded -> out [n, 4, hw]: what 1 mean * scale (mode), 2 (mean + std noise) * scale
 * (sample, noise [n, 4, hw]), 3 logvar (clamped to [-30, 20]), 4 std = exp(0.5 logvar), 5 var = exp(logvar); scale applies to 1 and 2. */
int latte_vae_posterior(const float* moments, const float* noise, int n, int hw, float scale, int what, float* out, void* stream);
/* Training batches from STORED moments: out[r] from row rows[r] of store, DEVICE [n_rows, 8, hw] fp32 (store_half = 0) or f16 (1) in
 * the out_mode 0 layout of latte_vae_encode, computed in fp32.  what keeps the codes of latte_vae_posterior, plus 0: 0 the moments
 * themselves, out [n_out, 8, hw] (gather + upcast); 1 mean * scale and 2 (mean + exp(0.5 clamp(logvar, -30, 20)) noise) * scale, out
 * [n_out, 4, hw] -- the device function of latte_vae_posterior, so the two agree bit for bit on the gathered rows.  noise: DEVICE
 * [n_out, 4, hw], or NULL with what == 2: the noise is drawn in the kernel, element i of out taking the normal the engine's generator
 * writes at i of a slab at (seed, offset) (as latte_known_blend); seed == LATTE_SEED_NONE then says "no seed either" and is refused.
 * rows: a HOST array of n_out entries, each checked against [0, n_rows) BEFORE anything is launched -- a bad entry returns
 * LATTE_ERR_INVALID, latte_last_error() names it, and out is untouched -- and handed to the kernel by value, 256 per launch: the call
 * keeps no reference to it, needs no staging buffer and does not synchronise.  LATTE_ERR_INVALID also for hw % 8 != 0 (16-byte accesses
 * of eight halves), n_out <= 0, a NULL store / rows / out, and a store, noise or out that is not 16-byte aligned. */
#define LATTE_SEED_NONE UINT64_MAX
int latte_moment_sample(const void* store, int store_half, int64_t n_rows, int hw, const int64_t* rows, int n_out, const float* noise,
                        uint64_t seed, uint64_t offset, float scale, int what, float* out, void* stream);
/* latte_vae_profile_decode for the encoder: the same five kernel classes (4 = conv_in, conv_out + posterior, fp32 -> half copies). */
int latte_vae_profile_encode(latte_vae_t* v, const void* x, int n_frames, int in_mode, const float* noise, float scale, int out_mode, float* out,
                             float* ms_out, int* launches_out, int n, void* stream);

/* ------------------------------------------------------------------ video preprocessing in front of the encoder
 * The reference's per-item frame pipeline (datasets/__init__.py:13-76, datasets/video_transforms.py) as one launch:
 * ToTensorVideo -> [RandomHorizontalFlipVideo] -> UCFCenterCropVideo | CenterCropResizeVideo -> Normalize(0.5, 0.5).
 * kind: LATTE_VT_NONE (taichi) flip and normalise only, output size = source size (out_h = out_w = 0 or the source size);
 * LATTE_VT_UCF_CENTER_CROP (ffs, ucf101) resize_scale by out_h / min(src_h, src_w) -- torch's scale_factor form: intermediate size
 * floor(dim * scale), source coordinates from the GIVEN scale's reciprocal -- then center_crop to out_h x out_w, which fails with the
 * reference's "height and width must be no smaller than crop_size" when the intermediate is smaller;
 * LATTE_VT_CENTER_CROP_RESIZE (sky) center_crop_using_short_edge then bilinear resize to out_h x out_w (coordinate scale in / out). */
#define LATTE_VT_NONE 0
#define LATTE_VT_UCF_CENTER_CROP 1
#define LATTE_VT_CENTER_CROP_RESIZE 2
/* What the host works out for one (kind, source size, output size) and the kernel consumes: output pixel (oy, ox) is intermediate
 * pixel (oy + crop_i, ox + crop_j) of a mid_h x mid_w bilinear resize (align_corners = False, coordinate scales scale_h / scale_w)
 * of the reg_h x reg_w region at (reg_y, reg_x) of the -- flipped, when asked -- source frame. */
typedef struct latte_video_plan {
  int kind, src_h, src_w, out_h, out_w;
  int mid_h, mid_w, crop_i, crop_j;
  int reg_y, reg_x, reg_h, reg_w;
  float scale_h, scale_w;
} latte_video_plan;
/* Host only (no device needed). */
int latte_video_transform_plan(int kind, int src_h, int src_w, int out_h, int out_w, latte_video_plan* plan);
/* src: uint8 NHWC [n, src_h, src_w, 3] (device); flip: one byte per frame (device), non-zero = that frame is mirrored left-right
 * BEFORE the crop and resize, as the reference does, or NULL; out: fp32 NCHW [n, 3, out_h, out_w] in [-1, 1] (device) =
 * ((bilinear blend of x / 255) - 0.5) / 0.5 in torch's order of operations -- the in_mode 0 input of latte_vae_encode. */
int latte_video_transform(const uint8_t* src, int n, int src_h, int src_w, int kind, int out_h, int out_w, const uint8_t* flip, float* out,
                          void* stream);

/* ------------------------------------------------------------------ LatteT2V denoiser (Latte-1 text-to-video)
 * LatteT2V.forward, /root/reference/models/latte_t2v.py:677-941 (constructor :475-672).
 * PixArt-alpha style blocks with norm_type "ada_norm_single", attention_bias = True, activation_fn "gelu-approximate",
 * norm_elementwise_affine = False, norm_eps 1e-6 -- the configuration Latte-1 ships; weights by the reference's
 * state-dict keys (to_q / to_k / to_v are packed into one fused GEMM on load).  The diffusers 0.24.0 leaves the reference
 * imports are restated, not vendored: parity is pinned against the reference's own file only (oracle/latte_t2v_oracle.py). */
typedef struct latte_t2v latte_t2v_t;
typedef struct {
  int num_attention_heads, attention_head_dim;   /* inner dim = heads * head_dim (16 x 72 = 1152) */
  int in_channels, out_channels;                 /* 4, 8 (learned sigma) */
  int num_layers;                                /* 28 spatial + 28 temporal blocks */
  int sample_size, patch_size;                   /* latent side (64 for 512 px), 2 */
  int cross_attention_dim, caption_channels;     /* 1152 (= inner dim), 4096 (T5-XXL features) */
  int video_length;                              /* frames, 16 */
  int max_text_tokens;                           /* workspace for the text tokens of one sample (120) */
  int compute_dtype;                             /* LATTE_DTYPE_BF16 | LATTE_DTYPE_F16 */
} latte_t2v_config_t;
int latte_t2v_create(const latte_t2v_config_t* cfg, int max_batch, latte_t2v_t** out);
void latte_t2v_destroy(latte_t2v_t* e);
int latte_t2v_num_keys(const latte_t2v_t* e);
const char* latte_t2v_key(const latte_t2v_t* e, int i);
int latte_t2v_load_tensor(latte_t2v_t* e, const char* key, const float* data, int64_t numel, int on_device, void* stream);
int latte_t2v_check_weights(latte_t2v_t* e);
/* "fuse_qkv_attn": as latte_engine_set_option (the to_q | to_k | to_v projection of attn1 and its attention core as one kernel
 * wherever the sequences are 256 tokens of a frame / 16 frames of a token; default 3; every setting gives the same bits). */
int latte_t2v_set_option(latte_t2v_t* e, const char* name, int64_t value);
/* x:[B,C,F,H,W] fp32 (channels before frames, latte_t2v.py:729), t: int64[B], encoder_hidden_states:[B,n_text,caption_channels]
 * fp32, encoder_attention_mask:[B,n_text] fp32 1 = keep / 0 = padded, or NULL; out:[B,out_channels,F,H,W] fp32.  All device
 * pointers.  enable_temporal_attentions = 0 skips the temporal blocks (latte_t2v.py:867). */
int latte_t2v_forward(latte_t2v_t* e, const float* x, const int64_t* t, const float* encoder_hidden_states,
                      const float* encoder_attention_mask, int batch, int n_text, int enable_temporal_attentions, float* out,
                      void* stream);

/* Chain-level text context: the caption projection, the cross-attention K|V of every spatial block and the mask bias depend on
 * the text only; latte_t2v_set_text computes them once ([batch, n_text, caption_channels] fp32, mask [batch, n_text] or NULL)
 * and latte_t2v_forward with encoder_hidden_states == NULL / latte_t2v_guided_ddim_loop reuse them for every step.  Loading
 * a tensor uninstalls the context; encoder_hidden_states == NULL here uninstalls it too. */
int latte_t2v_set_text(latte_t2v_t* e, const float* encoder_hidden_states, const float* encoder_attention_mask, int batch,
                       int n_text, void* stream);
/* The denoising loop of LattePipeline.__call__ (sample/pipeline_latte.py:700-760) for the classifier-free-guidance case with
 * a DDIM scheduler at eta = 0, entirely inside the engine: per step the transformer on the guidance pair (the latents are
 * duplicated inside, :725), noise_pred = uncond + s (text - uncond) (:748-749), the learned-sigma half dropped (:752-753),
 * and DDIMScheduler.step (x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t); x' = sqrt(a_prev) x0 + sqrt(1 - a_prev) eps).
 * x: [samples, C, F, H, W] fp32, updated in place; the installed text context must hold 2 * samples rows ordered
 * [negative prompts | prompts] (:647).  timesteps / alpha_t / alpha_prev: HOST arrays of n_steps entries (the scheduler's
 * timesteps and alphas_cumprod at t and at the previous timestep, final_alpha_cumprod for the last step). */
int latte_t2v_guided_ddim_loop(latte_t2v_t* e, float* x, int samples, int n_steps, const int64_t* timesteps,
                               const double* alpha_t, const double* alpha_prev, float guidance_scale,
                               int enable_temporal_attentions, void* stream);
/* latte_t2v_guided_ddim_loop with a known part held fixed (the scheme of latte_sample_loop_known, without resampling): one blend
 * (latte_known_blend, frames_inner = 1) at alpha_t[0] before step 0 and one at alpha_prev[k] after step k; the last step blends with
 * (1, 0) whatever alpha_prev is, so the known part of the result is `known`.  known: [samples, C, F, H, W] fp32 clean latents; mask:
 * [samples, F, H, W] fp32; noise: DEVICE [n_steps][samples * C * F * H * W] fp32, required (this engine draws none): slab 0 for the
 * blend before step 0, slab k + 1 for the blend after step k.  Preconditions as latte_t2v_guided_ddim_loop, plus LATTE_ERR_INVALID for
 * H * W % 4 != 0, a NULL known / mask / noise and an alpha out of range; nothing is launched when a check fails. */
int latte_t2v_guided_ddim_loop_known(latte_t2v_t* e, float* x, int samples, int n_steps, const int64_t* timesteps,
                                     const double* alpha_t, const double* alpha_prev, float guidance_scale, const float* known,
                                     const float* mask, const float* noise, int enable_temporal_attentions, void* stream);
/* The same guided loop for every sampler whose update is a linear combination of the latents, the newest guided model output, up to
 * three remembered outputs and fresh noise (latte_amd/schedulers.py: Euler, Euler-ancestral, Heun, DPM-Solver++ multistep build the
 * table with engine_plan()).  plan: HOST doubles [n_evals][LATTE_T2V_PLAN_COLS], one row per denoiser evaluation, narrowed to fp32 at
 * launch like the DDIM loop's coefficients:
 *   timestep (integral), in_scale, m_x, m_eps, c_x, c0, c1, c2, c3, c_noise, push (0 / 1), reserved (0)
 * Per row: the transformer on in_scale * x at that timestep, eps = uncond + s (text - uncond) on the first C channels, then
 *   m0 = m_x x + m_eps eps;   x = c_x x + c0 m0 + c1 h1 + c2 h2 + c3 h3 + c_noise noise[row];   push: (h1, h2, h3) <- (m0, h1, h2)
 * noise: DEVICE [n_evals][samples * C * F * H * W] fp32 (only the rows with c_noise != 0 are read), or NULL when no row has one.
 * Preconditions as latte_t2v_guided_ddim_loop; LATTE_ERR_INVALID also for a non-finite entry, a non-integral or negative timestep,
 * c_noise != 0 without noise, and a c_j (j >= 1) that is non-zero before j rows with push have run.  Nothing is launched when a
 * check fails.  The table is the one of latte_sample_plan_loop (csrc/plan.h: PlanCol). */
#define LATTE_T2V_PLAN_COLS LATTE_PLAN_COLS
int latte_t2v_guided_linear_loop(latte_t2v_t* e, float* x, int samples, int n_evals, const double* plan, const float* noise,
                                 float guidance_scale, int enable_temporal_attentions, void* stream);
/* The two guided loops on x [samples, C, total_frames, H, W] with overlapping temporal windows (the scheme of
 * latte_sample_loop_windows, F = video_length; the noise rows of the linear loop have x's shape).  The installed text context must hold
 * 2 * samples * W rows ordered [negative prompts | prompts], each prompt's row repeated W times.  Behind the weights check:
 * LATTE_ERR_INVALID for total_frames < video_length, stride outside 1 ... video_length and H * W % 4 != 0; then LATTE_ERR_STATE for
 * 2 * samples * W > max_batch and a text context of another row count; then the checks of the plain loops.  Nothing is launched
 * when a check fails. */
int latte_t2v_guided_ddim_loop_windows(latte_t2v_t* e, float* x, int samples, int n_steps, const int64_t* timesteps, const double* alpha_t,
                                       const double* alpha_prev, float guidance_scale, int enable_temporal_attentions, int total_frames,
                                       int stride, void* stream);
int latte_t2v_guided_linear_loop_windows(latte_t2v_t* e, float* x, int samples, int n_evals, const double* plan, const float* noise,
                                         float guidance_scale, int enable_temporal_attentions, int total_frames, int stride, void* stream);

/* ------------------------------------------------------------------ T5 v1.1 text encoder
 * transformers.T5EncoderModel (feed_forward_proj "gated-gelu"): the text_encoder of Latte-1 text-to-video (T5-v1.1-XXL: d_model 4096,
 * d_kv 64, 64 heads, d_ff 10240, 24 layers).  Pre-norm blocks on an fp32 residual stream, RMSNorm statistics and softmax in fp32, no
 * bias anywhere, scores unscaled, + position_bias[h][key - query] from block 0's relative_attention_bias (bidirectional buckets) and a
 * key mask that removes padded keys exactly.  Projection operands (activations and weights) are split f16 pairs
 * (hi + 2^-11 lo, csrc/t5.hip), attention operands plain f16.  d_kv must be 64, d_model and d_ff multiples of 64, max_len <= 512,
 * compute_dtype LATTE_DTYPE_F16. */
typedef struct latte_t5 latte_t5_t;
typedef struct {
  int d_model, d_kv, num_heads, d_ff, num_layers, vocab_size;
  int relative_attention_num_buckets;   /* 32 */
  int relative_attention_max_distance;  /* 128 */
  float layer_norm_epsilon;             /* 1e-6 */
  int compute_dtype;
} latte_t5_config_t;
/* Allocates the packed weights and the workspace of max_batch x max_len tokens on the current device. */
int latte_t5_create(const latte_t5_config_t* cfg, int max_batch, int max_len, latte_t5_t** out);
void latte_t5_destroy(latte_t5_t* t);
int latte_t5_num_keys(const latte_t5_t* t);
const char* latte_t5_key(const latte_t5_t* t, int i);
/* load_state_dict for ONE tensor under its transformers key ("shared.weight", "encoder.block.3.layer.1.DenseReluDense.wi_0.weight",
 * ...): fp32 in DEVICE memory, shape[ndim] checked against the configuration; packed here, `data` is not kept.
 * "encoder.embed_tokens.weight" is the tied duplicate of "shared.weight": either fills the one table. */
int latte_t5_load_weight(latte_t5_t* t, const char* key, const float* data, const int64_t* shape, int ndim, void* stream);
int latte_t5_check_weights(latte_t5_t* t);
/* last_hidden_state: ids int64 [B, L], mask fp32 [B, L] (> 0.5 = attend; NULL = all), out fp32 [B, L, d_model]; all device memory.
 * An id outside [0, vocab_size) reads embedding row 0.  A row's result does not depend on B or on the other rows. */
int latte_t5_forward(latte_t5_t* t, const int64_t* ids, const float* mask, int B, int L, float* out, void* stream);

/* ------------------------------------------------------------------ measurement hooks (bench.py)
 * Runs ONE denoiser forward eagerly with HIP events around every kernel launch on `stream`,
 * synchronises, and reports per-kernel-class totals.  classes (fixed order):
 *   0 gemm_qkv 1 gemm_proj 2 gemm_fc1 3 gemm_fc2 4 attn_spatial 5 attn_temporal 6 ln_modulate
 *   7 embed_cond 8 patch_embed 9 final_layer 10 qkv_attn_spatial 11 qkv_attn_temporal (the fused QKV projection +
 *   attention kernel of csrc/qkv_attn.hip, which replaces classes 0 + 4 / 0 + 5 in the blocks whose shape allows it)
 * ms_out / launches_out: arrays of n (>= 12). */
#define LATTE_NUM_KERNEL_CLASSES 12
int latte_profile_forward(latte_engine_t* e, const float* x, const int64_t* t, const int64_t* y, int batch,
                          float* out, float* ms_out, int* launches_out, int n, void* stream);
/* The same with guided != 0: the denoiser call of latte_forward_with_cfg (x = the first half of the batch, used for both halves;
 * split operands per the "guided_split" option), WITHOUT the guidance combination -- so the table describes the kernels a guided
 * sampling step really runs (bench.py: config3.roofline_table). */
int latte_profile_forward_ex(latte_engine_t* e, const float* x, const int64_t* t, const int64_t* y, int batch, int guided,
                             float* out, float* ms_out, int* launches_out, int n, void* stream);
/* Stand-alone timing of the dominant kernel: C[M,N] = A[M,K] * W[N,K]^T (+bias epilogue `epi`,
 * 0 = bf16 out, 1 = bias+GELU, 2 = gated residual) on synthetic operands already resident in HBM;
 * `iters` back-to-back launches between two HIP events on `stream`.  variant selects the tile
 * configuration (0 = engine default for the shape). */
int latte_bench_gemm(int M, int N, int K, int epi, int dtype, int variant, int iters, float* ms_per_launch,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LATTE_AMD_H_ */
