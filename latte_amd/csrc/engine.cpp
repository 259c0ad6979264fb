// Engine host logic: weight ingestion, workspace, the denoiser forward and the fused sampling loop.
//
//   Latte.forward / forward_with_cfg      /root/reference/models/latte.py:314-398
//   p_sample_loop / ddim_sample_loop      /root/reference/diffusion/gaussian_diffusion.py:423-515,604-684
//   _WrappedModel (index -> timestep)     /root/reference/diffusion/respace.py:125-130
//
// Data layout in HBM (one canonical token order, no transposes between spatial and temporal blocks):
//   residual stream  xres  fp32 [B*F*T (padded to 256), D]   row = (b*F + f)*T + t
//   GEMM operands    xn    half [rows, D], qkv half [rows, 3D], h half [rows, mlp]
//   conditioning     mod   fp32 [B, depth*6D + 2D]  (all adaLN outputs of one forward, computed once per
//                    SAMPLE; the reference recomputes them on F or T repeated rows, latte.py:333-339)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "block.h"
#include "plan.h"
#include "weight_store.h"

namespace latte {

static thread_local std::string g_last_error;
static std::atomic<int> g_debug_choice[DBG_NUM_CHOICES];
int debug_choice(DebugChoice c) { return g_debug_choice[c].load(std::memory_order_relaxed); }
int set_debug_choice(const char* name, int value) {
  static const char* const names[DBG_NUM_CHOICES] = {"attn_variant", "xattn_flash", "tn_kernel", "tn_wn", "attn_bwd_tiles", "conv_kernel", "vae_split", "gated_rmw_shape", "stream_policy"};
  static const int allowed[DBG_NUM_CHOICES][4] = {{1, 5, 12, 13}, {1, 0, 0, 0}, {4, 0, 0, 0}, {4, 0, 0, 0}, {1, 2, 0, 0}, {1, 2, 3, 4}, {0, 0, 0, 0}, {1, 2, 0, 0}, {0, 0, 0, 0}};
  for (int i = 0; i < DBG_NUM_CHOICES; ++i) {
    if (name && std::string(name) == names[i]) {
      bool ok = value == 0;
      for (int k = 0; k < 4; ++k) ok = ok || (allowed[i][k] != 0 && value == allowed[i][k]);
      ok = ok || (i == DBG_VAE_SPLIT && (value >> 24) == 1);   // (1 << 24) | pass mask (vae_engine.cpp: vae_split_mask)
      ok = ok || (i == DBG_STREAM_POLICY && (value >> 4) == 1);   // 16 | StreamPolicy mask (debug.hip: debug_stream_policy)
      if (!ok) return -1;
      g_debug_choice[i].store(value, std::memory_order_relaxed);
      return 0;
    }
  }
  return -1;
}
void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

enum PackKind { PK_F32, PK_F32_TRANSPOSE, PK_H16 };   // WeightSlot::kind; PK_F32_TRANSPOSE: source [rows][cols]

}  // namespace latte

using namespace latte;

struct latte_engine {
  latte_model_config_t cfg;
  int max_batch = 0;
  int D = 0, T = 0, F = 0, G = 0, Cin = 0, Cout = 0, H = 0, P = 0, KPE = 0, Hm = 0, hd = 0;
  int nmod = 0;           // depth*6D + 2D
  int64_t rows_max = 0, rows_pad = 0;
  int gemm_variant = 0;  // 0 = per-shape choice (gemm_auto_variant)
  int gemm_variant_of[4] = {0, 0, 0, 0};   // per-GEMM override (qkv, proj, fc1, fc2); 0 = gemm_variant
  int fuse_qkv_attn = 3;                   // bit 0: spatial blocks, bit 1: temporal blocks run qkv projection + attention as ONE kernel
                                           // (qkv_attn.hip) wherever the shape allows it (T == 256 / F == 16); 0 = the un-fused pair;
                                           // bits 2, 3: QkvAttnArgs::flags (schedule variants, same results)
  int gated_split_k = 0;                   // gated GEMMs of small batches: 0 = rule of gated_gemm (block.cpp), 1 = never split, 2..4 = force
  int gated_rmw_shape = GATED_RMW_SHAPE_DEFAULT;   // GemmArgs::rmw_mode of the out-projection and fc2: 0 = fragment-wise, 1 = line-wise residual accesses
  int stream_policy = STREAM_POLICY_DEFAULT;       // StreamPolicy bits: which once-used streams of a block are issued `nt` (unguided forward)
  bool stream_policy_set = false;                  // set through the option: applies at every batch, not only where the streams overflow the cache
  int fc2_temp_embed = 1;                  // the first block's fc2 adds temp_embed in its epilogue where its kernel can (GemmArgs::te); 0 = the
                                           // second block's first LayerNorm pass adds it (an extra write of the residual stream); same bits
  // Guided calls (forward_with_cfg, latte.py:379-398): eps_u + s (eps_c - eps_u) amplifies the part of the operand rounding that differs
  // between the two halves (s = 7: 7 c - 6 u).  At trained-scale gates the f16 forward of XL/2 then sits AT north_star's 1e-3 (0.6 - 1.2e-3
  // over gate_std x timestep x seed, two of twelve draws above: profiles/r5_gate_parity_guided.json); the per-rounding-point attribution
  // on CPU (oracle/emulate_operands.py) names the operands of the out-projection (attention output) and of fc1 / fc2.  guided_split:
  // bit 0 = the attention output, bit 1 = the LayerNorm-modulate output in front of fc1 are carried as SPLIT pairs [hi | lo] (two halves
  // per value, ~22 mantissa bits) against weights stored [W | W] -- the same GEMM kernels on K' = 2 K, no rounding of that operand.
  // Round 6: bit 2 / bit 3 = the same two operands with the remainder in FP8 (e4m3 of lo 2^12, one byte per value) and the product
  // lo . W8^T collected by a block-scaled fp8 MFMA pass behind the f16 K loop of the same GEMM launch (GemmArgs::A8, gemm_pw.hip):
  // half the MFMA time and a quarter of the operand bytes of the [hi | lo] . [W | W] form; the remainder term is 2^-12 of the product,
  // so its own fp8 rounding (2^-4 relative) is 2^-16 -- below the weight operand's f16 rounding.  A bit-2/3 setting wins over bit 0/1
  // for its operand.  Guided calls of f16 engines only (bf16 cannot reach 1e-3 with or without it: default 0 there); where a shape
  // Round 6, second form: bit 4 = fc1's operand with the remainder in FP4 (e2m1 codes, one E8M0 scale per row: ln_modulate's SPLIT4 output,
  // GemmArgs::A4) -- the block-scaled MFMA runs fp4 x fp4 at twice the fp8 rate and a code row is half the bytes; wins over bits 1 / 3.
  // has no split form (un-fused attention, N % 192, K % 128) that operand stays plain -- latte_engine_get_info("guided_split_active")
  // reports what the last guided forward really ran.
  int guided_split = 20;
  int guided_split_active = 0;             // what the last guided forward used (bits as above)
  bool split_failed = false;               // an allocation for the split operands failed once: guided calls run plain from then on
  bool split_w_ready = false;              // the derived weight copies (proj_w2 / fc1_w2 / proj_w8 / fc1_w8) hold the current weights
  hipEvent_t load_event = nullptr;         // recorded behind every weight conversion on ITS stream: the derived copies wait for it
  half_t* xn2 = nullptr;                   // [rows_pad, 2 D]: split LayerNorm-modulate output (lazily allocated)
  unsigned char* lo8 = nullptr;            // [rows_pad, D] bytes: the fp8 remainder of the attention output, then of fc1's operand
  unsigned char *lo4 = nullptr, *lo4s = nullptr;   // [rows_pad, lo4_pitch(D)] e2m1 codes + [rows_pad] row scales: the fp4 remainder of fc1's operand (bit 4)
  float *split_ws = nullptr, *zero_bias = nullptr;   // partial products of the split gated GEMMs, a zero bias row for them
  std::vector<BlockLinears> blocks;
  float *ada_w = nullptr, *ada_b = nullptr, *pos = nullptr, *temp = nullptr, *pe_wt = nullptr, *pe_b = nullptr,
        *t0_w = nullptr, *t0_b = nullptr, *t2_w = nullptr, *t2_b = nullptr, *ytab = nullptr, *fin_wt = nullptr,
        *fin_b = nullptr;
  float *xres = nullptr, *mod = nullptr, *temb0 = nullptr, *cvec = nullptr, *model_out = nullptr, *noise_buf = nullptr;
  half_t *xn = nullptr, *qkv = nullptr, *hbuf = nullptr;
  int64_t* tmap_dev = nullptr;
  int64_t tmap_cap = 0;
  // extras == 78 (latte.py:238-242): text projection weights, the projected rows of the current text batch, identity
  // row index (the projected rows enter the conditioning exactly where the label-table rows do), t-only vector / rows
  // for the final layer, whose conditioning never includes the text (latte.py:372-373)
  float *txt_w = nullptr, *txt_b = nullptr, *txt_proj = nullptr, *cvec_t = nullptr, *cond_rows_t = nullptr;
  int64_t* iota = nullptr;
  int64_t cond_t_cap = 0;
  int txt_rows = 0;
  // conditioning of a whole chain (latte_sample_loop): timestep-embedding table (own or installed after the RCCL
  // broadcast), per-(step, sample) conditioning rows and all adaLN outputs
  float *temb_table = nullptr, *temb_own = nullptr, *temb_work = nullptr, *cond_rows = nullptr, *mod_all = nullptr;
  int temb_table_n = 0;        // > 0: an installed table of that many respaced steps
  std::vector<int64_t> temb_table_map;   // the timestep_map the installed table was computed for
  std::vector<int64_t> temb_own_map;     // the timestep_map temb_own currently holds (empty: none); a chain run in several
                                         // latte_sample_loop segments computes its table once
  int64_t temb_table_cap = 0, temb_own_cap = 0, temb_cap = 0, cond_cap = 0, mod_all_cap = 0;
  float *bpd_xt = nullptr, *bpd_ws = nullptr;   // latte_bpd_loop: x_t of the step, the reduction's per-block slots
  int64_t bpd_xt_cap = 0, bpd_ws_cap = 0;
  // latte_sample_plan_loop (taken from the arena by its first call): the ring of three remembered outputs and the scaled model input,
  // max_batch latents each; t_embedder of every row of the plan, in chain order
  float *plan_hist[3] = {nullptr, nullptr, nullptr}, *plan_xin = nullptr, *plan_temb = nullptr;
  int64_t plan_temb_cap = 0;
  // overlapping temporal windows (taken from the arena by the first windowed chain): the gathered clips (the size of noise_buf), the
  // merged model output (the size of model_out), the labels repeated per window
  float *win_clips = nullptr, *win_merged = nullptr;
  int64_t* win_y = nullptr;
  int train_timesteps = 1000;   // latte_sample_plan_loop refuses timesteps at or above it (diffusion_steps of create_diffusion)
  WeightSlots weights;
  DeviceArena arena;
  uint64_t seed = 0, rng_offset = 0;
};

namespace {

// Derived weights / operand buffers of the split operands of a guided call, for the bits of `need` only (guided_split), each pointer
// guarded on its own.  An allocation failure does not fail the forward: it is reported once on stderr, `split_failed` is set and this
// and every later guided call runs the plain f16 path.  The copies are built on the forward's stream BEHIND the last weight
// conversion (load_event), whatever stream that ran on.  Returns the bits that are usable.
int ensure_split_weights(latte_engine* e, int need, hipStream_t st) {
  const int D = e->D, Hm = e->Hm;
  if (e->split_failed) return 0;
  auto give_up = [&](const char* what) {
    fprintf(stderr, "latte_amd: guided_split: allocation of %s failed (%s); guided calls run with plain f16 operands\n", what, latte_last_error());
    e->split_failed = true;
    return 0;
  };
  bool fresh = false;
  if ((need & 2) && !e->xn2 && e->arena.alloc(&e->xn2, (size_t)e->rows_pad * 2 * D)) return give_up("the [rows, 2 D] operand buffer");
  if ((need & 12) && !e->lo8 && e->arena.alloc(&e->lo8, (size_t)e->rows_pad * D)) return give_up("the fp8 remainder buffer");
  if ((need & 16) && !e->lo4 && (e->arena.alloc(&e->lo4, (size_t)e->rows_pad * lo4_pitch(D)) || e->arena.alloc(&e->lo4s, (size_t)e->rows_pad)))
    return give_up("the fp4 remainder buffer");   // (zero-filled: the padding columns of a code row stay zero codes)
  for (auto& w : e->blocks) {
    if ((need & 1) && !w.proj_w2) { if (e->arena.alloc(&w.proj_w2, (size_t)D * 2 * D, false)) return give_up("[W | W] of the out-projection"); fresh = true; }
    if ((need & 2) && !w.fc1_w2) { if (e->arena.alloc(&w.fc1_w2, (size_t)Hm * 2 * D, false)) return give_up("[W | W] of fc1"); fresh = true; }
    if ((need & 4) && !w.proj_w8) { if (e->arena.alloc(&w.proj_w8, (size_t)D * D, false)) return give_up("W8 of the out-projection"); fresh = true; }
    if ((need & 8) && !w.fc1_w8) { if (e->arena.alloc(&w.fc1_w8, (size_t)Hm * D, false)) return give_up("W8 of fc1"); fresh = true; }
    if ((need & 16) && !w.fc1_w4) {
      if (e->arena.alloc(&w.fc1_w4, (size_t)Hm * lo4_pitch(D), false) || e->arena.alloc(&w.fc1_w4s, (size_t)Hm, false)) return give_up("W4 of fc1");
      fresh = true;
    }
  }
  if (e->split_w_ready && !fresh) return need;
  if (e->load_event && hipStreamWaitEvent(st, e->load_event, 0) != hipSuccess) return give_up("the wait for the weight conversion");
  const int dt = e->cfg.compute_dtype;
  for (auto& w : e->blocks) {
    for (int h = 0; h < 2; ++h) {
      if (w.proj_w2 && hipMemcpy2DAsync(w.proj_w2 + h * D, (size_t)2 * D * 2, w.proj_w, (size_t)D * 2, (size_t)D * 2, D, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return give_up("the [W | W] copy");
      if (w.fc1_w2 && hipMemcpy2DAsync(w.fc1_w2 + h * D, (size_t)2 * D * 2, w.fc1_w, (size_t)D * 2, (size_t)D * 2, Hm, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return give_up("the [W | W] copy");
    }
    if (w.proj_w8 && launch_pack_w8(w.proj_w, w.proj_w8, (int64_t)D * D, dt, st)) return give_up("the W8 pack");
    if (w.fc1_w8 && launch_pack_w8(w.fc1_w, w.fc1_w8, (int64_t)Hm * D, dt, st)) return give_up("the W8 pack");
    if (w.fc1_w4 && launch_pack_w4(w.fc1_w, w.fc1_w4, w.fc1_w4s, Hm, D, dt, st)) return give_up("the W4 pack");
  }
  e->split_w_ready = true;
  return need;
}

// mod_override != nullptr: the adaLN outputs of this step were precomputed ([B or 1 rows, nmod], row stride mod_stride;
// stride 0 = one row shared by every sample) and the conditioning launches are skipped.
int run_forward(latte_engine* e, const float* x, const int64_t* t, const int64_t* y, int B, bool cfg_dup, float* out,
                hipStream_t st, EventProfile* prof, const float* mod_override = nullptr, int mod_stride_override = 0) {
  const auto& c = e->cfg;
  if (B <= 0 || B > e->max_batch) return fail(LATTE_ERR_STATE, "forward: batch exceeds max_batch of the engine");
  if (c.extras == 2 && y == nullptr && !mod_override) return fail(LATTE_ERR_INVALID, "forward: class-conditional model needs y");
  if (c.extras == 78 && e->txt_rows != B && !mod_override)
    return fail(LATTE_ERR_STATE, "forward: text-conditioned model needs latte_engine_set_text_embedding with one row per sample first");
  if (cfg_dup && (B % 2)) return fail(LATTE_ERR_INVALID, "forward_with_cfg: batch must be even");
  const int D = e->D, T = e->T, F = e->F, dt = c.compute_dtype;
  const int M = B * F * T;
  const int rps = F * T;
  Timer tm{prof, st};
  int rc;
  tm.mark(C_NONE);
  // --- conditioning: t_emb = MLP(sincos(t)) (latte.py:119-123); c = t_emb (+ y_emb) (:337,:348); all adaLN at once
  const float* modp = e->mod;
  int mstride = e->nmod;
  if (mod_override) {
    modp = mod_override;
    mstride = mod_stride_override;
  } else {
    if ((rc = launch_small_linear(IN_TFREQ, nullptr, t, e->t0_w, e->t0_b, nullptr, nullptr, e->temb0, B, D, 256, D, st))) return rc;
    const float* add_tab = c.extras == 2 ? e->ytab : c.extras == 78 ? e->txt_proj : nullptr;
    const int64_t* add_idx = c.extras == 78 ? e->iota : y;
    if ((rc = launch_small_linear(IN_SILU, e->temb0, nullptr, e->t2_w, e->t2_b, add_tab, add_idx, e->cvec, B, D, D, D, st))) return rc;
    // adaLN_modulation = Linear(SiLU(c)): SiLU once per row here, not once per output feature inside the linear
    if ((rc = launch_silu_rows(e->cvec, e->cvec, (size_t)B * D, st))) return rc;
    if ((rc = launch_small_linear(IN_PLAIN, e->cvec, nullptr, e->ada_w, e->ada_b, nullptr, nullptr, e->mod, B, e->nmod, D,
                                  e->nmod, st))) return rc;
    if (c.extras == 78) {   // final layer: c = t only (latte.py:372-373) -> redo its 2D columns from the plain t_emb
      const size_t fo = (size_t)c.depth * 6 * D;
      if ((rc = launch_small_linear(IN_SILU, e->temb0, nullptr, e->t2_w, e->t2_b, nullptr, nullptr, e->cvec_t, B, D, D, D, st))) return rc;
      if ((rc = launch_silu_rows(e->cvec_t, e->cvec_t, (size_t)B * D, st))) return rc;
      if ((rc = launch_small_linear(IN_PLAIN, e->cvec_t, nullptr, e->ada_w + fo * D, e->ada_b + fo, nullptr, nullptr,
                                    e->mod + fo, B, 2 * D, D, e->nmod, st))) return rc;
    }
  }
  tm.mark(C_COND);
  // --- patch embed + pos_embed (latte.py:330-331)
  if (cfg_dup) {
    const int hb = B / 2;
    if ((rc = launch_patch_embed(x, e->pe_wt, e->pe_b, e->pos, e->xres, hb * F, e->Cin, e->H, c.patch_size, D, st))) return rc;
    if ((rc = launch_patch_embed(x, e->pe_wt, e->pe_b, e->pos, e->xres + (size_t)hb * rps * D, hb * F, e->Cin, e->H,
                                 c.patch_size, D, st))) return rc;
  } else {
    if ((rc = launch_patch_embed(x, e->pe_wt, e->pe_b, e->pos, e->xres, B * F, e->Cin, e->H, c.patch_size, D, st))) return rc;
  }
  tm.mark(C_PATCH);
  // split-operand linears of a guided call (latte_engine::guided_split); the K' = 2 K operands must stay inside the 32-bit buffer offsets
  int gsplit = cfg_dup ? e->guided_split : 0;
  if (dt != LATTE_DTYPE_F16) gsplit &= 3;                                          // the fp8 / fp4 remainders exist beside f16 only
  if ((gsplit & 16) && !gemm_lo4_ok(M, e->Hm, D)) gsplit = (gsplit & ~16) | 8;     // no fp4 form for the shape: the fp8 one
  if (gsplit & 16) gsplit &= ~10;                                                  // one form per operand: fp4 wins for fc1's
  if (gsplit & 4) gsplit &= ~1;                                                    // fp8 wins over the f16 pair
  if (gsplit & 8) gsplit &= ~2;
  if ((gsplit & 4) && !gemm_lo8_ok(M, D, D)) gsplit = (gsplit & ~4) | 1;          // no fp8 form for the shape (N % 192, K % 128): the f16 pair
  if ((gsplit & 8) && !gemm_lo8_ok(M, e->Hm, D)) gsplit = (gsplit & ~8) | 2;
  if ((gsplit & 3) && (uint64_t)e->rows_pad * 2 * D * 2 >= (1ull << 32)) gsplit &= ~3;
  if (gsplit) gsplit = ensure_split_weights(e, gsplit, st);
  // Stream hints: the split-operand kernels of a guided call have no hinted forms; and the library's own default applies only where
  // the hidden activations cannot stay in the 256 MiB Infinity Cache beside the residual anyway (B = 8 at XL/2: 302 + 151 MB) -- a
  // hidden stream that fits (B <= 4) is served from the cache when fc2 reads it back, and a hint would take that away.
  const bool streams_overflow = (int64_t)M * (2 * e->Hm + 4 * D) > (256ll << 20);
  const int stream_policy = gsplit ? 0 : (e->stream_policy_set || streams_overflow) ? e->stream_policy : 0;
  BlockCtx bc{};
  bc.B = B; bc.F = F; bc.T = T; bc.D = D; bc.heads = c.num_heads; bc.hd = e->hd; bc.Hm = e->Hm; bc.dt = dt;
  bc.xres = e->xres; bc.xn = e->xn; bc.qkv = e->qkv; bc.hbuf = e->hbuf;
  bc.mod_stride = mstride;
  bc.fuse_qkv_attn = e->fuse_qkv_attn;
  for (int k = 0; k < 4; ++k) bc.gemm_variant_of[k] = e->gemm_variant_of[k] ? e->gemm_variant_of[k] : e->gemm_variant;
  bc.gated_split_k = e->gated_split_k; bc.rmw_mode = e->gated_rmw_shape; bc.stream_policy = stream_policy;
  bc.split_ws = e->split_ws; bc.zero_bias = e->zero_bias;
  bc.gsplit = gsplit; bc.xn2 = e->xn2; bc.lo8 = e->lo8; bc.lo4 = e->lo4; bc.lo4s = e->lo4s;
  bc.guided_split_active = gsplit & 26;   // bits 1 / 3 / 4 always apply; bits 0 / 2 once an attention kernel has produced the pair
  bc.prof = prof;
  // x + temp_embed once, after the first spatial block (latte.py:357-358): in that block's fc2 epilogue where fc2 runs on the
  // rolling 12-wave kernel, else in the second block's first LayerNorm pass
  bc.temp = e->temp;
  bc.te_in_fc2 = e->fc2_temp_embed && c.depth > 1 && block_fc2_takes_te(bc);
  for (int i = 0; i < c.depth; ++i) {
    const float* mb = modp + (size_t)i * 6 * D;  // chunk(6): shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
    if ((rc = block_attention(bc, e->blocks[i], i, mb, st)) || (rc = block_mlp(bc, e->blocks[i], i, mb, st))) return rc;
  }
  // --- final layer (latte.py:197-201) + unpatchify (:297-310)
  const float* fm = modp + (size_t)c.depth * 6 * D;  // chunk(2): shift, scale
  if ((rc = launch_final_layer(e->xres, fm, fm + D, mstride, e->fin_wt, e->fin_b, out, M, D, rps, T, c.patch_size,
                               e->Cout, e->H, st))) return rc;
  tm.mark(C_FINAL);
  if (cfg_dup) e->guided_split_active = bc.guided_split_active;
  return LATTE_OK;
}

// fp32 emulation of the reference's per-step tensor arithmetic (gaussian_diffusion.py:869-881: fp64 table ->
// .float()); compiled with -ffp-contract=off.
int grow(latte_engine* e, float** p, int64_t* cap, int64_t need) {
  if (*cap >= need) return LATTE_OK;
  if (*p) {   // release the smaller block (setup path: the implicit device synchronisation of hipFree is fine here)
    e->arena.release(*p);
    *p = nullptr;
    *cap = 0;
  }
  int rc = e->arena.alloc(p, (size_t)need, false);
  if (!rc) *cap = need;
  return rc;
}

// Timestep-embedding table of a schedule: row i = t_embedder(timestep_map[i]) (latte.py:84-123, respace.py:125-130).
// This is the [steps, D] fp32 table rank 0 broadcasts over RCCL in the multi-GPU driver (1.15 MB for 250 x 1152).
// `ts`: n HOST timesteps (row i = t_embedder(ts[i]); repeats allowed).
int compute_temb_rows(latte_engine* e, const int64_t* ts, int n, float* out, hipStream_t st) {
  const int D = e->D;
  int rc;
  if (e->tmap_cap < n) {
    if ((rc = e->arena.alloc(&e->tmap_dev, (size_t)n, false))) return rc;
    e->tmap_cap = n;
  }
  LATTE_HIP(hipMemcpyAsync(e->tmap_dev, ts, sizeof(int64_t) * n, hipMemcpyHostToDevice, st));
  LATTE_HIP(hipStreamSynchronize(st));   // the host vector may be freed by the caller
  if ((rc = grow(e, &e->temb_work, &e->temb_cap, (int64_t)n * D))) return rc;
  constexpr int CH = 64;   // rows per launch: the kernel keeps a weight row in registers and loops over the rows
  for (int r0 = 0; r0 < n; r0 += CH) {
    const int rows = std::min(CH, n - r0);
    if ((rc = launch_small_linear(IN_TFREQ, nullptr, e->tmap_dev + r0, e->t0_w, e->t0_b, nullptr, nullptr,
                                  e->temb_work + (size_t)r0 * D, rows, D, 256, D, st))) return rc;
    if ((rc = launch_small_linear(IN_SILU, e->temb_work + (size_t)r0 * D, nullptr, e->t2_w, e->t2_b, nullptr, nullptr,
                                  out + (size_t)r0 * D, rows, D, D, D, st))) return rc;
  }
  return LATTE_OK;
}
int compute_temb_table(latte_engine* e, const latte_schedule_t* s, float* out, hipStream_t st) {
  return compute_temb_rows(e, s->timestep_map.data(), s->num_timesteps, out, st);
}

// ---- conditioning of a whole chain (latte_sample_loop_ex, latte_bpd_loop): it depends on (timestep, label) only, never on x.
struct ChainCond {
  const float* temb;   // [num_timesteps, D] timestep-embedding table, own or installed
  int bu;              // conditioning rows per step: 1 for an unconditional model, else the batch
  int chunk_steps;     // steps whose rows fit mod_all at once
  int lo = 0, hi = -1; // table rows whose conditioning mod_all holds right now (chain_mod)
};

// chunk size and row buffers of a chain of n_run steps with cc->bu rows each
int chain_row_buffers(latte_engine* e, int n_run, ChainCond* cc) {
  const int D = e->D, bu = cc->bu;
  int rc;
  cc->chunk_steps = std::max(1, 256 / bu);
  const int64_t rows_chunk = (int64_t)std::min(cc->chunk_steps, n_run) * bu;
  if ((rc = grow(e, &e->cond_rows, &e->cond_cap, rows_chunk * D))) return rc;
  if ((rc = grow(e, &e->mod_all, &e->mod_all_cap, rows_chunk * e->nmod))) return rc;
  if (e->cfg.extras == 78 && (rc = grow(e, &e->cond_rows_t, &e->cond_t_cap, rows_chunk * D))) return rc;
  return LATTE_OK;
}

// Picks the timestep-embedding table (computing the engine's own when none is installed for this timestep_map) and sizes the row
// buffers.  The conditioning rows of the chain are produced in chunks of <= 256 rows (= 256 / bu steps), right before the steps
// that use them: the adaLN outputs are 783 KB per row at XL/2 (nmod = 195 840 fp32), so the whole chain at once would
// be 3.1 GB for 250 guided steps at B = 16.  The adaLN weights are streamed once per 64 rows either way.
int chain_prepare(latte_engine* e, const latte_schedule_t* s, int bu, int n_run, hipStream_t st, ChainCond* cc) {
  const int n = s->num_timesteps, D = e->D;
  int rc;
  cc->bu = bu;
  if (e->temb_table_n == n && e->temb_table_map == s->timestep_map) {   // installed for exactly this timestep_map
    cc->temb = e->temb_table;
  } else {
    if (e->temb_own_map != s->timestep_map) {
      e->temb_own_map.clear();
      if ((rc = grow(e, &e->temb_own, &e->temb_own_cap, (int64_t)n * D))) return rc;
      if ((rc = compute_temb_table(e, s, e->temb_own, st))) return rc;
      e->temb_own_map = s->timestep_map;
    }
    cc->temb = e->temb_own;
  }
  return chain_row_buffers(e, n_run, cc);
}

// conditioning of respaced steps [lo, lo + cnt) into mod_all: rows ordered by index ascending, row (i - lo) * bu + b
int chain_conditioning(latte_engine* e, const ChainCond& cc, const int64_t* y, int lo, int cnt, hipStream_t st) {
  const int D = e->D, ex = e->cfg.extras, bu = cc.bu;
  const float* temb = cc.temb;
  const size_t fo = (size_t)e->cfg.depth * 6 * D;
  const int64_t rows_all = (int64_t)cnt * bu;
  int r2;
  if ((r2 = launch_cond_rows(temb + (size_t)lo * D, ex == 2 ? e->ytab : ex == 78 ? e->txt_proj : nullptr,
                             ex == 78 ? e->iota : y, e->cond_rows, cnt, bu, D, st))) return r2;
  if (ex == 78 &&   // t-only rows for the final layer (latte.py:372-373)
      (r2 = launch_cond_rows(temb + (size_t)lo * D, nullptr, nullptr, e->cond_rows_t, cnt, bu, D, st))) return r2;
  for (int64_t r0 = 0; r0 < rows_all; r0 += 64) {
    const int rows = (int)std::min<int64_t>(64, rows_all - r0);
    if ((r2 = launch_small_linear(IN_PLAIN, e->cond_rows + (size_t)r0 * D, nullptr, e->ada_w, e->ada_b, nullptr, nullptr,
                                  e->mod_all + (size_t)r0 * e->nmod, rows, e->nmod, D, e->nmod, st))) return r2;
    if (ex == 78 &&
        (r2 = launch_small_linear(IN_PLAIN, e->cond_rows_t + (size_t)r0 * D, nullptr, e->ada_w + fo * D, e->ada_b + fo, nullptr,
                                  nullptr, e->mod_all + (size_t)r0 * e->nmod + fo, rows, 2 * D, D, e->nmod, st))) return r2;
  }
  return LATTE_OK;
}

// The cursor over mod_all: the adaLN rows of table row i of a chain that walks towards row `last` (ascending when last >= i, else
// descending).  When row i is not resident the chunk is refilled from i in the direction of travel, capped at chunk_steps rows and at
// `last`.  This is the only place that indexes mod_all for a step.
int chain_mod(latte_engine* e, ChainCond* cc, const int64_t* y, int i, int last, hipStream_t st, const float** mod, int* stride) {
  if (i < cc->lo || i > cc->hi) {
    const int far = last >= i ? std::min(last, i + cc->chunk_steps - 1) : std::max(last, i - cc->chunk_steps + 1);
    cc->lo = std::min(i, far);
    cc->hi = std::max(i, far);
    int rc = chain_conditioning(e, *cc, y, cc->lo, cc->hi - cc->lo + 1, st);
    if (rc) return rc;
  }
  *mod = e->mod_all + (size_t)(i - cc->lo) * cc->bu * e->nmod;
  *stride = cc->bu == 1 ? 0 : e->nmod;
  return LATTE_OK;
}

// ---- what every fused loop shares besides its conditioning
// rows [lo, hi] of a schedule of n timesteps; `why2` is the entry point's own text for n < 2
int range_check(const std::string& who, int n, int lo, int hi, const char* why2) {
  if (hi >= n || lo < 0 || hi < lo) return fail(LATTE_ERR_INVALID, who + ": bad index range");
  if (n < 2) return fail(LATTE_ERR_INVALID, who + ": " + why2);
  return LATTE_OK;
}

// The argument block, in this order: batch, learn_sigma (skipped without a schedule), doubled batch, y, text.
// rows_per_sample: the denoiser rows of one sample, > 1 for a windowed chain (the text rows are installed per clip)
int chain_check(const std::string& who, const latte_engine* e, const latte_schedule_t* s, int batch, bool guided, const int64_t* y,
                bool text_allowed, int rows_per_sample = 1) {
  if (batch <= 0 || batch > e->max_batch) return fail(LATTE_ERR_STATE, who + ": batch exceeds max_batch");
  if (s && (s->var_type == 0) != (e->Cout == 2 * e->Cin))
    return fail(LATTE_ERR_INVALID, who + ": the model's learn_sigma and the diffusion's learn_sigma disagree "
                                         "(model output channels vs ModelVarType, gd:290 / :338)");
  if (guided && (batch % 2)) return fail(LATTE_ERR_INVALID, who + ": guidance needs the doubled batch");
  const int ex = e->cfg.extras;
  if (ex == 2 && y == nullptr) return fail(LATTE_ERR_INVALID, who + ": class-conditional model needs y");
  if (ex == 78 && !text_allowed) return fail(LATTE_ERR_INVALID, who + ": serves the class-conditional and unconditional models only");
  if (ex == 78 && e->txt_rows != batch * rows_per_sample)
    return fail(LATTE_ERR_STATE, who + ": text-conditioned model needs latte_engine_set_text_embedding with one row per sample first");
  return LATTE_OK;
}

// noise of step k: the caller's row k, else one draw from the engine's Philox stream (option "seed"), which advances
int chain_noise(latte_engine* e, const float* noise, int k, size_t numel, hipStream_t st, const float** nz) {
  if (noise) {
    *nz = noise + (size_t)k * numel;
    return LATTE_OK;
  }
  int rc = launch_fill_normal(e->noise_buf, numel, e->seed, e->rng_offset, st);
  if (rc) return rc;
  e->rng_offset += numel;
  *nz = e->noise_buf;
  return LATTE_OK;
}

// x after step k into slot k of a trail (NULL: no trail)
int chain_trail(float* trail, int k, const float* x, size_t numel, hipStream_t st) {
  if (trail) LATTE_HIP(hipMemcpyAsync(trail + (size_t)k * numel, x, sizeof(float) * numel, hipMemcpyDeviceToDevice, st));
  return LATTE_OK;
}

// ---- overlapping temporal windows: a chain over x of ws.L >= F frames evaluates the denoiser on the W
// windows of every batch row at once and averages their outputs where they overlap; the update kernels then run with frames = L.
// The checks of a windowed chain, after the shared ones: the window set and H * W % 4 (LATTE_ERR_INVALID), then the clips against
// max_batch (LATTE_ERR_STATE).
int chain_window_check(const std::string& who, const latte_engine* e, const WindowSet& ws, int batch) {
  int rc = window_check(who, ws, e->H * e->H);
  if (rc) return rc;
  if ((int64_t)batch * ws.count() > e->max_batch) return fail(LATTE_ERR_STATE, who + ": the clips (batch * windows) exceed max_batch");
  return LATTE_OK;
}

// First use: the clip and merged-output buffers (batch * L <= batch * W * F, so the sizes of noise_buf and model_out hold them); then
// the labels of the clips, y repeated per window.  *y_clips: what the conditioning and the forward of the chain index.
int chain_window_prepare(latte_engine* e, const WindowSet& ws, const int64_t* y, int batch, hipStream_t st, const int64_t** y_clips) {
  int rc;
  const size_t frame = (size_t)e->max_batch * e->F * e->H * e->H;
  if (!e->win_clips && (rc = e->arena.alloc(&e->win_clips, frame * e->Cin, false))) return rc;
  if (!e->win_merged && (rc = e->arena.alloc(&e->win_merged, frame * e->Cout, false))) return rc;
  if (!e->win_y && (rc = e->arena.alloc(&e->win_y, (size_t)e->max_batch, false))) return rc;
  *y_clips = y;
  if (!y) return LATTE_OK;
  const int W = ws.count();
  for (int w = 0; w < W; ++w)   // win_y[g W + w] = y[g]
    LATTE_HIP(hipMemcpy2DAsync(e->win_y + w, sizeof(int64_t) * W, y, sizeof(int64_t), sizeof(int64_t), batch, hipMemcpyDeviceToDevice, st));
  *y_clips = e->win_y;
  return LATTE_OK;
}

// One denoiser evaluation of a chain on x_in, *out = where its output lies ([batch, frames, Cout, HW]): the forward itself, or with
// windows gather -> the forward on the batch * W clips -> merge.
int chain_forward(latte_engine* e, const WindowSet* ws, const float* x_in, const int64_t* y, int batch, bool use_cfg, const float* mod,
                  int mstride, hipStream_t st, const float** out) {
  int rc;
  const int HW = e->H * e->H;
  if (ws) {
    if ((rc = launch_window_gather(x_in, e->win_clips, batch, *ws, e->Cin, HW, 0, st))) return rc;
    x_in = e->win_clips;
    batch *= ws->count();
  }
  if ((rc = run_forward(e, x_in, nullptr, y, batch, use_cfg, e->model_out, st, nullptr, mod, mstride))) return rc;
  *out = e->model_out;
  if (!ws) return LATTE_OK;
  *out = e->win_merged;
  return launch_window_merge(e->model_out, e->win_merged, batch / ws->count(), *ws, e->Cout, HW, 0, st);
}

SamplerCoefs make_coefs(const latte_schedule_t* s, int method, int i, float eta, int clip) {
  SamplerCoefs c{};
  c.method = method;
  c.clip = clip;
  c.min_log = (float)s->posterior_log_variance_clipped[i];
  c.max_log = (float)s->log_betas[i];
  c.sqrt_recip = (float)s->sqrt_recip_alphas_cumprod[i];
  c.sqrt_recipm1 = (float)s->sqrt_recipm1_alphas_cumprod[i];
  c.coef1 = (float)s->posterior_mean_coef1[i];
  c.coef2 = (float)s->posterior_mean_coef2[i];
  const float ab = (float)s->alphas_cumprod[i], abp = (float)s->alphas_cumprod_prev[i];
  // gd:549-553  sigma = eta * sqrt((1-abp)/(1-ab)) * sqrt(1 - ab/abp)
  const float sigma = (eta * std::sqrt((1.0f - abp) / (1.0f - ab))) * std::sqrt(1.0f - ab / abp);
  c.sigma = sigma;
  c.sqrt_ab_prev = std::sqrt(abp);
  c.dir_coef = std::sqrt((1.0f - abp) - sigma * sigma);  // gd:558: sqrt(1 - abp - sigma**2)
  if (method == LATTE_METHOD_DDIM_REVERSE) {   // gd:597-600 on the extracted fp32 alpha_bar_next; the update is the DDIM one
    const float abn = (float)s->alphas_cumprod_next[i];
    c.sigma = 0.0f;
    c.sqrt_ab_prev = std::sqrt(abn);
    c.dir_coef = std::sqrt(1.0f - abn);
  }
  c.nonzero = i == 0 ? 0.0f : 1.0f;
  c.cfg_scale = 1.0f;
  c.sqrt_one_minus_ab = std::sqrt(1.0f - ab);   // gd:368 on the fp32 alpha_bar
  c.mean_type = s->mean_type;
  c.var_type = s->var_type;
  // gd:298-313: FIXED_LARGE = log(append(posterior_variance[1], betas[1:])), FIXED_SMALL = posterior_log_variance_clipped
  if (s->var_type == 1) c.fixed_log_var = (float)std::log(i == 0 ? s->posterior_variance[1] : s->betas[i]);
  else c.fixed_log_var = (float)s->posterior_log_variance_clipped[i];
  return c;
}

// DDPM draws at every index but 0, DDIM where sigma != 0 (eta > 0), the reverse (inversion) step never
bool step_needs_noise(int method, const SamplerCoefs& c, int index) {
  return method == LATTE_METHOD_DDPM ? index != 0 : (c.sigma != 0.0f && index != 0);
}

// ---- known-region sampling: the noise slabs of a chain, in the order they are consumed.
// Repetition u (1 ... resample) of index i takes, in this order: the step's own noise, the noise of the blend that follows it, and
// the noise of the forward jump back to level i.  The chain loop and latte_known_chain_slabs both walk this.
struct KnownSlabs {
  bool step, blend, jump;
  int count() const { return (int)step + (int)blend + (int)jump; }
};
KnownSlabs known_slabs(int method, const SamplerCoefs& c, int i, int u, int resample) {
  return {step_needs_noise(method, c, i), i > 0, u < resample && i > 0};
}
// the fp32 (sqrt(abar), sqrt(1 - abar)) of a level, as make_coefs narrows its tables
void level_coefs(double abar, float* a, float* b) {
  const float ab = (float)abar;
  *a = std::sqrt(ab);
  *b = std::sqrt(1.0f - ab);
}

int known_method_check(const std::string& who, int method, int resample) {
  if (method != LATTE_METHOD_DDPM && method != LATTE_METHOD_DDIM) return fail(LATTE_ERR_INVALID, who + ": method must be DDPM or DDIM");
  if (resample < 1) return fail(LATTE_ERR_INVALID, who + ": resample must be >= 1");
  return LATTE_OK;
}

// The known part of a chain (latte_sample_loop_known): after every step the known part of x is replaced by `known` at the level x is at
struct KnownRegion {
  const float *known, *mask;
  int resample;      // repetitions of every index, the one-level forward jump between them
  int blend_start;   // blend at the level of start_index before the first step
};

// The caller's noise rows, two public contracts: a plain chain reads row k at step k (a DDPM step at index 0 has a row and skips it), a
// known chain reads the next unconsumed slab.  Engine-drawn noise (noise == NULL) never asks.
struct NoiseCursor {
  bool by_step;
  int next = 0;
  int row(int k) { return by_step ? k : next++; }
};

// latte_sample_loop_ex (dir = -1: start_index down to end_index), latte_invert_loop (dir = +1: start_index up to end_index) and
// latte_sample_loop_known (dir = -1 with `kn`: every index `resample` times, the known part of x replaced after every step);
// latte_sample_loop_windows (`ws`: x, the noise rows and the trails have ws->L frames)
int sampler_chain(const std::string& who, latte_engine* e, const latte_schedule_t* s, int method, int dir, float eta, int clip_denoised,
                  int guided, float cfg_scale, float* x, const int64_t* y, int batch, int start_index, int end_index, const KnownRegion* kn,
                  const float* noise, float* trail_sample, float* trail_x0, hipStream_t st, const WindowSet* ws = nullptr) {
  if (!e || !s || !x) return fail(LATTE_ERR_INVALID, who + ": null argument");
  int rc = latte_engine_check_weights(e);
  if (rc) return rc;
  if ((rc = range_check(who, s->num_timesteps, dir > 0 ? start_index : end_index, dir > 0 ? end_index : start_index,
                        "learned-range variance needs >= 2 timesteps"))) return rc;
  const bool use_cfg = guided != 0;   // forward_with_cfg semantics for ANY scale (latte.py:379-398 has no threshold)
  if ((rc = chain_check(who, e, s, batch, use_cfg, y, true, ws && ws->valid() ? ws->count() : 1))) return rc;
  const int HW = e->H * e->H;
  if (ws && (rc = chain_window_check(who, e, *ws, batch))) return rc;
  if (kn) {
    if ((rc = known_method_check(who, method, kn->resample))) return rc;
    if (!kn->known || !kn->mask) return fail(LATTE_ERR_INVALID, who + ": known and mask are required");
    if (HW % 4) return fail(LATTE_ERR_INVALID, who + ": H * W must be a multiple of 4 (16-byte accesses of the blend kernel)");
    if (dir > 0) return fail(LATTE_ERR_INVALID, who + ": a known region needs a descending chain");
  }
  // ---- conditioning of the whole chain: it depends on (timestep, label) only, never on x.
  //   temb[i]      = t_embedder(timestep_map[i])           (own, or the table installed after the RCCL broadcast)
  //   c[i, b]      = SiLU(temb[i] (+ y_embedder(y[b])))     latte.py:337,348 (+ the SiLU of :173)
  //   mod[i, b, :] = all 28 adaLN_modulation + the final layer's, = Linear(SiLU(c))   latte.py:172-178,192-198
  // Unconditional models have one row per step shared by every sample (row stride 0).  The adaLN weights (0.9 GB
  // fp32) are then streamed once per 64 rows instead of once per denoising step.
  const int n_run = (end_index - start_index) * dir + 1;
  const int frames = ws ? ws->L : e->F, rows = ws ? batch * ws->count() : batch;   // with windows the conditioning rows are per clip
  if (ws && (rc = chain_window_prepare(e, *ws, y, batch, st, &y))) return rc;
  ChainCond cc;
  if ((rc = chain_prepare(e, s, e->cfg.extras == 1 ? 1 : rows, n_run, st, &cc))) return rc;
  const size_t numel = (size_t)batch * frames * e->Cin * HW;
  const int reps = kn ? kn->resample : 1;
  NoiseCursor cur{kn == nullptr};
  // one blend at the level abar; its noise is the caller's next slab, or drawn in the kernel from the engine's stream
  // (level 0 takes none: alphas_cumprod_prev[0] = 1 gives (1, 0))
  auto blend = [&](double abar, bool takes_slab) -> int {
    float a = 1.0f, b = 0.0f;
    const float* nz = nullptr;
    const uint64_t off = e->rng_offset;
    if (takes_slab) {
      level_coefs(abar, &a, &b);
      if (noise) nz = noise + (size_t)cur.row(0) * numel;
      else e->rng_offset += numel;
    }
    return launch_known_blend(x, kn->known, kn->mask, nz, e->seed, off, a, b, batch, e->F, e->Cin, HW, 0, st);
  };
  if (kn && kn->blend_start && (rc = blend(s->alphas_cumprod[start_index], true))) return rc;
  for (int k = 0; k < n_run; ++k) {
    const int i = start_index + dir * k;
    const float* mod_i;
    int mstride;
    if ((rc = chain_mod(e, &cc, y, i, end_index, st, &mod_i, &mstride))) return rc;
    SamplerCoefs c = make_coefs(s, method, i, eta, clip_denoised);
    c.cfg_scale = cfg_scale;
    float* x0 = trail_x0 ? trail_x0 + (size_t)k * numel : nullptr;
    for (int u = 1; u <= reps; ++u) {
      const KnownSlabs need = known_slabs(method, c, i, u, reps);   // a plain chain takes the step's noise only
      const float* mo;
      if ((rc = chain_forward(e, ws, x, y, batch, use_cfg, mod_i, mstride, st, &mo))) return rc;
      const float* nz = nullptr;
      if (need.step && (rc = chain_noise(e, noise, cur.row(k), numel, st, &nz))) return rc;
      if ((rc = launch_sampler_update(c, x, mo, nz, batch, frames, e->Cin, HW, use_cfg ? 1 : 0, x, x0, st))) return rc;
      if (!kn) continue;
      if ((rc = blend(s->alphas_cumprod_prev[i], need.blend))) return rc;   // (1, 0) at i == 0: the known latents themselves
      if (need.jump) {   // back to level i: x <- sqrt(1 - beta_i) x + sqrt(beta_i) z, in place
        if ((rc = chain_noise(e, noise, cur.row(k), numel, st, &nz))) return rc;
        const float beta = (float)s->betas[i];
        if ((rc = launch_q_sample_scalar(std::sqrt(1.0f - beta), std::sqrt(beta), x, nz, numel, x, st))) return rc;
      }
    }
    if ((rc = chain_trail(trail_sample, k, x, numel, st))) return rc;
  }
  return LATTE_OK;
}

}  // namespace

extern "C" {

const char* latte_last_error(void) { return latte::g_last_error.c_str(); }
const char* latte_version(void) { return "latte_amd 0.1 (gfx950, HIP MFMA engine)"; }

int latte_engine_create(const latte_model_config_t* cfg, int max_batch, latte_engine_t** out) {
  if (!cfg || !out || max_batch <= 0) return fail(LATTE_ERR_INVALID, "engine_create: bad arguments");
  const auto& c = *cfg;
  if (c.hidden_size % 128 != 0) return fail(LATTE_ERR_INVALID, "engine_create: hidden_size must be a multiple of 128");
  if (c.depth <= 0 || c.depth % 2) return fail(LATTE_ERR_INVALID, "engine_create: depth must be even (spatial/temporal pairs)");
  if (c.num_heads <= 0 || c.hidden_size % c.num_heads) return fail(LATTE_ERR_INVALID, "dim should be divisible by num_heads");
  const int hd = c.hidden_size / c.num_heads;
  if (hd != 64 && hd != 72) return fail(LATTE_ERR_INVALID, "engine_create: head_dim must be 64 or 72");
  if (c.patch_size <= 0 || c.input_size % c.patch_size) return fail(LATTE_ERR_INVALID, "engine_create: input_size % patch_size != 0");
  if (c.mlp_hidden % 128 != 0) return fail(LATTE_ERR_INVALID, "engine_create: mlp_hidden must be a multiple of 128");
  if (c.extras != 1 && c.extras != 2 && c.extras != 78)
    return fail(LATTE_ERR_INVALID, "engine_create: extras must be 1 (uncond), 2 (class-cond) or 78 (text embedding)");
  if (c.in_channels != 4) return fail(LATTE_ERR_INVALID, "engine_create: in_channels must be 4 (guidance is hard-wired to 4 channels, latte.py:394)");
  if (c.compute_dtype != LATTE_DTYPE_BF16 && c.compute_dtype != LATTE_DTYPE_F16) return fail(LATTE_ERR_INVALID, "engine_create: bad compute dtype");

  auto* e = new latte_engine();
  e->cfg = c;
  if (c.compute_dtype != LATTE_DTYPE_F16) e->guided_split = 0;   // bf16 operands are a 3e-3 type at trained-scale gates, pair or not
  e->max_batch = max_batch;
  e->D = c.hidden_size;
  e->G = c.input_size / c.patch_size;
  e->T = e->G * e->G;
  e->F = c.num_frames;
  e->Cin = c.in_channels;
  e->Cout = c.learn_sigma ? 2 * c.in_channels : c.in_channels;
  e->H = c.input_size;
  e->P = c.patch_size * c.patch_size * e->Cout;
  e->KPE = c.in_channels * c.patch_size * c.patch_size;
  e->Hm = c.mlp_hidden;
  e->hd = hd;
  e->nmod = c.depth * 6 * e->D + 2 * e->D;
  e->rows_max = (int64_t)max_batch * e->F * e->T;
  e->rows_pad = (e->rows_max + 255) / 256 * 256;
  const int D = e->D;
  int rc = LATTE_OK;
#define TRY(x) do { if ((rc = (x))) { latte_engine_destroy(e); return rc; } } while (0)
  TRY(e->arena.alloc(&e->ada_w, (size_t)e->nmod * D));
  TRY(e->arena.alloc(&e->ada_b, (size_t)e->nmod));
  TRY(e->arena.alloc(&e->pos, (size_t)e->T * D));
  TRY(e->arena.alloc(&e->temp, (size_t)e->F * D));
  TRY(e->arena.alloc(&e->pe_wt, (size_t)e->KPE * D));
  TRY(e->arena.alloc(&e->pe_b, (size_t)D));
  TRY(e->arena.alloc(&e->t0_w, (size_t)D * 256));
  TRY(e->arena.alloc(&e->t0_b, (size_t)D));
  TRY(e->arena.alloc(&e->t2_w, (size_t)D * D));
  TRY(e->arena.alloc(&e->t2_b, (size_t)D));
  TRY(e->arena.alloc(&e->fin_wt, (size_t)D * e->P));
  TRY(e->arena.alloc(&e->fin_b, (size_t)e->P));
  e->weights.add("pos_embed", (int64_t)e->T * D, PK_F32, e->pos);
  e->weights.add("temp_embed", (int64_t)e->F * D, PK_F32, e->temp);
  e->weights.add("x_embedder.proj.weight", (int64_t)D * e->KPE, PK_F32_TRANSPOSE, e->pe_wt, D, e->KPE);
  e->weights.add("x_embedder.proj.bias", D, PK_F32, e->pe_b);
  e->weights.add("t_embedder.mlp.0.weight", (int64_t)D * 256, PK_F32, e->t0_w);
  e->weights.add("t_embedder.mlp.0.bias", D, PK_F32, e->t0_b);
  e->weights.add("t_embedder.mlp.2.weight", (int64_t)D * D, PK_F32, e->t2_w);
  e->weights.add("t_embedder.mlp.2.bias", D, PK_F32, e->t2_b);
  if (c.extras == 2) {
    TRY(e->arena.alloc(&e->ytab, (size_t)(c.num_classes + 1) * D));
    e->weights.add("y_embedder.embedding_table.weight", (int64_t)(c.num_classes + 1) * D, PK_F32, e->ytab);
  }
  if (c.extras == 78) {
    constexpr int64_t TK = 77 * 768;   // latte.py:241
    TRY(e->arena.alloc(&e->txt_w, (size_t)D * TK));
    TRY(e->arena.alloc(&e->txt_b, (size_t)D));
    TRY(e->arena.alloc(&e->txt_proj, (size_t)max_batch * D));
    TRY(e->arena.alloc(&e->cvec_t, (size_t)max_batch * D));
    TRY(e->arena.alloc(&e->iota, (size_t)max_batch));
    TRY(launch_iota(e->iota, max_batch, nullptr));
    LATTE_HIP(hipStreamSynchronize(nullptr));
    e->weights.add("text_embedding_projection.1.weight", (int64_t)D * TK, PK_F32, e->txt_w);
    e->weights.add("text_embedding_projection.1.bias", D, PK_F32, e->txt_b);
  }
  e->blocks.resize(c.depth);
  for (int i = 0; i < c.depth; ++i) {
    BlockLinears& w = e->blocks[i];
    TRY(alloc_block_linears(e->arena, w, D, e->Hm));
    const std::string p = "blocks." + std::to_string(i) + ".";
    e->weights.add(p + "attn.qkv.weight", (int64_t)3 * D * D, PK_H16, w.qkv_w);
    e->weights.add(p + "attn.qkv.bias", 3 * D, PK_F32, w.qkv_b);
    e->weights.add(p + "attn.proj.weight", (int64_t)D * D, PK_H16, w.proj_w);
    e->weights.add(p + "attn.proj.bias", D, PK_F32, w.proj_b);
    e->weights.add(p + "mlp.fc1.weight", (int64_t)e->Hm * D, PK_H16, w.fc1_w);
    e->weights.add(p + "mlp.fc1.bias", e->Hm, PK_F32, w.fc1_b);
    e->weights.add(p + "mlp.fc2.weight", (int64_t)D * e->Hm, PK_H16, w.fc2_w);
    e->weights.add(p + "mlp.fc2.bias", D, PK_F32, w.fc2_b);
    e->weights.add(p + "adaLN_modulation.1.weight", (int64_t)6 * D * D, PK_F32, e->ada_w + (size_t)i * 6 * D * D);
    e->weights.add(p + "adaLN_modulation.1.bias", 6 * D, PK_F32, e->ada_b + (size_t)i * 6 * D);
  }
  e->weights.add("final_layer.linear.weight", (int64_t)e->P * D, PK_F32_TRANSPOSE, e->fin_wt, e->P, D);
  e->weights.add("final_layer.linear.bias", e->P, PK_F32, e->fin_b);
  e->weights.add("final_layer.adaLN_modulation.1.weight", (int64_t)2 * D * D, PK_F32, e->ada_w + (size_t)c.depth * 6 * D * D);
  e->weights.add("final_layer.adaLN_modulation.1.bias", 2 * D, PK_F32, e->ada_b + (size_t)c.depth * 6 * D);

  TRY(e->weights.alloc_stage(e->arena, false));
  TRY(e->arena.alloc(&e->xres, (size_t)e->rows_pad * D));
  TRY(e->arena.alloc(&e->split_ws, (size_t)SPLIT_WS_FLOATS, false));
  TRY(e->arena.alloc(&e->zero_bias, (size_t)std::max(D, e->Hm)));
  TRY(e->arena.alloc(&e->xn, (size_t)e->rows_pad * D));
  TRY(e->arena.alloc(&e->qkv, (size_t)e->rows_pad * 3 * D));
  TRY(e->arena.alloc(&e->hbuf, (size_t)e->rows_pad * e->Hm));
  TRY(e->arena.alloc(&e->mod, (size_t)max_batch * e->nmod));
  TRY(e->arena.alloc(&e->temb0, (size_t)max_batch * D));
  TRY(e->arena.alloc(&e->cvec, (size_t)max_batch * D));
  TRY(e->arena.alloc(&e->model_out, (size_t)max_batch * e->F * e->Cout * e->H * e->H));
  TRY(e->arena.alloc(&e->noise_buf, (size_t)max_batch * e->F * e->Cin * e->H * e->H));
#undef TRY
  *out = e;
  return LATTE_OK;
}

void latte_engine_destroy(latte_engine_t* e) {
  if (!e) return;
  if (e->load_event) (void)hipEventDestroy(e->load_event);
  delete e;   // the arena frees every device block
}

int latte_engine_num_keys(const latte_engine_t* e) { return e ? e->weights.size() : 0; }
const char* latte_engine_key(const latte_engine_t* e, int i) { return e ? e->weights.key(i) : nullptr; }

int latte_engine_set_option(latte_engine_t* e, const char* name, int64_t value) {
  if (!e || !name) return fail(LATTE_ERR_INVALID, "set_option: null argument");
  const std::string k = name;
  if (k == "gemm_variant") {
    if (value < 0 || (value > 13 && value != 18 && value != 19)) return fail(LATTE_ERR_INVALID, "gemm_variant must be 0..13, 18 or 19");
    const int bn = value >= 7 && value <= 9 ? gemm_tile_n((int)value) / 4 : gemm_tile_n((int)value);   // 7-9: whole wave widths
    if (value != 0 && ((3 * e->D) % bn || e->D % bn || e->Hm % bn))
      return fail(LATTE_ERR_INVALID, "gemm_variant: every N of the model must be a multiple of the tile width");
    e->gemm_variant = (int)value;
    return LATTE_OK;
  }
  for (int gi = 0; gi < 4; ++gi) {
    static const char* names[4] = {"gemm_variant_qkv", "gemm_variant_proj", "gemm_variant_fc1", "gemm_variant_fc2"};
    if (k == names[gi]) {
      if (value < 0 || (value > 13 && value != 18 && value != 19)) return fail(LATTE_ERR_INVALID, "gemm_variant_*: must be 0..13, 18 or 19");
      e->gemm_variant_of[gi] = (int)value;
      return LATTE_OK;
    }
  }
  if (k == "gated_split_k") {
    if (value < 0 || value > 4) return fail(LATTE_ERR_INVALID, "gated_split_k: 0 (rule), 1 (off) or 2..4 splits");
    e->gated_split_k = (int)value;
    return LATTE_OK;
  }
  if (k == "gated_rmw_shape") {
    if (value < 0 || value > 1) return fail(LATTE_ERR_INVALID, "gated_rmw_shape: 0 (fragment-wise) or 1 (line-wise residual accesses of the gated GEMMs)");
    e->gated_rmw_shape = (int)value;
    return LATTE_OK;
  }
  if (k == "stream_policy") {
    if (value < 0 || value > SP_ALL)
      return fail(LATTE_ERR_INVALID, "stream_policy: bit 0 = fc1's hidden stores, bit 1 = fc2's A operand, bit 2 = attention output stores, bit 3 = the out-projection's A operand carry the nt hint (0..15)");
    e->stream_policy = (int)value;
    e->stream_policy_set = true;
    return LATTE_OK;
  }
  if (k == "fc2_temp_embed") {
    if (value < 0 || value > 1) return fail(LATTE_ERR_INVALID, "fc2_temp_embed: 0 (LayerNorm pass adds temp_embed) or 1 (the first block's fc2 epilogue does)");
    e->fc2_temp_embed = (int)value;
    return LATTE_OK;
  }
  if (k == "fuse_qkv_attn") {
    if (value < 0 || value > 31)
      return fail(LATTE_ERR_INVALID, "fuse_qkv_attn: bit 0 = spatial blocks, bit 1 = temporal blocks, bits 2-4 = schedule features off (0..31)");
    e->fuse_qkv_attn = (int)value;
    return LATTE_OK;
  }
  if (k == "guided_split") {
    if (value < 0 || value > 31)
      return fail(LATTE_ERR_INVALID, "guided_split: bit 0 / 1 = attention output / fc1 operand as f16 split pairs, bit 2 / 3 = the same with an fp8 remainder, bit 4 = fc1's operand with an fp4 remainder, in guided calls (0..31)");
    e->guided_split = (int)value;
    return LATTE_OK;
  }
  if (k == "seed") {
    e->seed = (uint64_t)value;
    e->rng_offset = 0;
    return LATTE_OK;
  }
  if (k == "train_timesteps") {
    if (value < 1 || value > (1 << 30)) return fail(LATTE_ERR_INVALID, "train_timesteps: the number of trained timesteps, >= 1");
    e->train_timesteps = (int)value;
    return LATTE_OK;
  }
  return fail(LATTE_ERR_INVALID, "set_option: unknown option '" + k + "'");
}

int latte_engine_get_option(const latte_engine_t* e, const char* name, int64_t* value) {
  if (!e || !name || !value) return fail(LATTE_ERR_INVALID, "get_option: null argument");
  const std::string k = name;
  if (k == "gemm_variant") *value = e->gemm_variant;
  else if (k == "gemm_variant_qkv") *value = e->gemm_variant_of[0];
  else if (k == "gemm_variant_proj") *value = e->gemm_variant_of[1];
  else if (k == "gemm_variant_fc1") *value = e->gemm_variant_of[2];
  else if (k == "gemm_variant_fc2") *value = e->gemm_variant_of[3];
  else if (k == "gated_split_k") *value = e->gated_split_k;
  else if (k == "gated_rmw_shape") *value = e->gated_rmw_shape;
  else if (k == "stream_policy") *value = e->stream_policy;
  else if (k == "fc2_temp_embed") *value = e->fc2_temp_embed;
  else if (k == "fuse_qkv_attn") *value = e->fuse_qkv_attn;
  else if (k == "guided_split") *value = e->guided_split;
  else if (k == "guided_split_active") *value = e->guided_split_active;
  else if (k == "guided_split_failed") *value = e->split_failed ? 1 : 0;
  else if (k == "seed") *value = (int64_t)e->seed;
  else if (k == "train_timesteps") *value = e->train_timesteps;
  else return fail(LATTE_ERR_INVALID, "get_option: unknown option '" + k + "'");
  return LATTE_OK;
}

int latte_engine_load_tensor(latte_engine_t* e, const char* key, const float* data, int64_t numel, int on_device,
                             void* stream) {
  if (!e || !key || !data) return fail(LATTE_ERR_INVALID, "load_tensor: null argument");
  hipStream_t st = (hipStream_t)stream;
  WeightSlot* slot = nullptr;
  const float* src = nullptr;
  int rc = e->weights.begin_load("load_tensor", key, data, numel, on_device, st, &slot, &src);
  if (rc) return rc;
  WeightSlot& s = *slot;
  switch (s.kind) {
    case PK_F32:
      LATTE_HIP(hipMemcpyAsync(s.dst, src, sizeof(float) * numel, hipMemcpyDeviceToDevice, st));
      break;
    case PK_F32_TRANSPOSE:
      rc = launch_transpose_f32(src, (float*)s.dst, s.rows, s.cols, st);
      break;
    case PK_H16:
      rc = launch_convert_f32_to_h16(src, (half_t*)s.dst, numel, e->cfg.compute_dtype, st);
      break;
  }
  if (rc || (rc = e->weights.end_load(s, on_device, st))) return rc;
  if (s.kind == PK_H16) {   // a block weight changed: the derived copies ([W | W], W8) are stale and must be rebuilt BEHIND this conversion
    e->split_w_ready = false;
    if (!e->load_event) LATTE_HIP(hipEventCreateWithFlags(&e->load_event, hipEventDisableTiming));
    LATTE_HIP(hipEventRecord(e->load_event, st));
  }
  if (s.key.compare(0, 11, "t_embedder.") == 0) {   // an installed timestep-embedding table was computed from the old weights
    e->temb_table_n = 0;
    e->temb_table_map.clear();
    e->temb_own_map.clear();
  }
  return LATTE_OK;
}

int latte_engine_check_weights(latte_engine_t* e) {
  if (!e) return fail(LATTE_ERR_INVALID, "check_weights: null engine");
  return e->weights.check_loaded();
}

int latte_engine_temb_table(latte_engine_t* e, const latte_schedule_t* s, float* out, void* stream) {
  if (!e || !s || !out) return fail(LATTE_ERR_INVALID, "temb_table: null argument");
  int rc = latte_engine_check_weights(e);
  if (rc) return rc;
  return compute_temb_table(e, s, out, (hipStream_t)stream);
}

int latte_engine_set_temb_table(latte_engine_t* e, const latte_schedule_t* s, const float* table, void* stream) {
  if (!e) return fail(LATTE_ERR_INVALID, "set_temb_table: null engine");
  if (!table || !s) {   // uninstall: the engine computes its own table again
    e->temb_table_n = 0;
    e->temb_table_map.clear();
    return LATTE_OK;
  }
  const int num_timesteps = s->num_timesteps;
  int rc = grow(e, &e->temb_table, &e->temb_table_cap, (int64_t)num_timesteps * e->D);
  if (rc) return rc;
  LATTE_HIP(hipMemcpyAsync(e->temb_table, table, sizeof(float) * (size_t)num_timesteps * e->D, hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
  e->temb_table_n = num_timesteps;
  e->temb_table_map = s->timestep_map;   // row i is t_embedder(timestep_map[i]): valid for this map only
  return LATTE_OK;
}

int latte_engine_set_text_embedding(latte_engine_t* e, const float* text_embedding, int batch, void* stream) {
  if (!e || !text_embedding) return fail(LATTE_ERR_INVALID, "set_text_embedding: null argument");
  if (e->cfg.extras != 78) return fail(LATTE_ERR_STATE, "set_text_embedding: the model has no text_embedding_projection (extras != 78)");
  if (batch <= 0 || batch > e->max_batch) return fail(LATTE_ERR_STATE, "set_text_embedding: batch exceeds max_batch of the engine");
  int rc = latte_engine_check_weights(e);
  if (rc) return rc;
  if ((rc = launch_text_proj(text_embedding, e->txt_w, e->txt_b, e->txt_proj, batch, e->D, 77 * 768, (hipStream_t)stream))) return rc;
  e->txt_rows = batch;
  return LATTE_OK;
}

int latte_forward(latte_engine_t* e, const float* x, const int64_t* t, const int64_t* y, int batch, float* out,
                  void* stream) {
  if (!e || !x || !t || !out) return fail(LATTE_ERR_INVALID, "forward: null argument");
  int rc = latte_engine_check_weights(e);
  if (rc) return rc;
  return run_forward(e, x, t, y, batch, false, out, (hipStream_t)stream, nullptr);
}

int latte_forward_with_cfg(latte_engine_t* e, const float* x, const int64_t* t, const int64_t* y, int batch,
                           float cfg_scale, float* out, void* stream) {
  if (!e || !x || !t || !out) return fail(LATTE_ERR_INVALID, "forward_with_cfg: null argument");
  int rc = latte_engine_check_weights(e);
  if (rc) return rc;
  if ((rc = run_forward(e, x, t, y, batch, true, out, (hipStream_t)stream, nullptr))) return rc;
  return launch_cfg_combine(out, batch / 2, e->F, e->Cout, e->H * e->H, cfg_scale, (hipStream_t)stream);
}

int latte_sampler_step_ex(const latte_schedule_t* s, int method, int index, float eta, int clip_denoised, const float* x,
                          const float* model_out, const float* noise, const float* pred_xstart_in, const float* cond_grad,
                          int predict_only, int batch, int frames, int channels, int hw, float* sample_out,
                          float* pred_xstart_out, void* stream) {
  if (!s || !x || !model_out) return fail(LATTE_ERR_INVALID, "sampler_step: null argument");
  if (predict_only ? !pred_xstart_out : !sample_out) return fail(LATTE_ERR_INVALID, "sampler_step: null output");
  if (index < 0 || index >= s->num_timesteps) return fail(LATTE_ERR_INVALID, "sampler_step: index out of range");
  if (method != LATTE_METHOD_DDPM && method != LATTE_METHOD_DDIM && method != LATTE_METHOD_DDIM_REVERSE)
    return fail(LATTE_ERR_INVALID, "sampler_step: bad method");
  if (method == LATTE_METHOD_DDIM_REVERSE && eta != 0.0f)
    return fail(LATTE_ERR_INVALID, "sampler_step: Reverse ODE only for deterministic path (eta must be 0, gd:580)");
  if (s->num_timesteps < 2) return fail(LATTE_ERR_INVALID, "sampler_step: learned-range variance needs >= 2 timesteps");
  SamplerCoefs c = make_coefs(s, method, index, eta, clip_denoised);
  if (!predict_only && method == LATTE_METHOD_DDPM && index != 0 && noise == nullptr)
    return fail(LATTE_ERR_INVALID, "sampler_step: DDPM needs noise for index > 0");
  return launch_sampler_update(c, x, model_out, step_needs_noise(method, c, index) ? noise : nullptr, batch, frames, channels, hw, 0, sample_out,
                               pred_xstart_out, (hipStream_t)stream, pred_xstart_in, cond_grad, predict_only);
}

int latte_sampler_step(const latte_schedule_t* s, int method, int index, float eta, int clip_denoised, const float* x,
                       const float* model_out, const float* noise, int batch, int frames, int channels, int hw,
                       float* sample_out, float* pred_xstart_out, void* stream) {
  return latte_sampler_step_ex(s, method, index, eta, clip_denoised, x, model_out, noise, nullptr, nullptr, 0, batch, frames,
                               channels, hw, sample_out, pred_xstart_out, stream);
}

int latte_sample_loop(latte_engine_t* e, const latte_schedule_t* s, int method, float eta, int clip_denoised,
                      float cfg_scale, float* x, const int64_t* y, int batch, int start_index, int end_index,
                      const float* noise, float* trail_sample, float* trail_x0, void* stream) {
  return latte_sample_loop_ex(e, s, method, eta, clip_denoised, cfg_scale > 1.0f ? 1 : 0 /* sample.py:51 */, cfg_scale, x, y,
                              batch, start_index, end_index, noise, trail_sample, trail_x0, stream);
}

int latte_sample_loop_ex(latte_engine_t* e, const latte_schedule_t* s, int method, float eta, int clip_denoised, int guided,
                         float cfg_scale, float* x, const int64_t* y, int batch, int start_index, int end_index,
                         const float* noise, float* trail_sample, float* trail_x0, void* stream) {
  return sampler_chain("sample_loop", e, s, method, -1, eta, clip_denoised, guided, cfg_scale, x, y, batch, start_index, end_index, nullptr,
                       noise, trail_sample, trail_x0, (hipStream_t)stream);
}

// ---- DDIM inversion (gaussian_diffusion.py:566-602 ddim_reverse_sample, stepped over ascending indices: index i carries level i to
// level i + 1)
int latte_invert_loop(latte_engine_t* e, const latte_schedule_t* s, int clip_denoised, int guided, float cfg_scale, float* x,
                      const int64_t* y, int batch, int start_index, int end_index, float* trail_sample, float* trail_x0, void* stream) {
  return sampler_chain("invert_loop", e, s, LATTE_METHOD_DDIM_REVERSE, +1, 0.0f, clip_denoised, guided, cfg_scale, x, y, batch, start_index,
                       end_index, nullptr, nullptr, trail_sample, trail_x0, (hipStream_t)stream);
}

// ---- known-region sampling: prediction, interpolation, inpainting by replacement (include/latte_amd.h)
int latte_sample_loop_known(latte_engine_t* e, const latte_schedule_t* s, int method, float eta, int clip_denoised, int guided,
                            float cfg_scale, float* x, const int64_t* y, int batch, int start_index, int end_index, const float* known,
                            const float* mask, int resample, int blend_start, const float* noise, float* trail_sample, float* trail_x0,
                            void* stream) {
  const KnownRegion kn{known, mask, resample, blend_start};
  return sampler_chain("sample_loop_known", e, s, method, -1, eta, clip_denoised, guided, cfg_scale, x, y, batch, start_index, end_index, &kn,
                       noise, trail_sample, trail_x0, (hipStream_t)stream);
}

int latte_known_chain_slabs(const latte_schedule_t* s, int method, float eta, int start_index, int end_index, int resample,
                            int blend_start, int64_t* n_slabs) {
  if (!s || !n_slabs) return fail(LATTE_ERR_INVALID, "known_chain_slabs: null argument");
  int rc = range_check("known_chain_slabs", s->num_timesteps, end_index, start_index, "learned-range variance needs >= 2 timesteps");
  if (rc) return rc;
  if ((rc = known_method_check("known_chain_slabs", method, resample))) return rc;
  int64_t n = blend_start ? 1 : 0;
  for (int i = start_index; i >= end_index; --i) {
    const SamplerCoefs c = make_coefs(s, method, i, eta, 0);
    for (int u = 1; u <= resample; ++u) n += known_slabs(method, c, i, u, resample).count();
  }
  *n_slabs = n;
  return LATTE_OK;
}

int latte_known_blend(float* x, const float* known, const float* mask, const float* noise, uint64_t seed, uint64_t offset, float a,
                      float b, int batch, int frames, int channels, int hw, int frames_inner, void* stream) {
  return launch_known_blend(x, known, mask, noise, seed, offset, a, b, batch, frames, channels, hw, frames_inner, (hipStream_t)stream);
}

}  // extern "C"

namespace {
// ---- linear samplers as a plan (include/latte_amd.h; the table is latte_amd/schedulers.py: engine_plan()): the body of
// latte_sample_plan_loop, and latte_sample_plan_loop_windows (`ws`: x, the noise rows and the trail have ws->L frames)
int plan_chain(const std::string& who, latte_engine* e, int guided, float cfg_scale, float* x, const int64_t* y, int batch, int n_evals,
               const double* plan, const float* noise, float* trail_sample, hipStream_t st, const WindowSet* ws) {
  if (!e || !x || !plan || batch <= 0 || n_evals <= 0) return fail(LATTE_ERR_INVALID, who + ": bad arguments");
  int rc = latte_engine_check_weights(e);
  if (rc) return rc;
  const bool use_cfg = guided != 0;   // forward_with_cfg semantics for ANY scale, as latte_sample_loop_ex
  if ((rc = chain_check(who, e, nullptr, batch, use_cfg, y, true, ws && ws->valid() ? ws->count() : 1))) return rc;
  const int HW = e->H * e->H;
  if (n_evals <= LATTE_PLAN_MAX_EVALS && HW % 4)   // plan_check refuses a longer table first
    return fail(LATTE_ERR_INVALID, who + ": H * W must be a multiple of 4 (16-byte accesses of the step kernel)");
  PlanInfo info;   // the engine may draw the noise of a row itself
  if ((rc = plan_check(who.c_str(), plan, n_evals, LATTE_PLAN_MAX_EVALS, e->train_timesteps, noise != nullptr, true, &info))) return rc;
  if (ws && (rc = chain_window_check(who, e, *ws, batch))) return rc;
  const int frames = ws ? ws->L : e->F, rows = ws ? batch * ws->count() : batch;   // with windows the conditioning rows are per clip
  if (ws && (rc = chain_window_prepare(e, *ws, y, batch, st, &y))) return rc;
  const size_t per = (size_t)e->F * e->Cin * HW;
  const size_t numel = (size_t)batch * frames * e->Cin * HW;   // <= rows * per <= max_batch * per: the ring and plan_xin hold it
  if (!e->plan_xin) {   // first use: the ring and the scaled model input
    for (auto& h : e->plan_hist)
      if (!h && (rc = e->arena.alloc(&h, (size_t)e->max_batch * per, false))) return rc;
    if ((rc = e->arena.alloc(&e->plan_xin, (size_t)e->max_batch * per, false))) return rc;
  }
  // ---- conditioning: t_embedder of every row (chain order), then the adaLN outputs chunk by chunk right before the rows that use them
  if ((rc = grow(e, &e->plan_temb, &e->plan_temb_cap, (int64_t)n_evals * e->D))) return rc;
  if ((rc = compute_temb_rows(e, info.ts.data(), n_evals, e->plan_temb, st))) return rc;
  ChainCond cc;
  cc.temb = e->plan_temb;
  cc.bu = e->cfg.extras == 1 ? 1 : rows;
  if ((rc = chain_row_buffers(e, n_evals, &cc))) return rc;
  // what the denoiser reads: x itself when every in_scale is 1, else in_scale * x kept beside it by the step kernel
  float* x_in = info.scaled ? e->plan_xin : x;
  if (info.scaled) {
    LATTE_HIP(hipMemcpyAsync(x_in, x, sizeof(float) * numel, hipMemcpyDeviceToDevice, st));
    if ((rc = launch_scale_f32(x_in, (float)plan[P_IN], numel, st))) return rc;
  }
  HistRing ring{{e->plan_hist[0], e->plan_hist[1], e->plan_hist[2]}};
  for (int k = 0; k < n_evals; ++k) {
    const float* mod_k;
    int mstride;
    if ((rc = chain_mod(e, &cc, y, k, n_evals - 1, st, &mod_k, &mstride))) return rc;
    const float* mo;
    if ((rc = chain_forward(e, ws, x_in, y, batch, use_cfg, mod_k, mstride, st, &mo))) return rc;
    const LinearStep s = plan_step(plan, k, n_evals, cfg_scale);
    const float* nz = nullptr;
    if (plan[(size_t)k * LATTE_PLAN_COLS + P_CN] != 0.0 && (rc = chain_noise(e, noise, k, numel, st, &nz))) return rc;
    if ((rc = launch_linear_step(x, k + 1 == n_evals ? x : x_in, mo, ring.h1(), ring.h2(), ring.h3(), nz, ring.write(), batch,
                                 e->Cin, e->Cout, frames, HW, use_cfg ? 1 : 0, s, st))) return rc;
    if (s.push) ring.push();
    if ((rc = chain_trail(trail_sample, k, x, numel, st))) return rc;
  }
  return LATTE_OK;
}
}  // namespace

extern "C" {

int latte_sample_plan_loop(latte_engine_t* e, int guided, float cfg_scale, float* x, const int64_t* y, int batch, int n_evals,
                           const double* plan, const float* noise, float* trail_sample, void* stream) {
  return plan_chain("sample_plan_loop", e, guided, cfg_scale, x, y, batch, n_evals, plan, noise, trail_sample, (hipStream_t)stream, nullptr);
}

// ---- overlapping temporal windows (include/latte_amd.h)
int latte_window_plan(int total_frames, int frames, int stride, int* starts_out, int* counts_out, int cap) {
  const WindowSet ws{total_frames, frames, stride};
  if (window_check("window_plan", ws, 4)) return -LATTE_ERR_INVALID;
  const int W = ws.count();
  if (starts_out && cap < W) return -fail(LATTE_ERR_INVALID, "window_plan: starts_out holds fewer than the windows");
  for (int w = 0; starts_out && w < W; ++w) starts_out[w] = ws.start(w);
  for (int f = 0; counts_out && f < total_frames; ++f) {
    counts_out[f] = 0;
    for (int w = 0; w < W; ++w) counts_out[f] += f >= ws.start(w) && f < ws.start(w) + frames;
  }
  return W;
}

int latte_window_gather(const float* x, float* clips, int groups, int total_frames, int frames, int stride, int channels, int hw,
                        int frames_inner, void* stream) {
  return launch_window_gather(x, clips, groups, WindowSet{total_frames, frames, stride}, channels, hw, frames_inner, (hipStream_t)stream);
}

int latte_window_merge(const float* out, float* merged, int groups, int total_frames, int frames, int stride, int channels, int hw,
                       int frames_inner, void* stream) {
  return launch_window_merge(out, merged, groups, WindowSet{total_frames, frames, stride}, channels, hw, frames_inner, (hipStream_t)stream);
}

int latte_sample_loop_windows(latte_engine_t* e, const latte_schedule_t* s, int method, float eta, int clip_denoised, int guided,
                              float cfg_scale, float* x, const int64_t* y, int batch, int start_index, int end_index, const float* noise,
                              float* trail_sample, float* trail_x0, int total_frames, int stride, void* stream) {
  if (!e) return fail(LATTE_ERR_INVALID, "sample_loop_windows: null argument");
  const WindowSet ws{total_frames, e->F, stride};
  return sampler_chain("sample_loop_windows", e, s, method, -1, eta, clip_denoised, guided, cfg_scale, x, y, batch, start_index, end_index,
                       nullptr, noise, trail_sample, trail_x0, (hipStream_t)stream, &ws);
}

int latte_sample_plan_loop_windows(latte_engine_t* e, int guided, float cfg_scale, float* x, const int64_t* y, int batch, int n_evals,
                                   const double* plan, const float* noise, float* trail_sample, int total_frames, int stride,
                                   void* stream) {
  if (!e) return fail(LATTE_ERR_INVALID, "sample_plan_loop_windows: bad arguments");
  const WindowSet ws{total_frames, e->F, stride};
  return plan_chain("sample_plan_loop_windows", e, guided, cfg_scale, x, y, batch, n_evals, plan, noise, trail_sample, (hipStream_t)stream,
                    &ws);
}

// fp32 device copies of the schedule tables for the batched-timestep kernels (one device per schedule object)
int schedule_device_tables(const latte_schedule_t* s, const float** out, hipStream_t st) {
  int dev = 0;
  LATTE_HIP(hipGetDevice(&dev));
  const int n = s->num_timesteps;
  if (s->dev_tables && s->dev_tables_device == dev) {
    *out = s->dev_tables;
    return LATTE_OK;
  }
  if (n < 2) return fail(LATTE_ERR_INVALID, "training: needs >= 2 timesteps (posterior_log_variance_clipped)");
  if (s->dev_tables) {
    (void)hipFree(s->dev_tables);
    s->dev_tables = nullptr;
  }
  std::vector<float> h((size_t)LATTE_NUM_DEV_TABLES * n);
  auto put = [&](int which, const std::vector<double>& v) {
    for (int i = 0; i < n; ++i) h[(size_t)which * n + i] = (float)v[i];
  };
  put(DT_SQRT_AC, s->sqrt_alphas_cumprod);
  put(DT_SQRT_1MAC, s->sqrt_one_minus_alphas_cumprod);
  put(DT_COEF1, s->posterior_mean_coef1);
  put(DT_COEF2, s->posterior_mean_coef2);
  put(DT_POST_LOGVAR, s->posterior_log_variance_clipped);
  put(DT_LOG_BETAS, s->log_betas);
  put(DT_SQRT_RECIP, s->sqrt_recip_alphas_cumprod);
  put(DT_SQRT_RECIPM1, s->sqrt_recipm1_alphas_cumprod);
  for (int i = 0; i < n; ++i)   // gd:298-313: FIXED_LARGE = log(append(posterior_variance[1], betas[1:])), else the clipped posterior
    h[(size_t)DT_FIXED_LOGVAR * n + i] = s->var_type == 1 ? (float)std::log(i == 0 ? s->posterior_variance[1] : s->betas[i])
                                                          : (float)s->posterior_log_variance_clipped[i];
  float* d = nullptr;
  LATTE_HIP(hipMalloc((void**)&d, h.size() * sizeof(float)));
  LATTE_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  (void)st;
  s->dev_tables = d;
  s->dev_tables_device = dev;
  *out = d;
  return LATTE_OK;
}

int latte_q_sample(const latte_schedule_t* s, const float* x_start, const float* noise, const int64_t* t, int batch,
                   int64_t numel_per_sample, float* x_t, void* stream) {
  if (!s || !x_start || !noise || !t || !x_t || batch <= 0 || numel_per_sample <= 0)
    return fail(LATTE_ERR_INVALID, "q_sample: bad arguments");
  const float* tab = nullptr;
  int rc = schedule_device_tables(s, &tab, (hipStream_t)stream);
  if (rc) return rc;
  return launch_q_sample(tab, s->num_timesteps, x_start, noise, t, batch, (size_t)numel_per_sample, x_t, (hipStream_t)stream);
}

int latte_training_losses(const latte_schedule_t* s, int loss_type, const float* x_start, const float* x_t, const float* noise,
                          const float* model_out, const int64_t* t, int batch, int frames, int channels, int hw, float* workspace,
                          int64_t workspace_floats, float* mse_out, float* vb_out, float* loss_out, void* stream) {
  if (!s || !x_start || !x_t || !noise || !model_out || !t || !workspace || !loss_out || batch <= 0)
    return fail(LATTE_ERR_INVALID, "training_losses: bad arguments");
  if (loss_type < 0 || loss_type > 3) return fail(LATTE_ERR_INVALID, "training_losses: loss_type must be 0 MSE, 1 RESCALED_MSE, 2 KL, 3 RESCALED_KL");
  const size_t per = (size_t)frames * channels * hw;
  const int blocks = training_terms_blocks(per);
  const int64_t need = (int64_t)batch * blocks * 2 + 2 * (int64_t)batch;
  if (workspace_floats < need)
    return fail(LATTE_ERR_INVALID, "training_losses: workspace too small (latte_training_workspace_floats)");
  const float* tab = nullptr;
  hipStream_t st = (hipStream_t)stream;
  int rc = schedule_device_tables(s, &tab, st);
  if (rc) return rc;
  float* partial = workspace;
  float* mse = workspace + (size_t)batch * blocks * 2;
  float* vb = mse + batch;
  if ((rc = launch_training_terms(tab, s->num_timesteps, s->mean_type, s->var_type, x_start, x_t, noise, model_out, t, batch, frames,
                                  channels, hw, partial, blocks, mse, vb, st))) return rc;
  // gd:741-793: which terms exist and how they are scaled
  const bool kl = loss_type >= 2;
  const bool has_vb = kl || s->var_type == 0;
  float vb_scale = 1.0f;
  if (loss_type == 3) vb_scale = (float)s->num_timesteps;                       // RESCALED_KL, gd:751-752
  if (loss_type == 1) vb_scale = (float)(s->num_timesteps / 1000.0);            // RESCALED_MSE, gd:771-774
  return launch_training_combine(mse, vb, has_vb ? 1 : 0, kl ? 1 : 0, vb_scale, batch, mse_out, vb_out, loss_out, st);
}

int64_t latte_training_workspace_floats(int batch, int64_t numel_per_sample) {
  if (batch <= 0 || numel_per_sample <= 0) return 0;
  return (int64_t)batch * training_terms_blocks((size_t)numel_per_sample) * 2 + 2 * (int64_t)batch;
}

// ---- likelihood evaluation (gaussian_diffusion.py:813-866 calc_bpd_loop, :686-717 _vb_terms_bpd, :797-811 _prior_bpd)
int64_t latte_bpd_workspace_floats(int batch, int64_t numel_per_sample) {
  if (batch <= 0 || numel_per_sample <= 0) return 0;
  return (int64_t)batch * training_terms_blocks((size_t)numel_per_sample) * 3;
}

int latte_prior_bpd(const latte_schedule_t* s, const float* x_start, int batch, int64_t numel_per_sample, float* out, void* stream) {
  if (!s || !x_start || !out) return fail(LATTE_ERR_INVALID, "prior_bpd: null argument");
  if (batch <= 0 || numel_per_sample <= 0) return fail(LATTE_ERR_INVALID, "prior_bpd: batch and numel_per_sample must be positive");
  const int last = s->num_timesteps - 1;   // gd:806
  return launch_prior_bpd((float)s->sqrt_alphas_cumprod[last], (float)std::log(1.0 - s->alphas_cumprod[last]) /* gd:183 */, x_start,
                          batch, (size_t)numel_per_sample, out, (hipStream_t)stream);
}

int latte_bpd_terms(const latte_schedule_t* s, int index, int clip_denoised, const float* x_start, const float* x_t, const float* noise,
                    const float* model_out, int batch, int frames, int channels, int hw, float* workspace, int64_t workspace_floats,
                    float* vb_out, float* xstart_mse_out, float* mse_out, int64_t out_stride, float* pred_xstart_out, void* stream) {
  if (!s || !x_start || !x_t || !noise || !model_out || !workspace || !vb_out || !xstart_mse_out || !mse_out)
    return fail(LATTE_ERR_INVALID, "bpd_terms: null argument");
  if (batch <= 0 || frames <= 0 || channels <= 0 || hw <= 0 || out_stride <= 0)
    return fail(LATTE_ERR_INVALID, "bpd_terms: batch, frames, channels, hw and out_stride must be positive");
  if (index < 0 || index >= s->num_timesteps) return fail(LATTE_ERR_INVALID, "bpd_terms: index out of range");
  if (s->num_timesteps < 2) return fail(LATTE_ERR_INVALID, "bpd_terms: needs >= 2 timesteps (posterior_log_variance_clipped)");
  const size_t per = (size_t)frames * channels * hw;
  if (workspace_floats < latte_bpd_workspace_floats(batch, (int64_t)per))
    return fail(LATTE_ERR_INVALID, "bpd_terms: workspace too small (latte_bpd_workspace_floats)");
  const SamplerCoefs c = make_coefs(s, LATTE_METHOD_DDPM, index, 0.0f, clip_denoised);
  return launch_bpd_terms(c, x_start, x_t, noise, model_out, batch, frames, channels, hw, workspace, training_terms_blocks(per), vb_out,
                          xstart_mse_out, mse_out, out_stride, pred_xstart_out, (hipStream_t)stream);
}

int latte_bpd_loop(latte_engine_t* e, const latte_schedule_t* s, int clip_denoised, const float* x_start, const int64_t* y, int batch,
                   int start_index, int end_index, const float* noise, float* vb, float* xstart_mse, float* mse, void* stream) {
  if (!e || !s || !x_start || !vb || !xstart_mse || !mse) return fail(LATTE_ERR_INVALID, "bpd_loop: null argument");
  int rc = latte_engine_check_weights(e);
  if (rc) return rc;
  if ((rc = range_check("bpd_loop", s->num_timesteps, end_index, start_index, "needs >= 2 timesteps (posterior_log_variance_clipped)")))
    return rc;
  if ((rc = chain_check("bpd_loop", e, s, batch, false, y, false))) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int n_run = start_index - end_index + 1;
  const size_t per = (size_t)e->F * e->Cin * e->H * e->H;
  const size_t numel = (size_t)batch * per;
  const int blocks = training_terms_blocks(per);
  ChainCond cc;
  if ((rc = chain_prepare(e, s, e->cfg.extras == 1 ? 1 : batch, n_run, st, &cc))) return rc;
  if ((rc = grow(e, &e->bpd_xt, &e->bpd_xt_cap, (int64_t)e->max_batch * (int64_t)per))) return rc;
  if ((rc = grow(e, &e->bpd_ws, &e->bpd_ws_cap, latte_bpd_workspace_floats(e->max_batch, (int64_t)per)))) return rc;
  for (int k = 0; k < n_run; ++k) {   // gd:835: t = T-1 first
    const int i = start_index - k;
    const float *mod_i, *nz;
    int mstride;
    if ((rc = chain_mod(e, &cc, y, i, end_index, st, &mod_i, &mstride))) return rc;
    if ((rc = chain_noise(e, noise, k, numel, st, &nz))) return rc;   // gd:837: one draw per step
    if ((rc = launch_q_sample_scalar((float)s->sqrt_alphas_cumprod[i], (float)s->sqrt_one_minus_alphas_cumprod[i], x_start, nz, numel,
                                     e->bpd_xt, st))) return rc;                       // gd:838
    if ((rc = run_forward(e, e->bpd_xt, nullptr, y, batch, false, e->model_out, st, nullptr, mod_i, mstride))) return rc;
    const SamplerCoefs c = make_coefs(s, LATTE_METHOD_DDPM, i, 0.0f, clip_denoised);
    if ((rc = launch_bpd_terms(c, x_start, e->bpd_xt, nz, e->model_out, batch, e->F, e->Cin, e->H * e->H, e->bpd_ws, blocks, vb + k,
                               xstart_mse + k, mse + k, n_run, nullptr, st))) return rc;   // gd:841-852
  }
  return LATTE_OK;
}

int latte_profile_forward(latte_engine_t* e, const float* x, const int64_t* t, const int64_t* y, int batch, float* out,
                          float* ms_out, int* launches_out, int n, void* stream) {
  return latte_profile_forward_ex(e, x, t, y, batch, 0, out, ms_out, launches_out, n, stream);
}

int latte_profile_forward_ex(latte_engine_t* e, const float* x, const int64_t* t, const int64_t* y, int batch, int guided, float* out,
                             float* ms_out, int* launches_out, int n, void* stream) {
  if (!e || !ms_out || !launches_out || n < LATTE_NUM_KERNEL_CLASSES) return fail(LATTE_ERR_INVALID, "profile_forward: bad arguments");
  int rc = latte_engine_check_weights(e);
  if (rc) return rc;
  EventProfile prof;   // (destroys its events on every return path)
  hipStream_t st = (hipStream_t)stream;
  rc = run_forward(e, x, t, y, batch, guided != 0, out, st, &prof);
  if (rc) return rc;
  LATTE_HIP(hipStreamSynchronize(st));
  return prof.collect("profile_forward", ms_out, launches_out, n);
}

int latte_bench_gemm(int M, int N, int K, int epi, int dtype, int variant, int iters, float* ms_per_launch, void* stream) {
  int stagger = 0, tag = 0;
  if (variant >= 1000) { tag = variant / 1000; variant %= 1000; }    // measurement: + 1000 * call-site tag (GemmArgs::tag)
  if (variant >= 100) { stagger = variant / 100; variant %= 100; }   // measurement: variant + 100 * cohorts
  if (M <= 0 || N <= 0 || K <= 0 || iters <= 0 || !ms_per_launch) return fail(LATTE_ERR_INVALID, "bench_gemm: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int64_t Mp = ((int64_t)M + 255) / 256 * 256;
  half_t *A = nullptr, *W = nullptr;
  float *bias = nullptr, *gate = nullptr, *tmp = nullptr;
  void* out = nullptr;
  const size_t out_bytes = (size_t)Mp * N * 4;
  LATTE_HIP(hipMalloc((void**)&A, (size_t)Mp * K * 2));
  LATTE_HIP(hipMalloc((void**)&W, (size_t)N * K * 2));
  LATTE_HIP(hipMalloc((void**)&bias, (size_t)N * 4));
  LATTE_HIP(hipMalloc((void**)&gate, (size_t)N * 4));
  LATTE_HIP(hipMalloc(&out, out_bytes));
  const size_t big = (size_t)Mp * K > (size_t)N * K ? (size_t)Mp * K : (size_t)N * K;
  LATTE_HIP(hipMalloc((void**)&tmp, big * 4));
  LATTE_HIP(hipMemsetAsync(out, 0, out_bytes, st));
  int rc = LATTE_OK;
  // uniform-ish random operands (guide §5.4 rule 25: never bench MFMA kernels on zero-filled data)
  if (!rc) rc = launch_fill_normal(tmp, (size_t)Mp * K, 1234, 0, st);
  if (!rc) rc = launch_convert_f32_to_h16(tmp, A, (int64_t)Mp * K, dtype, st);
  if (!rc) rc = launch_fill_normal(tmp, (size_t)N * K, 99, 0, st);
  if (!rc) rc = launch_convert_f32_to_h16(tmp, W, (int64_t)N * K, dtype, st);
  if (!rc) rc = launch_fill_normal(bias, (size_t)N, 7, 0, st);
  if (!rc) rc = launch_fill_normal(gate, (size_t)N, 8, 0, st);
  GemmArgs g{};
  g.A = A; g.W = W; g.bias = bias; g.out = out; g.gate = gate; g.M = M; g.N = N; g.K = K;
  g.gate_stride = 0; g.rows_per_sample = M; g.stagger = stagger; g.tag = tag;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  for (int i = 0; i < 3 && !rc; ++i) rc = launch_gemm(g, epi, dtype, variant, st);
  if (!rc) {
    (void)hipEventRecord(e0, st);
    for (int i = 0; i < iters && !rc; ++i) rc = launch_gemm(g, epi, dtype, variant, st);
    (void)hipEventRecord(e1, st);
    hipError_t he = hipStreamSynchronize(st);
    if (he != hipSuccess) rc = fail(LATTE_ERR_HIP, std::string("bench_gemm: ") + hipGetErrorString(he));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    *ms_per_launch = ms / iters;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(A); (void)hipFree(W); (void)hipFree(bias); (void)hipFree(gate); (void)hipFree(out); (void)hipFree(tmp);
  return rc;
}

}  // extern "C"
