/*
 * latte_amd_debug.h — per-kernel test hooks of liblatte_amd.so (C-ABI, same conventions as
 * latte_amd.h).  They exist so tests/ can check every HIP kernel against the PyTorch op sequence it
 * replaces (the reference has no tests at all).  All pointers are device pointers;
 * "half" buffers hold bf16 or f16 bit patterns according to `dtype` (LATTE_DTYPE_*).
 */
#ifndef LATTE_AMD_DEBUG_H_
#define LATTE_AMD_DEBUG_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* C[M,N] = A[M,K] W[N,K]^T with epilogue epi: 0 half=acc+bias | 1 half=gelu_tanh(acc+bias) |
 * 2 out_f32[m,n] += gate[(m / rows_per_sample) * gate_stride + n] * (acc+bias) | 3 out_f32 = acc+bias.
 * A must be allocated with rows padded to a multiple of 256.  (nn.Linear, latte.py:43,45,171)
 * variant: tile configuration as in csrc/common.h (0 = the engine's choice) + 1000 * call-site tag of a gated-residual
 * GEMM (0 attention out-projection, 1 fc2: separate kernel symbols for the profiler). */
int latte_debug_gemm(const void* A, const void* W, const float* bias, void* out, const float* gate, int M, int N,
                     int K, int gate_stride, int rows_per_sample, int epi, int dtype, int variant, void* stream);
/* The training step's GELU epilogues of the rolling 12-wave GEMM (csrc/gemm_pw.hip; needs N % 192 == 0, K % 64 == 0, K >= 128):
 * epi 13: out = u = A W^T + bias (half) and aux = gelu_tanh(u) of the rounded u (latte.py:170 through fc1, one launch);
 * epi 14: out = (A W^T + bias) * gelu_tanh'(aux) with aux = u read only (the fc2 input-gradient GEMM of train.py's backward). */
int latte_debug_gemm_gelu(const void* A, const void* W, const float* bias, void* out, void* aux, int M, int N, int K, int epi, int dtype,
                          void* stream);
/* The same product with the FP8 CORRECTION PASS of a split operand (round 6; engine option guided_split bits 2 / 3): the tile's
 * accumulators also collect  dec(A8) 2^-12 . (dec(W8) 2^-6)^T  -- A8 [Mpad, K] / W8 [N, K] bytes of OCP e4m3 codes -- on the block-
 * scaled MFMA v_mfma_scale_f32_16x16x128_f8f6f4 behind the half-precision K loop (csrc/gemm_pw.hip, rolling 12-wave kernel; f16,
 * N % 192 == 0, K % 128 == 0; epi 1 = bias + GELU -> half, epi 2 = gated fp32 read-modify-write). */
int latte_debug_gemm_lo8(const void* A, const void* W, const void* A8, const void* W8, const float* bias, void* out, const float* gate,
                         int M, int N, int K, int gate_stride, int rows_per_sample, int epi, int dtype, void* stream);
/* W8 of an f16 weight: out8[i] = e4m3(clamp(w[i] * 2^6, +-448)) (n % 4 == 0). */
int latte_debug_pack_w8(const void* w, void* out8, int64_t n, int dtype, void* stream);
/* FP4 form of the correction pass (round 6): OCP e2m1 codes, two per byte (element k in bits 4 (k & 1) of byte k >> 1), rows of
 * ((K + 255) / 256) * 128 bytes (zero padded) with ONE E8M0 scale byte per row (value = code * 2^(scale - 127)); the block-scaled MFMA runs
 * them at twice the fp8 rate.  latte_debug_pack_w4: [N, K] f16 weights -> codes + row scales; latte_debug_ln_modulate_split4: LayerNorm-
 * modulate with y [M, D] = the nearest f16 (the plain call's bits) + y4 / y4s = codes and row scales of the remainder; latte_debug_gemm_lo4:
 * the GEMM of latte_debug_gemm (epi 1 or 2) with  (A4 2^A4s) . (W4 2^W4s)^T  collected behind its f16 K loop. */
int latte_debug_pack_w4(const void* w, void* out4, void* out_scale, int N, int K, int dtype, void* stream);
int latte_debug_ln_modulate_split4(const float* x, void* y, void* y4, void* y4s, const float* shift, const float* scale, int mod_stride, int M,
                                   int D, int rows_per_sample, int dtype, void* stream);
int latte_debug_gemm_lo4(const void* A, const void* W, const void* A4, const void* A4s, const void* W4, const void* W4s, const float* bias,
                         void* out, const float* gate, int M, int N, int K, int gate_stride, int rows_per_sample, int epi, int dtype,
                         void* stream);
/* latte_debug_ln_modulate with the split output of the fp8 form: y [M, D] = the nearest f16 (bit for bit the plain kernel's output),
 * y8 [M, D] bytes = e4m3(clamp((value - y) * 2^12, +-448)). */
int latte_debug_ln_modulate_split8(const float* x, void* y, void* y8, const float* shift, const float* scale, int mod_stride, int M, int D,
                                   int rows_per_sample, int dtype, void* stream);
/* latte_debug_qkv_attention with the same split of the attention output: out [B F T, D] f16 + out8 [B F T, D] bytes. */
int latte_debug_qkv_attention_split8(const void* xn, const void* w, const float* bias, void* out, void* out8, int B, int F, int T, int D,
                                     int heads, int mode, int dtype, void* stream);
/* Attention core of latte.py:50-70 on a [rows, 3*D] qkv buffer (see AttnArgs in csrc/common.h). */
/* Host logic only (no GPU needed): the tile / kernel variant launch_gemm picks for C[M, N] = A[M, K] W[N, K]^T with epilogue
 * `epi` when none is forced (csrc/gemm.hip: gemm_resolve_variant; variants as for the "gemm_variant" engine option). */
int latte_debug_gemm_choice(int M, int N, int K, int epi);
/* Host logic only: 1 when the fused QKV projection + attention kernel takes the shape (csrc/qkv_attn.hip: head_dim 64 | 72,
 * spatial mode 0: 256 tokens per frame; temporal mode 1: 16 frames and a token count that is a multiple of 16; operands inside the
 * 4 GiB buffer-offset range), else the engine runs the separate qkv GEMM + attention kernels. */
int latte_debug_qkv_attention_fusable(int D, int heads, int F, int T, int mode, int64_t rows);
/* Host logic only: how the weight-gradient GEMM dW[N, K] = dY[M, N]^T X[M, K] splits its contraction (csrc/gemm_tn.hip):
 * returns the number of partial products, *rows_per_split (a multiple of 64) rows of M each. */
int latte_debug_gemm_tn_plan(int M, int N, int K, int* rows_per_split);
int latte_debug_attention(const void* qkv, void* out, int num_seq, int L, int heads, int hd, int U,
                          int64_t sample_stride, int64_t seq_stride, int64_t row_stride, int dtype, void* stream);
/* Text cross-attention of LatteT2V (attn2, latte_t2v.py:740-760; csrc/attention.hip: launch_cross_attention): queries from q viewed as
 * [rows, q_ld] (column head * hd + d, q_ld >= D = heads * hd, q_ld % 8 == 0), keys / values of sample s = seq / U at rows [s Lk, (s + 1) Lk)
 * of kv [num_samples Lk, 2 D] = [K | V], kbias_or_null: additive score bias fp32 [num_samples, Lk]; out [rows, D].  Sequences are addressed
 * as in latte_debug_attention.  Lk <= 128 and L >= 128 run the whole-panel kernel, everything else (and everything under
 * latte_debug_set_choice("xattn_flash", 1)) the CROSS form of the generic flash kernel. */
int latte_debug_cross_attention(const void* q, int q_ld, const void* kv, const float* kbias_or_null, void* out, int num_seq, int L, int Lk,
                                int heads, int hd, int U, int64_t sample_stride, int64_t seq_stride, int64_t row_stride, int dtype,
                                void* stream);
/* The denoiser's fp32 bookend kernels (csrc/pointwise.hip), one launch each exactly as the engines make it, behind the argument checks
 * the launchers leave to their callers (refused with LATTE_ERR_INVALID):
 *   small_linear        out[b out_stride + n] = bias[n] + sum_k f(b, k) W[n, k] (+ add_table[add_idx[b]][n] when add_table != NULL), in_mode
 *                       0: f = in[b, k], 1: f = SiLU(in[b, k]), 2: f = the timestep sinusoid [cos | sin] of t[b] (int64; latte.py:97-117);
 *                       K % 128 == 0, K <= 1152, out_stride >= N
 *   patch_embed         out[tok, :] = Wt^T pixels(tok) + bias + pos[tok % T, :], x fp32 [BF, C, H, H], Wt [C p p, D], T = (H / p)^2 tokens
 *                       per frame; D % 128 == 0, H % p == 0, 16 C p p floats of dynamic LDS within the 64 KiB default
 *   final_layer         out [M / T, Cout, H, H] = unpatchify(LN(x[m, :]) (1 + scale[s]) + shift[s]) Wt + bias), s = m / rows_per_sample, shift /
 *                       scale rows mod_stride floats apart, Wt [D, p p Cout]; D in 128 * {1, 2, 3, 4, 6, 8, 9}, H % p == 0, T == (H / p)^2,
 *                       M % T == 0, rows_per_sample > 0, mod_stride even
 *   text_proj           out[b, n] = bias[n] + sum_k SiLU(text[b, k]) W[n, k]; K % 128 == 0
 *   gated_split_reduce  x[m, n] += gate[(m / rows_per_sample) gate_stride + n] ((sum_s ws[s stride + m N + n]) + bias[n]), slabs added in
 *                       order; N % 4 == 0, stride >= M N, stride % 4 == 0
 *   adaln_single        mod[b][j][:] = tables[j][:] + t6[b][(j % 6)][:] for j < 6 nblk, then the two head rows head_table[r][:] + temb[b][:]
 *   cond_rows           out[(i, b), :] = SiLU(temb[i, :] (+ ytab[y[b], :] when ytab != NULL)), i < n_steps, b < bu
 *   mask_bias           bias[i] = (1 - mask[i]) * -10000 */
int latte_debug_small_linear(int in_mode, const float* in, const int64_t* t, const float* W, const float* bias, const float* add_table,
                             const int64_t* add_idx, float* out, int B, int N, int K, int out_stride, void* stream);
int latte_debug_patch_embed(const float* x, const float* Wt, const float* bias, const float* pos, float* out, int BF, int C, int H, int p,
                            int D, void* stream);
int latte_debug_final_layer(const float* x, const float* shift, const float* scale, int mod_stride, const float* Wt, const float* bias,
                            float* out, int M, int D, int rows_per_sample, int T, int p, int Cout, int H, void* stream);
int latte_debug_text_proj(const float* text, const float* W, const float* bias, float* out, int B, int N, int K, void* stream);
int latte_debug_gated_split_reduce(float* x, const float* ws, int splits, int64_t stride, const float* bias, const float* gate,
                                   int gate_stride, int rows_per_sample, int M, int N, void* stream);
int latte_debug_adaln_single(const float* tables, const float* head_table, const float* t6, const float* temb, float* mod, int B, int nblk,
                             int D, void* stream);
int latte_debug_cond_rows(const float* temb, const float* ytab, const int64_t* y, float* out, int n_steps, int bu, int D, void* stream);
int latte_debug_mask_bias(const float* mask, float* bias, int64_t n, void* stream);
/* The table checks of latte_sample_plan_loop and latte_t2v_guided_linear_loop (csrc/plan.h: plan_check) on a HOST plan
 * [n_evals][LATTE_PLAN_COLS], nothing else: no engine, no GPU.  t_limit: timesteps must be below it, 0 = no bound (text-to-video);
 * a row with c_noise != 0 is refused unless noise_given or may_draw_noise.  LATTE_OK or LATTE_ERR_INVALID with latte_last_error(). */
int latte_debug_plan_check(const double* plan, int n_evals, int max_evals, int64_t t_limit, int noise_given, int may_draw_noise);
/* One launch of the guided linear sampler step (csrc/pointwise.hip: linear_step_kernel<T2VRows, V>) as latte_t2v_guided_linear_loop
 * makes it: x [b, C, F, hw] in place, model_out the guidance pair's output in frame layout [(2 b) F, Cout, hw] ([negative | prompt],
 * Cout >= C, only the first C channels are read),
 *   eps = un + scale (tx - un);  m0 = m_x x + m_eps eps;  x' = c_x x + c0 m0 + c1 h1 + c2 h2 + c3 h3 + c_noise noise;
 *   x = x';  x_in = in_scale_next x' unless x_in == x;  push != 0: hist_write = m0.
 * h1 / h2 / h3 / noise may be NULL where their coefficient is 0 (refused otherwise), hist_write may be one of h1..h3 and is needed
 * only with push.  hw % 4 == 0 and 16-byte aligned buffers take the 16-byte kernel, everything else the scalar one. */
int latte_debug_t2v_linear_step(float* x, float* x_in, const float* model_out, const float* h1, const float* h2, const float* h3,
                                const float* noise, float* hist_write, int b, int C, int Cout, int F, int hw, float scale, float m_x,
                                float m_eps, float c_x, float c0, float c1, float c2, float c3, float c_noise, float in_scale_next,
                                int push, void* stream);
/* One launch of the step kernel of latte_sample_plan_loop (csrc/pointwise.hip: linear_step_kernel<ClassGuidedRows | ClassPlainRows, 4>): the formula above on the
 * class-conditional / unconditional engine's layout -- x [B, F, C, hw] in place, model_out [B, F, Cout, hw] with Cout = C or 2 C (only the
 * first C channels are read).  guided != 0: B is the doubled batch of forward_with_cfg and eps of rows b and b + B / 2 is
 * uncond + scale (cond - uncond), cond = row b of model_out's first half, uncond = the same row of its second half; every one of the B
 * rows is updated.  guided == 0: eps is the row's own output, scale is unused.  NULL / aliasing rules as above.  16-byte accesses only:
 * hw % 4 != 0, a misaligned buffer, an odd guided B or another Cout is refused. */
int latte_debug_linear_step(float* x, float* x_in, const float* model_out, const float* h1, const float* h2, const float* h3,
                            const float* noise, float* hist_write, int B, int C, int Cout, int F, int hw, int guided, float scale, float m_x,
                            float m_eps, float c_x, float c0, float c1, float c2, float c3, float c_noise, float in_scale_next, int push,
                            void* stream);
/* latte_debug_attention with the f16 + fp8-remainder output of guided calls: out [rows, D] (bit for bit the plain call's output) and
 * out8 [rows, D] bytes = e4m3(clamp((value - out) * 2^12, +-448)); f16 only, every kernel of the un-fused path (L <= 16, generic flash,
 * 128 < L <= 256, L > 256). */
int latte_debug_attention_split8(const void* qkv, void* out, void* out8, int num_seq, int L, int heads, int hd, int U, int64_t sample_stride,
                                 int64_t seq_stride, int64_t row_stride, int dtype, void* stream);
/* Fused QKV projection + attention core (csrc/qkv_attn.hip; latte.py:48-70 up to, not including, the output projection):
 * out[B F T, D] = attention(xn[B F T, D] W[3D, D]^T + bias[3D]) per (sequence, head), rows in the canonical [B, F, T] order.
 * mode 0: spatial sequences (needs T == 256), mode 1: temporal sequences (needs F == 16, T % 16 == 0); head_dim D / heads
 * must be 64 or 72.  dbg_qkv (may be NULL): half [B F T, 3D] receives the q | k | v values the kernel holds in LDS (what the
 * un-fused qkv GEMM would have written).  xn must not alias out.  flags = QkvAttnArgs::flags, schedule variants with identical
 * results: bit 0 = the next unit's first operand tile is fetched under the attention phase, bit 1 = attention-phase issue priority
 * for wave group 0 (spatial mode), bit 2 = four heads per XCD instead of all heads of every eighth sequence group (16 heads);
 * bit 8 = QkvAttnArgs::out_split: out is [B F T, 2 D] = [hi | lo], the attention output as a split operand pair (the half nearest to
 * each value and the half nearest to the remainder) -- what guided calls feed the out-projection (engine option guided_split). */
int latte_debug_qkv_attention(const void* xn, const void* w, const float* bias, void* out, void* dbg_qkv, int B, int F, int T,
                              int D, int heads, int mode, int flags, int dtype, void* stream);
/* The same launch with a phase trace (measurement): trace = int64 [8 waves][4] receives workgroup 0's shader-clock ticks in
 * {QKV projection loop, LDS image write, attention phase} summed over its units, and its unit count. */
int latte_debug_qkv_attention_trace(const void* xn, const void* w, const float* bias, void* out, void* dbg_qkv, long long* trace,
                                    int B, int F, int T, int D, int heads, int mode, int flags, int dtype, void* stream);
/* Backward of the attention core (autograd of latte.py:61-70 on the [rows, 3 D] qkv layout): dqkv [rows, 3 D] from qkv, the
 * forward output o [rows, D] and its gradient dout [rows, D]; stats: float scratch [num_seq * heads * L * 3].  Sequences are
 * addressed as in latte_debug_attention.  L <= 16 runs one wave per (sequence, head), larger L the two tile passes
 * (latte_debug_set_choice("attn_bwd_tiles", 1) forces the tile passes: test hook). */
int latte_debug_attention_bwd(const void* qkv, const void* o, const void* dout, void* dqkv, float* stats, int num_seq, int L,
                              int heads, int hd, int U, int64_t sample_stride, int64_t seq_stride, int64_t row_stride, int dtype,
                              void* stream);
/* Weight-gradient product of the training step: dW[N, K] = sum_m dY[m, n] X[m, k] (autograd of nn.Linear, latte.py:43-45) on the
 * transposed-operand GEMM of csrc/gemm_tn.hip + its fixed-order split reduction; dY half [M, N], X half [M, K], both row-major.
 * workspace: >= splits * N * K floats (256 * 256 * ceil(N/256) * ceil(K/256) * 256 is always enough). */
int latte_debug_gemm_tn(const void* dY, const void* X, float* dW, float* workspace, int64_t workspace_floats, int M, int N, int K,
                        int dtype, void* stream);
/* The same product with colsum[n] = sum_m dY[m, n] (the linear's bias gradient, autograd of nn.Linear) formed on the launch from the
 * dY fragments the 8-wave kernel holds in registers (round 6b); M % 64 == 0, N % 128 == 0, K % 128 == 0, else LATTE_ERR_INVALID.
 * workspace: >= splits * (N * K + N) floats. */
int latte_debug_gemm_tn_colsum(const void* dY, const void* X, float* dW, float* colsum, float* workspace, int64_t workspace_floats,
                               int M, int N, int K, int dtype, void* stream);
/* half y = LN(x) * (1 + scale[sample]) + shift[sample]; optional x += temp_embed[frame] first
 * (latte.py:28-29,166,179; :357-358). */
int latte_debug_ln_modulate(float* x, void* y, const float* shift, const float* scale, int mod_stride, int M, int D,
                            int rows_per_sample, const float* temp_embed, int T, int F, int dtype, void* stream);
int latte_debug_convert(const float* in, void* out, int64_t n, int dtype, void* stream);
/* Row kernels of the training step (csrc/train.hip), one launch each as the trainer makes it.  Rows are [M, D] with M a multiple of
 * rows_per_sample; per-sample vectors (gate, shift, scale) are rows of [M / rows_per_sample][stride] fp32.
 * latte_debug_gated_add_ln: x_out = x_in + gate * y (+ temp_embed[(m / T) % F] when temp_embed != NULL) and xn (half) =
 * LN(x_out) (1 + scale) + shift, eps 1e-6 (latte.py:179-180 and the next block's modulated LayerNorm). */
int latte_debug_gated_add_ln(const float* x_in, const void* y, const float* gate, int gate_stride, float* x_out, void* xn,
                             const float* shift, const float* scale, int mod_stride, int M, int D, int rows_per_sample,
                             const float* temp_embed, int T, int F, int dtype, void* stream);
/* LayerNorm + modulate backward: for y = LN(x) (1 + scale) + shift and dy (half), dx_out = dx_in + dx (dx_in may be NULL or equal
 * to dx_out, the trainer's in-place form).  dshift / dscale != NULL: per-sample sums [M / rows_per_sample][out_stride] through the
 * finalize kernel.  y2 != NULL (then gate2, dy2 and gpartial too): the gated residual's backward of the branch below on the same
 * pass, dy2 (half) = gate2 * dx_out and gpartial [M / 32][2][D] = {sum dx_out * y2, sum gate2 * dx_out} over each 32 consecutive rows.
 * workspace: >= (M / 32) * 2 * D floats (the kernel's partial rows).  rows_per_sample must be a multiple of 32, D % 4 == 0, D <= 1280. */
int latte_debug_ln_bwd(const void* dy, const float* x, const float* scale, int mod_stride, const float* dx_in, float* dx_out,
                       float* dshift, float* dscale, int out_stride, int M, int D, int rows_per_sample, const void* y2,
                       const float* gate2, int gate2_stride, void* dy2, float* gpartial, float* workspace, int64_t workspace_floats,
                       int dtype, void* stream);
/* Gated residual backward: dy (half) = gate * dx; partial [M / 32][1 + bias_partial][D] = {sum dx * y [, sum gate * dx]} over each
 * 32 consecutive rows; dgate != NULL: per-sample sums of the first, [M / rows_per_sample][out_stride], through the finalize kernel.
 * Same shape rules as latte_debug_ln_bwd. */
int latte_debug_gate_bwd(const float* dx, const void* y, const float* gate, int gate_stride, void* dy, float* partial,
                         int64_t partial_floats, float* dgate, int out_stride, int M, int D, int rows_per_sample, int bias_partial,
                         int dtype, void* stream);
/* The training step's gradient writers (csrc/train.hip, csrc/train_fin.hip), one launch sequence each exactly as the trainer makes it.
 * Common to all: accumulate 0 assigns `out`, 1 adds to what it holds (gradient accumulation); inv_scale_dev is a device pointer to ONE
 * float, the loss scale (a power of two), or NULL: the SUM -- not the accumulated-into value -- is multiplied by 1 / scale on the way out.
 *   split_reduce   out[i] (+)= sum_s partial[s * stride + i], i < n, slabs added in order (16-byte kernel for n >= 4096, n % 4 ==
 *                  stride % 4 == 0 and 16-byte aligned buffers, else the scalar kernel: the same sum in the same order)
 *   colsum_half    out[c] (+)= sum_m in[m][c] of a half [M, C] matrix (C % 8 == 0); workspace: >= ceil(M / 512) * C floats, receives the
 *                  per-512-row chunk sums; out == NULL: they stay there unreduced (what the fused stage's finalize kernel reads)
 *   rows_sum       out[c] (+)= sum_b in[b * stride + c], c < N
 *   naive_gemm     C[m scm + n scn] (+)= alpha sum_k A[m sam + k sak] B[k sbk + n sbn] (fp32, any strides); splits > 1: the contraction is
 *                  cut into ranges whose products go to ws (>= splits * M * N floats) and are reduced into a dense C (scm == N, scn == 1)
 *   embedding_bwd  dtable[idx[b]][:] += dc[b][:] (/ scale), b in order (always adds; idx: int64 [B])
 *   silu_bwd       din[i] (+)= dout[i] silu'(pre[i]); din may be dout */
int latte_debug_split_reduce(const float* partial, int splits, int64_t stride, int64_t n, float* out, int accumulate,
                             const float* inv_scale_dev, void* stream);
int latte_debug_colsum_half(const void* in, int M, int C, float* workspace, int64_t workspace_floats, float* out_or_null, int accumulate,
                            int dtype, const float* inv_scale_dev, void* stream);
int latte_debug_rows_sum(const float* in, int B, int64_t stride, int N, float* out, int accumulate, const float* inv_scale_dev, void* stream);
int latte_debug_naive_gemm(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, float* C, int64_t scm,
                           int64_t scn, int M, int N, int K, float alpha, int accumulate, int splits, float* ws, int64_t ws_floats,
                           const float* inv_scale_dev, void* stream);
int latte_debug_embedding_bwd(const float* dc, const int64_t* idx, float* dtable, int B, int D, const float* inv_scale_dev, void* stream);
int latte_debug_silu_bwd(const float* dout, const float* pre, float* din, int64_t n, int accumulate, void* stream);
/* The optimiser step (csrc/train.hip), the two launches latte_trainer_optimizer_step makes, each alone:
 *   grad_norm   stats[0] = sqrt(sum g[i]^2) (fp64 sum; partial: double [latte_debug_sumsq_blocks()] scratch), stats[1] = the coefficient
 *               AdamW multiplies every gradient with: clip ? min(max_norm / (norm + 1e-6), 1) : 1, and 0 with stats[2] = 1 when the norm is
 *               not finite (the update is skipped); stats: float [4].  scaler_or_null: the trainer's eight floats {loss scale, applied
 *               steps since it changed, applied updates, skipped updates, this call skipped, dynamic on / off, growth interval, largest
 *               scale}, advanced by the call as described above gradnorm_finalize_kernel
 *   adamw_ema   torch.optim.AdamW's single-tensor update of p with g * stats[1] (weight decay p *= 1 - lr wd first), then ema = ema decay +
 *               p (1 - decay) (ema_or_null == NULL: none), then g = 0; stats_or_null[2] != 0: p, m, v, ema untouched, g zeroed.  step >= 1:
 *               the bias corrections' step; step == 0: it is read from step_dev_or_null[0] (a device float, the trainer's count of applied
 *               updates) -- refused when that is NULL, as is step < 0.  16-byte accesses when all five buffers are 16-byte aligned. */
int latte_debug_sumsq_blocks(void);
int latte_debug_grad_norm(const float* g, int64_t n, double* partial, float max_norm, int clip, float* stats, float* scaler_or_null,
                          void* stream);
int latte_debug_adamw_ema(float* p, float* g, float* m, float* v, float* ema_or_null, int64_t n, float lr, float b1, float b2, float eps,
                          float wd, int step, float ema_decay, const float* stats_or_null, const float* step_dev_or_null, void* stream);
/* The trainer's layout and pointwise helpers (csrc/train.hip, csrc/pointwise.hip), one launch each as the trainer makes it; n >= 1:
 *   gated_add       x_out[m, :] = x_in[m, :] + gate[(m / rows_per_sample) gate_stride + :] * y[m, :] (y half [M, D]; latte.py:179-180);
 *                   D % 4 == 0, gate_stride % 4 == 0, gate_stride >= D, x_in / x_out / gate 16-byte aligned
 *   gelu            bwd 0: out = gelu_tanh(u) (dh_or_null unused); bwd 1: out = dh * gelu_tanh'(u), out may be dh (latte.py:170 and its
 *                   autograd; the un-fused form, trainer option fuse_gelu 0); half buffers of n elements, n % 4 == 0
 *   tfreq           out[b, :] = [cos(t[b] f_i) | sin(t[b] f_i)], f_i = exp(-ln(10000) i / 128), i < 128 (latte.py:97-117; t int64 [B])
 *   gather_i64      out[i] = table[idx[i]] (the spaced schedule's timestep map)
 *   unpatchify_bwd  dtok[(bf G + gh) G + gw][(i p + j) Cout + c] = dout[bf][c][gh p + i][gw p + j] (inverse of latte.py:297-310)
 *   im2col_patch    pix[(bf G + gh) G + gw][(c p + i) p + j] = x[bf][c][gh p + i][gw p + j] (the Conv2d(k = s = p) patch of a token)
 *   add_rows        dst[i] += src[i]
 *   scale_f32_dev   p[i] *= s_dev[0] (inverse 0) or p[i] *= 1 / s_dev[0] (inverse 1), s_dev a device float holding a power of two
 *   silu_rows       out[i] = SiLU(in[i]), out may be in
 *   transpose_f32   out[c rows + r] = in[r cols + c], not in place
 *   widen           out[i] = fp32(in[i]) of a half buffer */
int latte_debug_gated_add(const float* x_in, const void* y, const float* gate, int gate_stride, float* x_out, int M, int D,
                          int rows_per_sample, int dtype, void* stream);
int latte_debug_gelu(const void* u, const void* dh_or_null, void* out, int64_t n, int bwd, int dtype, void* stream);
int latte_debug_tfreq(const int64_t* t, float* out, int B, void* stream);
int latte_debug_gather_i64(const int64_t* table, const int64_t* idx, int64_t* out, int n, void* stream);
/* joint image-video micro-batch (latte_trainer_begin_joint): x / noise [B, F + N, per] -> x_video / noise_video [B, F, per] and
 * x_image / noise_image [B N, per], t_image[b N + n] = t[b] (exact copies);  terms_out[k][b] = (F terms_video[k][b] +
 * sum_n terms_image[k][b N + n]) / (F + N) for k < 3 (summed in double, rounded once) and, when out_joint is not NULL, out_joint
 * [B, F + N, per] gathered back from out_video [B, F, per] / out_image [B N, per] */
int latte_debug_joint_split(const float* x, const float* noise, const int64_t* t, float* x_video, float* noise_video, float* x_image,
                            float* noise_image, int64_t* t_image, int B, int F, int N, int64_t per, void* stream);
int latte_debug_joint_merge(const float* terms_video, const float* terms_image, float* terms_out, const float* out_video, const float* out_image,
                            float* out_joint, int B, int F, int N, int64_t per, void* stream);
int latte_debug_unpatchify_bwd(const float* dout, float* dtok, int BF, int G, int p, int Cout, void* stream);
int latte_debug_im2col_patch(const float* x, float* pix, int BF, int G, int p, int C, void* stream);
int latte_debug_add_rows(float* dst, const float* src, int64_t n, void* stream);
int latte_debug_scale_f32_dev(float* p, const float* s_dev, int inverse, int64_t n, void* stream);
int latte_debug_silu_rows(const float* in, float* out, int64_t n, void* stream);
int latte_debug_transpose_f32(const float* in, float* out, int rows, int cols, void* stream);
int latte_debug_widen(const void* in, float* out, int64_t n, int dtype, void* stream);
/* The fused finalize launch of one block stage (csrc/train_fin.hip, StageFinArgs of csrc/common.h passed flat; the pointer and int
 * arrays are HOST arrays of n_mod (<= 6) and n_bias (<= 4) entries):  per modulation chunk c, mod_src[c] holds row-run partials
 * [B rows_per_sample][mod_nsum[c]][D] of which row mod_which[c] is summed per sample -> dmod[b][c D + col] (assigned, stays in the
 * loss-scaled domain), db[c D + col] (+)= sum_b dmod / scale, dW[c D + n][k] (+)= sum_b dmod[b][c D + n] csilu[b][k] / scale;  per bias
 * sum s, bias_out[s][col] (+)= sum_r bias_src[s][r bias_stride[s] + col] / scale, col < bias_cols[s], r < bias_rows[s].  D % 64 == 0,
 * D <= 1280. */
int latte_debug_stage_finalize(const float* const* mod_src, const int* mod_nsum, const int* mod_which, int n_mod, int rows_per_sample,
                               int B, int D, float* dmod, int dmod_stride, const float* csilu, float* dW, float* db, int n_bias,
                               const float* const* bias_src, const int* bias_rows, const int* bias_stride, const int* bias_cols,
                               float* const* bias_out, const float* scaler_dev, int accumulate, void* stream);
/* dc[b][k] = sum_n dmod[b][n] W(n)[k] (assigned), W = the concatenated adaLN weights: `depth` matrices of rows6 rows at w_blocks +
 * i * blk_stride, then the final layer's nmod - depth * rows6 rows at w_final; D % 64 == 0; ws: >= ceil(nmod / 1024) * B * D floats. */
int latte_debug_adaln_dc(const float* dmod, int nmod, int B, const float* w_blocks, int64_t blk_stride, int depth, int rows6,
                         const float* w_final, int D, float* ws, int64_t ws_floats, float* dc, void* stream);
/* Narrow-operand products (final linear / patch embed): dW[p so_p + k so_k] (+)= sum_m nar[m][p] wide[m][k] / scale, nsum_out[p] (+)= sum_m
 * nar[m][p] / scale, wsum_out[k] (+)= sum_m wide[m][k] / scale (either may be NULL); nar fp32 [M, P], wide [M, D] fp32 (wide_half 0) or half
 * of `dtype`; 1 <= P <= 32, D % 4 == 0, D <= 1280; ws: >= ceil(M / 128) * (P D + P + D) floats.
 * narrow_dx: out[m][k] = half(sum_p nar[m][p] W[p][k]), W fp32 [P, D]. */
int latte_debug_narrow_outer(const float* nar, int P, const void* wide, int wide_half, int D, int M, float* dW, int64_t so_p, int64_t so_k,
                             float* nsum_out, float* wsum_out, float* ws, int64_t ws_floats, int dtype, const float* inv_scale_dev,
                             int accumulate, void* stream);
int latte_debug_narrow_dx(const float* nar, int P, const float* W, int D, int M, void* out, int dtype, void* stream);
/* The patch embed's input gradient (latte_trainer_input_grad): out [BF, C, G p, G p] = dx [BF G^2, D] W [D, C p^2] scattered to the
 * pixels, the inverse of im2col_patch; everything fp32.  inv_scale_dev: optional DEVICE float, the loss scale -- the result is
 * multiplied by 1 / *inv_scale_dev.  C p^2 a multiple of 4 up to 64 (and D % 4 == 0, D <= 1280, the weight inside 96 KiB of LDS):
 * one wave per token row, dx and W 16-byte aligned; otherwise a plain product + scatter through a temporary (synchronises). */
int latte_debug_patch_embed_dgrad(const float* dx, const float* W, float* out, int BF, int G, int p, int C, int D, const float* inv_scale_dev,
                                  void* stream);
/* The half operand copies of fp32 [N, K] weights: wn = half [N, K], wt = half [K, N].  pack_weights: every linear of every block in one
 * launch -- HOST arrays w_ptrs / wn_ptrs / wt_ptrs [blocks * 4] (block-major), the four linears' shapes N[4], K[4] shared by all blocks;
 * builds the device table and the tile plan as the trainer does, synchronises and frees the table.  pack_weight: one matrix, one launch
 * (wn or wt may be NULL). */
int latte_debug_pack_weights(const float* const* w_ptrs, const int* N, const int* K, void* const* wn_ptrs, void* const* wt_ptrs, int blocks,
                             int dtype, void* stream);
int latte_debug_pack_weight(const float* w, void* wn, void* wt, int N, int K, int dtype, void* stream);
/* LoRA kernels of csrc/train_lora.hip (rank in {4, 8, 16, 32, 64} at kernel level -- latte_trainer_lora_enable offers 4 .. 32 --; R16 = rank rounded up to a multiple of 16).
 * pack_weights_lora: latte_debug_pack_weights with W + s B A in place of W -- HOST arrays a_ptrs / b_ptrs [blocks * 4] of fp32 A [rank, K]
 * and B [N, rank] (both NULL: the linear is not targeted); the sum is fp32, rank index ascending, and B = 0 leaves W's bits.  wf_ptrs
 * != NULL: the merge form -- the fp32 sum goes to wf_ptrs[i] ([N, K], targeted linears only) and no half copy is written.
 * lora_down: out half [M, 2 R16] = the split pair [hi | lo] of v = scale * big [M, Kbig] wd [R16, Kbig]^T (wd zero-padded by the caller):
 * hi = half(v), lo = half((v - hi) * L), L = 2048 for f16 and 256 for bf16; M % 64 == 0, Kbig % 128 == 0.
 * lora_outer: small half [M, 2 R16] in that form; sum over rows m of (hi + lo / L) [m, R16] (x) big [m, Kbig] as chunked partial products (rows_per_chunk rows each, a multiple of
 * 64; latte_debug_lora_outer_plan is the trainer's choice) + the fixed-order reduction: kr == 0: out fp32 [rank, Kbig], kr != 0: out
 * fp32 [Kbig, rank]; columns rank .. R16 - 1 of hi and of lo are not stored.  accumulate / inv_scale_dev as latte_debug_split_reduce.
 * workspace >= ceil(M / rows_per_chunk) * rank * Kbig floats. */
int latte_debug_pack_weights_lora(const float* const* w_ptrs, const int* N, const int* K, void* const* wn_ptrs, void* const* wt_ptrs,
                                  float* const* wf_ptrs, const float* const* a_ptrs, const float* const* b_ptrs, int blocks, int rank,
                                  float s, int dtype, void* stream);
/* Host logic only: the adapter table latte_trainer_lora_enable(rank, alpha, target_mask) lays out for a model of `cfg` (hidden_size,
 * mlp_hidden, depth are read) -- *num_params entries, *total floats; index >= 0: that entry's key (NUL-terminated into key_out
 * [key_cap]), offset and numel.  A rank, alpha or mask that latte_trainer_lora_enable refuses is refused here with its message. */
int latte_debug_lora_table(const struct latte_model_config* cfg, int rank, float alpha, int target_mask, int index, char* key_out,
                           int key_cap, int64_t* offset, int64_t* numel, int* num_params, int64_t* total);
int latte_debug_lora_down(const void* big, const void* wd, void* out, int M, int Kbig, int rank, float scale, int dtype, void* stream);
int latte_debug_lora_outer_plan(int M, int Kbig, int* rows_per_chunk);
int latte_debug_lora_outer(const void* small, const void* big, float* out, float* workspace, int64_t workspace_floats, int M, int Kbig,
                           int rank, int rows_per_chunk, int kr, int accumulate, const float* inv_scale_dev, int dtype, void* stream);
/* d mean_b(terms["loss"]) / d model_output of GaussianDiffusion.training_losses (gaussian_diffusion.py:719-795) for the schedule's
 * model types: loss_type 0 MSE, 1 RESCALED_MSE; x_start / x_t / noise [batch, frames, channels, hw], model_out and dmodel_out
 * [batch, frames, channels (x 2 when the schedule learns sigma), hw] fp32; t: int64 [batch] timestep indices. */
int latte_debug_loss_grad(const struct latte_schedule* s, int loss_type, const float* x_start, const float* x_t, const float* noise,
                          const float* model_out, const int64_t* t, int batch, int frames, int channels, int hw, float* dmodel_out,
                          void* stream);
int latte_debug_fill_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
/* Writes, for every lane l (0..63) and element j (0..3), the LDS element INDEX that
 * ds_read_b64_tr_b16 returned when lane l supplies byte address 8*l (LDS pre-filled with
 * lds[i] = i as 16-bit values): out[l*4 + j].  Documents the transpose-read lane map on this chip. */
int latte_debug_tr16_probe(uint16_t* out, void* stream);

/* 3x3 convolution, padding 1, NHWC half: out[N,H<<ups,W<<ups,Cout] = conv(nearest_upsample^ups(in[N,H,W,Cin]), w) + bias
 * (+ res).  w is the PyTorch weight [Cout,Cin,3,3] in fp32 (packed internally).  (F.conv2d / Upsample2D) */
int latte_debug_conv3x3(const void* in, const float* w, const float* bias, const void* res, void* out, int N, int H, int W,
                        int Cin, int Cout, int ups, int dtype, void* stream);
/* GroupNorm(32 groups, eps 1e-6, affine) [+ SiLU] on NHWC half [N, HW, C]. */
int latte_debug_groupnorm(const void* x, void* y, const float* gamma, const float* beta, int N, int HW, int C, int silu,
                          int dtype, void* stream);

/* The forms the decoder's fp32 residual stream uses: out32[N,Ho,Wo,Cout] = conv(in half) + bias (+ res32), nothing rounded to
 * half; GroupNorm [+ SiLU] of an fp32 NHWC input to a half output. */
/* The 3-tap form of the convolution kernels -- the temporal Conv3d (3,1,1) of AutoencoderKLTemporalDecoder on the "image"
 * [T frames][HW pixels] of one video chunk: in half [T, HW, Cin], w_packed half [Cout, 3 * Cin] (k = ky * Cin + ci), bias [Cout],
 * res32 (may be NULL) / out32 fp32 [T, HW, Cout].  HW may exceed 65535 (512 x 512 frames). */
int latte_debug_conv3rows_f32(const void* in, const void* w_packed, const float* bias, const float* res32, float* out32, int T, int HW,
                              int Cin, int Cout, int dtype, void* stream);
int latte_debug_conv3x3_f32(const void* in, const float* w, const float* bias, const float* res32, float* out32, int N, int H,
                            int W, int Cin, int Cout, int ups, int dtype, void* stream);
int latte_debug_groupnorm_f32(const float* x, void* y, const float* gamma, const float* beta, int N, int HW, int C, int silu,
                              int dtype, void* stream);

/* launch_groupnorm (csrc/vae.hip) with its three defaulted arguments exposed: x half or (x_is_f32) fp32 NHWC [N, HW, C], C in {128, 256,
 * 512}, y half; y_lo (may be NULL) receives the f16 rounding residual of y (the split-operand convolutions' second input); eps is the
 * variance floor (1e-6 SD-VAE, 1e-5 the temporal decoder's blocks); the statistics pass uses min(max(HW / 256, 1), max_slabs) slabs.
 * stats_out (may be NULL): fp32 [N][32][2] = (mean, rstd) per sample and group, copied from the launcher's statistics buffer.
 * Refused: max_slabs < 1; max_slabs > groupnorm_max_slabs() (256) unless N == 1 -- the temporal form, one sample of T HW pixels -- and
 * then at most 64 times it; a C the kernels are not built for; buffers that are not 16-byte aligned; a dtype other than f16. */
int latte_debug_groupnorm_ex(const void* x, int x_is_f32, void* y, void* y_lo_or_null, const float* gamma, const float* beta, int N, int HW,
                             int C, int silu, float eps, int max_slabs, float* stats_out_or_null, int dtype, void* stream);
/* The decoder's small kernels (csrc/vae.hip), one launcher each; every half buffer is f16.
 * latte_debug_vae_post_quant: z fp32 NCHW [N, 4, hw] * z_scale -> post_quant_conv (w [4, 4], b [4]) -> out fp32 NHWC [N, hw, 4].
 * latte_debug_vae_conv_in: x fp32 NHWC [N, H, W, 4], w fp32 [Cout, 4, 3, 3] (packed here), bias [Cout] -> out fp32 NHWC [N, H, W, Cout];
 *   Cout must be even and at least 2 (the kernel stores channel pairs).
 * latte_debug_vae_conv_out: x half NHWC [N, H, W, C] (x_lo: its f16 rounding residual, or NULL), w fp32 [3, C, 3, 3] (packed here), bias [3]
 *   -> out_mode 0: fp32 NCHW [N, 3, H, W]; 1: uint8 NHWC [N, H, W, 3] = ((v * 0.5 + 0.5) * 255 + 0.5).clamp(0, 255) truncated
 *   (sample.py:122).  C % 8 == 0 and 27 C floats within 64 KiB of LDS; C == 128 with W % 16 == 0 runs conv_out_c128_kernel, every other
 *   shape conv_out_kernel.
 * latte_debug_vae_softmax_rows: p half [rows, L] = softmax(scale * s fp32 [rows, L]) per row; L % 64 == 0, 64 <= L <= 4096.
 * latte_debug_vae_time_conv_out: Conv3d(3, 3, (3, 1, 1), padding (1, 0, 0)) over the T frames of one video: in fp32 [T, 3, HW], w [3, 3, 3]
 *   = [co][ci][tap], bias [3] -> out_mode 0: fp32 [T, 3, HW]; 1: uint8 [T, HW, 3] (the formula above).
 * latte_debug_vae_pack_conv_t: w fp32 [Cout, Cin, 3] -> out half [Cout][3 Cin] (k = tap Cin + ci), times sigmoid(*mix) when mix != NULL;
 *   out_lo (may be NULL): the f16 rounding residual.
 * latte_debug_vae_scale_by_sigmoid: out[i] = in[i] * sigmoid(*mix), n fp32 values (mix is a device pointer, not NULL).
 * latte_debug_vae_pack_conv_w: w fp32 [Cout, Cin, 3, 3] -> out half [Cout][9 Cin] (k = (ky 3 + kx) Cin + ci); out_lo as above.
 * latte_debug_convert_split: out = f16(in), out_lo = f16(in - out), n values (launch_convert_f32_to_h16_split).
 * Each refuses NULL buffers (other than the ones marked optional) and non-positive sizes; out_mode must be 0 or 1. */
int latte_debug_vae_post_quant(const float* z, const float* w, const float* b, float* out, int N, int hw, float z_scale, void* stream);
int latte_debug_vae_conv_in(const float* x, const float* w, const float* bias, float* out, int N, int H, int W, int Cout, void* stream);
int latte_debug_vae_conv_out(const void* x, const void* x_lo_or_null, const float* w, const float* bias, void* out, int N, int H, int W, int C,
                             int out_mode, void* stream);
int latte_debug_vae_softmax_rows(const float* s, void* p, int rows, int L, float scale, void* stream);
int latte_debug_vae_time_conv_out(const float* in, const float* w, const float* bias, void* out, int T, int HW, int out_mode, void* stream);
int latte_debug_vae_pack_conv_t(const float* w, const float* mix_or_null, void* out, void* out_lo_or_null, int Cout, int Cin, void* stream);
int latte_debug_vae_scale_by_sigmoid(const float* in, float* out, int n, const float* mix, void* stream);
int latte_debug_vae_pack_conv_w(const float* w, void* out, void* out_lo_or_null, int Cout, int Cin, void* stream);
int latte_debug_convert_split(const float* in, void* out, void* out_lo, int64_t n, void* stream);

/* Runs the VAE decoder (include/latte_amd.h) up to and including stage `stop_after` and returns that stage's NHWC
 * activation (the fp32 residual stream) (trace_dims = N, H, W, C).  Stages: 0 conv_in, 1 mid.resnets.0, 2 mid.attentions.0,
 * 3 mid.resnets.1, then for up block i: three resnets and (i < 3) the upsampler -> 4..18.  Localises a divergence. */
struct latte_vae;
int latte_debug_vae_trace(struct latte_vae* v, const float* z, int n_frames, float z_scale, int stop_after, float* trace_out,
                          int64_t* trace_numel, int* trace_dims, void* stream);
/* The same for the VAE encoder (latte_vae_create_encoder; x and in_mode as latte_vae_encode).  Stages: 0 conv_in, then per down block i
 * its two resnets and (i < 3) the down-sampler -> 1..11, 12 mid.resnets.0, 13 mid.attentions.0, 14 mid.resnets.1 (NHWC fp32 stream,
 * trace_dims = N, H, W, C), 15 the moments (fp32 NCHW [N, 8, h, w], trace_dims = N, 8, h, w). */
int latte_debug_vae_encode_trace(struct latte_vae* v, const void* x, int n_frames, int in_mode, int stop_after, float* trace_out,
                                 int64_t* trace_numel, int* trace_dims, void* stream);
/* The encoder's Downsample2D convolution alone: out32 [N, Hin/2, Win/2, Cout] = conv3x3(pad(in, (0, 1, 0, 1)), stride 2) + bias (+ res32);
 * in half NHWC [N, Hin, Win, Cin], w fp32 [Cout, Cin, 3, 3] (packed to f16 here). */
int latte_debug_conv3x3_down_f32(const void* in, const float* w, const float* bias, const float* res32, float* out32, int N, int Hin,
                                 int Win, int Cin, int Cout, int dtype, void* stream);
/* encoder.conv_in alone: x (in_mode 0 fp32 NCHW [N, 3, H, W], 1 uint8 NHWC [N, H, W, 3]), w fp32 [128, 3, 3, 3] -> out fp32 NHWC [N, H, W, 128]. */
int latte_debug_vae_enc_conv_in(const void* x, int in_mode, const float* w, const float* bias, float* out, int N, int H, int W, void* stream);
/* The encoder's tail after GroupNorm + SiLU: x half NHWC [N, H, W, 512] (x_lo: its f16 rounding residual, or NULL), conv_out w fp32
 * [8, 512, 3, 3] + b [8], quant_conv qw [8, 8, 1, 1] + qb [8] -> moments fp32 NCHW [N, 8, H, W]. */
int latte_debug_vae_enc_tail(const void* x, const void* x_lo, const float* w, const float* b, const float* qw, const float* qb, float* moments,
                             int N, int H, int W, void* stream);

/* Operand-path probe (measurement): 256 workgroups x `waves` waves, every wave issues `reps` bursts of 16 loads over a
 * cache-hot 16 KB window of `src` (>= 8 MiB readable).  mode 0: buffer_load_dwordx4 ... lds, 1: buffer_load_dword ... lds,
 * 2: global_load_dwordx4 into registers, 3: 2 + ds_write_b128.  out: int64 [8][2] = {issue ticks, landed ticks} of
 * workgroup 0 (s_memtime ticks, summed over the bursts). */
int latte_debug_dma_probe(const void* src, long long* out, int mode, int waves, int reps, void* stream);

/* Kernel-choice overrides for the A/B tests (process-global; value 0 restores the library's own choice).  Every offered value
 * selects another implementation of the SAME function (results equal up to rounding):
 *   "attn_variant"    1 = the generic flash kernel for every L > 16, 5 = the streaming kernel for 128 < L <= 256 too, 12 | 13 = the
 *                     round-6c forms of the streaming kernel on 32 x 32 x 16 MFMA tiles for head dim 72, L > 256 (4 waves x 64 queries on
 *                     one wave per SIMD with the softmax inside the P V stream | that pipeline on 8 waves; measured +14 % / -1 % against the default,
 *                     DESIGN.md section 4.2)
 *   "xattn_flash"     1 = the generic flash kernel for text cross-attention instead of the whole-panel kernel
 *   "tn_kernel"       4 = the 4-wave weight-gradient GEMM;   "tn_wn" 4 = its 256 x 128 tile
 *   "attn_bwd_tiles"  1 = the tiled attention-backward kernels for 16-token sequences too, 2 = also for 64 < L <= 256 (instead of the
 *                     resident-image kernels of round 6b)
 *   "conv_kernel"     1 = the plain 128 x 128 implicit-GEMM convolution everywhere, 2 | 3 = the ping-pong 256-pixel kernel everywhere,
 *                     4 = its persistent form (round 6: bit-identical, measured 6 - 13 % slower, not a default anywhere)
 *   "vae_split"       1024 + m: which stages of the temporal decoder run split-operand convolutions -- bits 0..4 of m = the spatial resnets of
 *                     {mid block, up block 0..3} add the pass on the activation's f16 rounding residual, bits 5..9 = the temporal resnets of the
 *                     same stages run three passes (hi*hi + lo*hi + hi*lo) instead of one (csrc/vae_engine.cpp: vae_split_mask); the SD-VAE
 *                     encoder reads the same layout (bit 0 mid block, 1 + i down block i, 12 + i / 21 + i the down-sampler of block i, 11
 *                     conv_out).  A decode / encode call reads the choice once, when it starts, and runs entirely on that mask
 *   "gated_rmw_shape" latte_debug_gemm / _lo8 / _lo4 with epi 2 on the rolling 12-wave kernel: 1 = fragment-wise residual accesses (16 rows x 64 B
 *                     per instruction), 2 = line-wise (8 rows x 128 B on the whole line of a wave's span): the engine option of the same name + 1
 *   "stream_policy"   16 + m: latte_debug_gemm / _lo8 / _lo4 and latte_debug_qkv_attention run with the engine option "stream_policy" = m (0..15)
 * Anything else is refused (LATTE_ERR_INVALID).  Replaces the LATTE_* environment variables round 3 read at every launch; the
 * measurement ablations whose results are garbage (attention variants 7-10, 16-19) were removed; profiles/ keeps their logs. */
int latte_debug_set_choice(const char* name, int value);

/* T5 encoder kernels (csrc/t5.hip) one at a time.  A "pair" is two f16 arrays hi / lo of one shape: value = hi + lo / 2048.
 *   embed        x[m, :] = table[ids[m], :]
 *   rmsnorm      w * x * rsqrt(mean(x^2) + eps) of fp32 rows -> the pair (out_f32 == NULL) or fp32
 *   bucket       the bidirectional bucket of key - query = rel (host)
 *   bias_table   table[h][d] = rel[bucket(d - (max_len - 1))][h], [heads, 2 max_len - 1]; synchronises
 *   attention    qkv f16 [B L, 3 heads 64] ([q | k | v], column head * 64 + d) -> the pair [B L, heads 64]; table as above, mask fp32
 *                [B, L] or NULL
 *   gated_act    u fp32 [M, 2 F] -> the pair [M, F] of gelu_new(u[:, :F]) * u[:, F:]
 *   pack         fp32 -> pair
 *   proj         out[M, N] (fp32) += A[M, K] . W[N, K]^T on pairs; A's arrays must hold M rounded up to 256 rows; slabs: scratch of
 *                proj_splits(N, K) * M * N floats */
int latte_debug_t5_embed(const int64_t* ids, const float* table, float* x, int M, int D, int vocab, void* stream);
int latte_debug_t5_rmsnorm(float* x, const float* w, void* out_hi, void* out_lo, float* out_f32, int M, int D, float eps, void* stream);
int latte_debug_t5_bucket(int rel, int num_buckets, int max_distance);
int latte_debug_t5_bias_table(const float* rel, int heads, int num_buckets, int max_distance, int max_len, float* table, void* stream);
int latte_debug_t5_attention(const void* qkv, const float* table, const float* mask, void* out_hi, void* out_lo, int B, int L, int heads,
                             int max_len, void* stream);
int latte_debug_t5_gated_act(const float* u, void* out_hi, void* out_lo, int M, int F, void* stream);
int latte_debug_t5_pack(const float* w, void* hi, void* lo, int64_t n, void* stream);
int latte_debug_t5_proj_splits(int N, int K);
int latte_debug_t5_proj(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, float* slabs, float* out, int M, int N, int K,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
