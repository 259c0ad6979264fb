// Per-kernel test hooks (include/latte_amd_debug.h).
#include "../../include/latte_amd_debug.h"
#include "common.h"

namespace {
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
__global__ void tr16_probe_kernel(uint16_t* out) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[512];
  for (int i = threadIdx.x; i < 512; i += 64) lds[i] = (uint16_t)i;
  __syncthreads();
  const int lane = threadIdx.x;
  auto p = (__attribute__((address_space(3))) bf16x4*)((__attribute__((address_space(3))) char*)lds + 8 * lane);
  bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p);
  typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;
  u16x4 u = __builtin_bit_cast(u16x4, v);
  for (int j = 0; j < 4; ++j) out[lane * 4 + j] = u[j];
}

// ---- operand-path probe: how fast can the waves of one CU move L2-resident data towards LDS / VGPRs?
// mode 0: buffer_load_dwordx4 ... lds (16 B per lane straight into LDS), 1: buffer_load_dword ... lds (4 B per lane),
// 2: global_load_dwordx4 into VGPRs (no LDS), 3: global_load_dwordx4 + ds_write_b128.
// Every wave issues `reps` bursts of 16 instructions over its own 16 KB source window (cache-hot) and reports the
// ticks (s_memtime) it spent ISSUING them and the ticks until they had all landed.
typedef __attribute__((address_space(3))) void lds_void_t;
__global__ void __launch_bounds__(512) dma_probe_kernel(const char* src, long long* out, int mode, int reps) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, 1u << 30, 0x00020000);
  char* my = smem + wave * 16384;
  const unsigned base = ((blockIdx.x & 63) * 8 + wave) * 16384u;
  long long t_issue = 0, t_all = 0;
  typedef __attribute__((ext_vector_type(4))) unsigned int u4;
  u4 sink = {0, 0, 0, 0};
  __syncthreads();
  if (mode >= 7 && mode <= 9 && wave >= 4) {
    // companion waves (one per SIMD next to a DMA wave): back-to-back MFMAs like a GEMM compute segment.
    // mode 7: at s_setprio 1, mode 8: default priority, mode 9: default priority while the DMA waves run at priority 3
    typedef __attribute__((ext_vector_type(8))) __bf16 bf8;
    typedef __attribute__((ext_vector_type(4))) float f4;
    bf8 a, b;
    for (int i = 0; i < 8; ++i) { a[i] = (__bf16)(float)(lane + i); b[i] = (__bf16)(float)(lane - i); }
    f4 acc[16];
    for (int i = 0; i < 16; ++i) acc[i] = (f4){0.f, 0.f, 0.f, 0.f};
    if (mode == 7) __builtin_amdgcn_s_setprio(1);
    const long long t0 = (long long)__builtin_readcyclecounter();
    for (int r = 0; r < reps * 3; ++r) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[i], 0, 0, 0);
    }
    const long long t1 = (long long)__builtin_readcyclecounter();
    __builtin_amdgcn_s_setprio(0);
    f4 sum = acc[0];
    for (int i = 1; i < 16; ++i) sum += acc[i];
    if (lane == 0 && blockIdx.x == 0) {
      out[wave * 2] = t1 - t0;             // ticks for reps * 3 * 64 MFMAs
      out[wave * 2 + 1] = (long long)reps * 3 * 64;
    }
    if (sum[0] == 12345.f) out[101] = 1;
    return;
  }
  if (mode == 9) __builtin_amdgcn_s_setprio(3);
  const int dmode = (mode >= 7 && mode <= 9) ? 0 : mode;
  for (int r = 0; r < reps; ++r) {
    const long long t0 = (long long)__builtin_readcyclecounter();
    if (dmode == 0) {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(my + j * 1024), 16, lane * 16u, base + j * 1024u, 0, 0);
    } else if (dmode == 1) {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(my + j * 256), 4, lane * 4u, base + j * 256u, 0, 0);
    } else if (dmode == 10 || dmode == 11) {
      // the GEMM's operand pattern: per instruction 8 rows x 128 B (row pitch 2304 B), K tile r of an own 256-row panel,
      // a new panel every 18 K tiles: never TCP-resident.  mode 11: all workgroups of an XCD share 4 panels (L2 reuse).
      const unsigned panel = (dmode == 10 ? blockIdx.x : (blockIdx.x & 7) * 4 + ((blockIdx.x >> 3) & 3)) + 256u * ((unsigned)r / 18u % 4u);
      const unsigned so = panel * 256u * 2304u + (unsigned)(r % 18) * 128u + (unsigned)(wave & 3) * 8u * 2304u;
      const unsigned vo = (unsigned)(lane >> 3) * 2304u + (unsigned)(lane & 7) * 16u;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(my + j * 1024), 16, vo, so + (unsigned)j * 32u * 2304u, 0, 0);
    } else if (dmode == 4) {   // one M0 value for the whole burst (same LDS destination), only the source moves
#pragma unroll
      for (int j = 0; j < 16; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)my, 16, lane * 16u, base + j * 1024u, 0, 0);
    } else if (dmode == 5) {   // one M0 value, LDS destination and source moved by the instruction's immediate offset
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(my + j * 4096), 16, lane * 16u, base + j * 4096u, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(my + j * 4096), 16, lane * 16u, base + j * 4096u, 1024, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(my + j * 4096), 16, lane * 16u, base + j * 4096u, 2048, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(my + j * 4096), 16, lane * 16u, base + j * 4096u, 3072, 0);
      }
    } else if (dmode == 6) {   // global_load ... lds (flat-global addressing) instead of the buffer form
#pragma unroll
      for (int j = 0; j < 16; ++j)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + base + j * 1024 + lane * 16),
                                         (lds_void_t*)(my + j * 1024), 16, 0, 0);
    } else {
      u4 v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = *(const u4*)(src + base + j * 1024 + lane * 16);
      const long long t1 = (long long)__builtin_readcyclecounter();   // (forces the loads to have been ISSUED only)
      t_issue += t1 - t0;
      if (dmode == 3) {
#pragma unroll
        for (int j = 0; j < 16; ++j) *(u4*)(my + j * 1024 + lane * 16) = v[j];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) sink += v[j];
      }
      t_all += (long long)__builtin_readcyclecounter() - t0;
      continue;
    }
    const long long t1 = (long long)__builtin_readcyclecounter();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    t_issue += t1 - t0;
    t_all += (long long)__builtin_readcyclecounter() - t0;
  }
  if (lane == 0 && blockIdx.x == 0) {
    out[wave * 2] = t_issue;
    out[wave * 2 + 1] = t_all;
  }
  if (sink[0] == 0x12345678u && sink[1] == 1u) out[100] = sink[2];
}
}  // namespace

using namespace latte;

// latte_debug_set_choice("stream_policy", 16 | mask): the StreamPolicy bits of the debug GEMM and fused-attention entries; 0 = the default
static int debug_stream_policy() {
  const int v = debug_choice(DBG_STREAM_POLICY);
  return v ? (v & SP_ALL) : STREAM_POLICY_DEFAULT;
}

extern "C" {

// out: int64 [8 waves][2] = {ticks spent issuing, ticks until landed}, each summed over `reps` bursts of 16 instructions.
int latte_debug_dma_probe(const void* src_1gib_window, long long* out, int mode, int waves, int reps, void* stream) {
  if (waves < 1 || waves > 8) return fail(LATTE_ERR_INVALID, "dma_probe: waves must be 1..8");
  return launch_lds<dma_probe_kernel>(dim3(256), dim3(64 * waves), 8 * 16384, (hipStream_t)stream, (const char*)src_1gib_window, out, mode,
                                      reps);
}

int latte_debug_gemm(const void* A, const void* W, const float* bias, void* out, const float* gate, int M, int N, int K,
                     int gate_stride, int rows_per_sample, int epi, int dtype, int variant, void* stream) {
  GemmArgs g{};
  g.A = (const half_t*)A; g.W = (const half_t*)W; g.bias = bias; g.out = out; g.gate = gate;
  g.M = M; g.N = N; g.K = K; g.gate_stride = gate_stride; g.rows_per_sample = rows_per_sample;
  if (epi == EPI_BIAS_RES_H16) g.res = (const half_t*)gate;   // epi 5: `gate` carries the half residual [Mpad, N]
  if (variant >= 1000) { g.tag = variant / 1000; variant %= 1000; }   // + 1000 * call-site tag (GemmArgs::tag)
  // latte_debug_set_choice("gated_rmw_shape", 1 | 2): the fragment-wise | line-wise residual accesses of the rolling kernel's gated epilogue
  const int shape = debug_choice(DBG_GATED_RMW_SHAPE);
  g.rmw_mode = shape ? shape - 1 : GATED_RMW_SHAPE_DEFAULT;
  g.stream_policy = debug_stream_policy();
  return launch_gemm(g, epi, dtype, variant, (hipStream_t)stream);
}

int latte_debug_gemm_gelu(const void* A, const void* W, const float* bias, void* out, void* aux, int M, int N, int K, int epi, int dtype,
                          void* stream) {
  if (epi != EPI_BIAS_GELU_DUAL_H16 && epi != EPI_DGELU_H16) return fail(LATTE_ERR_INVALID, "gemm_gelu: epi 13 (dual GELU) or 14 (dGELU)");
  GemmArgs g{};
  g.A = (const half_t*)A; g.W = (const half_t*)W; g.bias = bias; g.out = out; g.aux = (half_t*)aux;
  g.M = M; g.N = N; g.K = K; g.rows_per_sample = M;
  return launch_gemm_pw(g, epi, dtype, 1, (hipStream_t)stream);
}

int latte_debug_gemm_lo8(const void* A, const void* W, const void* A8, const void* W8, const float* bias, void* out, const float* gate,
                         int M, int N, int K, int gate_stride, int rows_per_sample, int epi, int dtype, void* stream) {
  if (!A8 || !W8) return fail(LATTE_ERR_INVALID, "gemm_lo8: null fp8 operand");
  GemmArgs g{};
  g.A = (const half_t*)A; g.W = (const half_t*)W; g.bias = bias; g.out = out; g.gate = gate;
  g.M = M; g.N = N; g.K = K; g.gate_stride = gate_stride; g.rows_per_sample = rows_per_sample;
  g.A8 = (const uint8_t*)A8; g.W8 = (const uint8_t*)W8;
  const int shape = debug_choice(DBG_GATED_RMW_SHAPE);
  g.rmw_mode = shape ? shape - 1 : GATED_RMW_SHAPE_DEFAULT;
  g.stream_policy = debug_stream_policy();
  return launch_gemm(g, epi, dtype, 0, (hipStream_t)stream);
}

int latte_debug_gemm_lo4(const void* A, const void* W, const void* A4, const void* A4s, const void* W4, const void* W4s, const float* bias,
                         void* out, const float* gate, int M, int N, int K, int gate_stride, int rows_per_sample, int epi, int dtype,
                         void* stream) {
  if (!A4 || !A4s || !W4 || !W4s) return fail(LATTE_ERR_INVALID, "gemm_lo4: null fp4 operand");
  GemmArgs g{};
  g.A = (const half_t*)A; g.W = (const half_t*)W; g.bias = bias; g.out = out; g.gate = gate;
  g.M = M; g.N = N; g.K = K; g.gate_stride = gate_stride; g.rows_per_sample = rows_per_sample;
  g.A4 = (const uint8_t*)A4; g.A4s = (const uint8_t*)A4s; g.W4 = (const uint8_t*)W4; g.W4s = (const uint8_t*)W4s;
  const int shape = debug_choice(DBG_GATED_RMW_SHAPE);
  g.rmw_mode = shape ? shape - 1 : GATED_RMW_SHAPE_DEFAULT;
  g.stream_policy = debug_stream_policy();
  return launch_gemm(g, epi, dtype, 0, (hipStream_t)stream);
}

int latte_debug_pack_w4(const void* w, void* out4, void* out_scale, int N, int K, int dtype, void* stream) {
  return launch_pack_w4((const half_t*)w, (unsigned char*)out4, (unsigned char*)out_scale, N, K, dtype, (hipStream_t)stream);
}

int latte_debug_ln_modulate_split4(const float* x, void* y, void* y4, void* y4s, const float* shift, const float* scale, int mod_stride, int M,
                                   int D, int rows_per_sample, int dtype, void* stream) {
  return launch_ln_modulate_split4(x, (half_t*)y, (unsigned char*)y4, (unsigned char*)y4s, shift, scale, mod_stride, M, D, rows_per_sample,
                                   dtype, (hipStream_t)stream);
}

int latte_debug_pack_w8(const void* w, void* out8, int64_t n, int dtype, void* stream) {
  return launch_pack_w8((const half_t*)w, (unsigned char*)out8, n, dtype, (hipStream_t)stream);
}

int latte_debug_ln_modulate_split8(const float* x, void* y, void* y8, const float* shift, const float* scale, int mod_stride, int M, int D,
                                   int rows_per_sample, int dtype, void* stream) {
  return launch_ln_modulate(x, nullptr, (half_t*)y, shift, scale, mod_stride, M, D, rows_per_sample, nullptr, 1, 1, dtype, (hipStream_t)stream, 2,
                            (unsigned char*)y8);
}

int latte_debug_qkv_attention_split8(const void* xn, const void* w, const float* bias, void* out, void* out8, int B, int F, int T, int D,
                                     int heads, int mode, int dtype, void* stream) {
  if (heads <= 0 || D % heads) return fail(LATTE_ERR_INVALID, "qkv_attention: D must be a multiple of heads");
  QkvAttnArgs a{};
  a.xn = (const half_t*)xn; a.w = (const half_t*)w; a.bias = bias; a.out = (half_t*)out; a.out8 = (unsigned char*)out8;
  a.B = B; a.F = F; a.T = T; a.D = D; a.heads = heads; a.hd = D / heads; a.mode = mode; a.flags = 7; a.out_split = 2;
  a.scale = 1.0f / sqrtf((float)a.hd);
  return launch_qkv_attention(a, dtype, (hipStream_t)stream);
}

int latte_debug_gemm_choice(int M, int N, int K, int epi) { return gemm_resolve_variant(M, N, K, epi); }

int latte_debug_qkv_attention_fusable(int D, int heads, int F, int T, int mode, int64_t rows) {
  return heads > 0 && D % heads == 0 && qkv_attention_fusable(D, heads, D / heads, F, T, mode, rows) ? 1 : 0;
}

int latte_debug_gemm_tn_plan(int M, int N, int K, int* rows_per_split) {
  int chunk = 0;
  const int splits = gemm_tn_plan(M, N, K, &chunk);
  if (rows_per_split) *rows_per_split = chunk;
  return splits;
}

int latte_debug_attention(const void* qkv, void* out, int num_seq, int L, int heads, int hd, int U, int64_t sample_stride,
                          int64_t seq_stride, int64_t row_stride, int dtype, void* stream) {
  AttnArgs a{};
  a.qkv = (const half_t*)qkv; a.out = (half_t*)out; a.num_seq = num_seq; a.L = L; a.heads = heads; a.hd = hd;
  a.D = heads * hd; a.U = U; a.sample_stride = sample_stride; a.seq_stride = seq_stride; a.row_stride = row_stride;
  a.scale = 1.0f / sqrtf((float)hd);
  return launch_attention(a, dtype, (hipStream_t)stream);
}

int latte_debug_attention_split8(const void* qkv, void* out, void* out8, int num_seq, int L, int heads, int hd, int U, int64_t sample_stride,
                                 int64_t seq_stride, int64_t row_stride, int dtype, void* stream) {
  AttnArgs a{};
  a.qkv = (const half_t*)qkv; a.out = (half_t*)out; a.out8 = (unsigned char*)out8; a.num_seq = num_seq; a.L = L; a.heads = heads; a.hd = hd;
  a.D = heads * hd; a.U = U; a.sample_stride = sample_stride; a.seq_stride = seq_stride; a.row_stride = row_stride;
  a.scale = 1.0f / sqrtf((float)hd);
  return launch_attention(a, dtype, (hipStream_t)stream);
}

// ---- text cross-attention and the denoiser's fp32 bookend kernels: argument checks + the engines' own launchers, unchanged
int latte_debug_cross_attention(const void* q, int q_ld, const void* kv, const float* kbias_or_null, void* out, int num_seq, int L, int Lk,
                                int heads, int hd, int U, int64_t sample_stride, int64_t seq_stride, int64_t row_stride, int dtype,
                                void* stream) {
  if (!q || !kv || !out || num_seq < 1 || L < 1 || Lk < 1 || heads < 1 || U < 1 || sample_stride < 0 || seq_stride < 0 || row_stride < 1)
    return fail(LATTE_ERR_INVALID, "cross_attention: bad arguments");
  if (hd != 64 && hd != 72) return fail(LATTE_ERR_INVALID, "cross_attention: head_dim must be 64 or 72");
  if (q_ld < heads * hd || q_ld % 8) return fail(LATTE_ERR_INVALID, "cross_attention: need q_ld >= heads * hd and q_ld % 8 == 0");
  AttnArgs a{};
  a.qkv = (const half_t*)q; a.out = (half_t*)out; a.num_seq = num_seq; a.L = L; a.heads = heads; a.hd = hd; a.D = heads * hd; a.U = U;
  a.sample_stride = sample_stride; a.seq_stride = seq_stride; a.row_stride = row_stride; a.scale = 1.0f / sqrtf((float)hd);
  a.kv = (const half_t*)kv; a.kbias = kbias_or_null; a.Lk = Lk; a.q_ld = q_ld;
  return launch_cross_attention(a, dtype, (hipStream_t)stream);
}

int latte_debug_small_linear(int in_mode, const float* in, const int64_t* t, const float* W, const float* bias, const float* add_table,
                             const int64_t* add_idx, float* out, int B, int N, int K, int out_stride, void* stream) {
  if (!W || !bias || !out || B < 1 || N < 1 || K < 1 || out_stride < N || (in_mode == IN_TFREQ ? !t : !in) || (add_table && !add_idx))
    return fail(LATTE_ERR_INVALID, "small_linear: bad arguments (out_stride >= N, t in mode 2, in otherwise, add_idx with add_table)");
  return launch_small_linear(in_mode, in, t, W, bias, add_table, add_idx, out, B, N, K, out_stride, (hipStream_t)stream);
}

int latte_debug_patch_embed(const float* x, const float* Wt, const float* bias, const float* pos, float* out, int BF, int C, int H, int p,
                            int D, void* stream) {
  if (!x || !Wt || !bias || !pos || !out || BF < 1 || C < 1 || H < 1 || p < 1 || D < 1)
    return fail(LATTE_ERR_INVALID, "patch_embed: bad arguments");
  if (D % 128) return fail(LATTE_ERR_INVALID, "patch_embed: D must be a multiple of 128");
  if (H % p) return fail(LATTE_ERR_INVALID, "patch_embed: H must be a multiple of the patch size");
  if ((int64_t)16 * C * p * p * (int64_t)sizeof(float) > 65536)
    return fail(LATTE_ERR_INVALID, "patch_embed: 16 tokens x C p p floats exceed the default dynamic LDS limit (64 KiB)");
  return launch_patch_embed(x, Wt, bias, pos, out, BF, C, H, p, D, (hipStream_t)stream);
}

int latte_debug_final_layer(const float* x, const float* shift, const float* scale, int mod_stride, const float* Wt, const float* bias,
                            float* out, int M, int D, int rows_per_sample, int T, int p, int Cout, int H, void* stream) {
  if (!x || !shift || !scale || !Wt || !bias || !out || M < 1 || D < 1 || T < 1 || p < 1 || Cout < 1 || H < 1 || mod_stride < 0)
    return fail(LATTE_ERR_INVALID, "final_layer: bad arguments");
  if (D % 128) return fail(LATTE_ERR_INVALID, "final_layer: D must be a multiple of 128");
  if (H % p) return fail(LATTE_ERR_INVALID, "final_layer: H must be a multiple of the patch size");
  if (rows_per_sample <= 0) return fail(LATTE_ERR_INVALID, "final_layer: rows_per_sample must be positive");
  if (T != (H / p) * (H / p) || M % T || mod_stride % 2)
    return fail(LATTE_ERR_INVALID, "final_layer: need T == (H / p)^2, whole frames (M % T == 0) and an even mod_stride");
  return launch_final_layer(x, shift, scale, mod_stride, Wt, bias, out, M, D, rows_per_sample, T, p, Cout, H, (hipStream_t)stream);
}

int latte_debug_text_proj(const float* text, const float* W, const float* bias, float* out, int B, int N, int K, void* stream) {
  if (!text || !W || !bias || !out || B < 1 || N < 1 || K < 1) return fail(LATTE_ERR_INVALID, "text_proj: bad arguments");
  return launch_text_proj(text, W, bias, out, B, N, K, (hipStream_t)stream);
}

int latte_debug_gated_split_reduce(float* x, const float* ws, int splits, int64_t stride, const float* bias, const float* gate,
                                   int gate_stride, int rows_per_sample, int M, int N, void* stream) {
  if (!x || !ws || !bias || !gate || M < 1 || N < 1 || rows_per_sample <= 0 || gate_stride < 0 || gate_stride % 4 || stride % 4 ||
      stride < (int64_t)M * N)
    return fail(LATTE_ERR_INVALID, "gated_split_reduce: need rows_per_sample > 0, stride >= M * N, stride and gate_stride multiples of 4");
  return launch_gated_split_reduce(x, ws, splits, (size_t)stride, bias, gate, gate_stride, rows_per_sample, M, N, (hipStream_t)stream);
}

int latte_debug_adaln_single(const float* tables, const float* head_table, const float* t6, const float* temb, float* mod, int B, int nblk,
                             int D, void* stream) {
  if (!tables || !head_table || !t6 || !temb || !mod || B < 1 || nblk < 1 || D < 1) return fail(LATTE_ERR_INVALID, "adaln_single: bad arguments");
  return launch_adaln_single(tables, head_table, t6, temb, mod, B, nblk, D, (hipStream_t)stream);
}

int latte_debug_cond_rows(const float* temb, const float* ytab, const int64_t* y, float* out, int n_steps, int bu, int D, void* stream) {
  if (!temb || !out || n_steps < 1 || bu < 1 || D < 1 || (ytab && !y)) return fail(LATTE_ERR_INVALID, "cond_rows: bad arguments");
  return launch_cond_rows(temb, ytab, y, out, n_steps, bu, D, (hipStream_t)stream);
}

int latte_debug_mask_bias(const float* mask, float* bias, int64_t n, void* stream) {
  if (!mask || !bias || n < 1) return fail(LATTE_ERR_INVALID, "mask_bias: bad arguments");
  return launch_mask_bias(mask, bias, (size_t)n, (hipStream_t)stream);
}

int latte_debug_t2v_linear_step(float* x, float* x_in, const float* model_out, const float* h1, const float* h2, const float* h3,
                                const float* noise, float* hist_write, int b, int C, int Cout, int F, int hw, float scale, float m_x,
                                float m_eps, float c_x, float c0, float c1, float c2, float c3, float c_noise, float in_scale_next,
                                int push, void* stream) {
  if (!x || !x_in || !model_out || b < 1 || C < 1 || Cout < C || F < 1 || hw < 1) return fail(LATTE_ERR_INVALID, "t2v_linear_step: bad arguments");
  if ((c1 != 0.0f && !h1) || (c2 != 0.0f && !h2) || (c3 != 0.0f && !h3) || (c_noise != 0.0f && !noise) || (push && !hist_write))
    return fail(LATTE_ERR_INVALID, "t2v_linear_step: a buffer with a non-zero coefficient (or the pushed slot) is NULL");
  const LinearStep s{scale, m_x, m_eps, c_x, c0, c1, c2, c3, c_noise, in_scale_next, push ? 1 : 0};
  return launch_t2v_guided_linear_step(x, x_in, model_out, h1, h2, h3, noise, hist_write, b, C, Cout, F, hw, s, (hipStream_t)stream);
}

int latte_debug_linear_step(float* x, float* x_in, const float* model_out, const float* h1, const float* h2, const float* h3,
                            const float* noise, float* hist_write, int B, int C, int Cout, int F, int hw, int guided, float scale, float m_x,
                            float m_eps, float c_x, float c0, float c1, float c2, float c3, float c_noise, float in_scale_next, int push,
                            void* stream) {
  if (!x || !x_in || !model_out) return fail(LATTE_ERR_INVALID, "linear_step: bad arguments");
  if ((c1 != 0.0f && !h1) || (c2 != 0.0f && !h2) || (c3 != 0.0f && !h3) || (c_noise != 0.0f && !noise) || (push && !hist_write))
    return fail(LATTE_ERR_INVALID, "linear_step: a buffer with a non-zero coefficient (or the pushed slot) is NULL");
  const LinearStep s{scale, m_x, m_eps, c_x, c0, c1, c2, c3, c_noise, in_scale_next, push ? 1 : 0};
  return launch_linear_step(x, x_in, model_out, h1, h2, h3, noise, hist_write, B, C, Cout, F, hw, guided ? 1 : 0, s, (hipStream_t)stream);
}

int latte_debug_qkv_attention(const void* xn, const void* w, const float* bias, void* out, void* dbg_qkv, int B, int F, int T, int D,
                              int heads, int mode, int flags, int dtype, void* stream) {
  return latte_debug_qkv_attention_trace(xn, w, bias, out, dbg_qkv, nullptr, B, F, T, D, heads, mode, flags, dtype, stream);
}

int latte_debug_qkv_attention_trace(const void* xn, const void* w, const float* bias, void* out, void* dbg_qkv, long long* trace, int B,
                                    int F, int T, int D, int heads, int mode, int flags, int dtype, void* stream) {
  if (heads <= 0 || D % heads) return fail(LATTE_ERR_INVALID, "qkv_attention: D must be a multiple of heads");
  QkvAttnArgs a{};
  a.xn = (const half_t*)xn; a.w = (const half_t*)w; a.bias = bias; a.out = (half_t*)out; a.dbg_qkv = (half_t*)dbg_qkv;
  a.dbg_trace = trace;
  a.B = B; a.F = F; a.T = T; a.D = D; a.heads = heads; a.hd = D / heads; a.mode = mode; a.flags = flags & 255;
  a.stream_policy = debug_stream_policy();
  a.out_split = (flags >> 8) & 1;   // flags bit 8: out is [rows, 2 D] = [hi | lo] (the split-pair output of guided calls)
  a.scale = 1.0f / sqrtf((float)a.hd);
  return launch_qkv_attention(a, dtype, (hipStream_t)stream);
}

int latte_debug_attention_bwd(const void* qkv, const void* o, const void* dout, void* dqkv, float* stats, int num_seq, int L, int heads,
                               int hd, int U, int64_t sample_stride, int64_t seq_stride, int64_t row_stride, int dtype, void* stream) {
  return launch_attention_bwd((const half_t*)qkv, (const half_t*)o, (const half_t*)dout, (half_t*)dqkv, stats, num_seq, L, heads, hd, U,
                              sample_stride, seq_stride, row_stride, dtype, (hipStream_t)stream);
}

int latte_debug_gemm_tn(const void* dY, const void* X, float* dW, float* workspace, int64_t workspace_floats, int M, int N, int K,
                        int dtype, void* stream) {
  int chunk = 0;
  const int splits = gemm_tn_plan(M, N, K, &chunk);
  if ((int64_t)splits * N * K > workspace_floats) return fail(LATTE_ERR_INVALID, "gemm_tn: workspace too small");
  if (int rc = launch_gemm_tn((const half_t*)dY, (const half_t*)X, workspace, M, N, K, chunk, dtype, (hipStream_t)stream)) return rc;
  return launch_split_reduce(workspace, splits, (size_t)N * K, (size_t)N * K, dW, 0, (hipStream_t)stream);
}

// the same product with the column sums of dY riding on the launch (gemm_tn8_kernel<DT, true>: the bias gradient of the linear);
// workspace: >= splits * (N * K + N) floats.  Shapes the 8-wave kernel does not take are refused.
int latte_debug_gemm_tn_colsum(const void* dY, const void* X, float* dW, float* colsum, float* workspace, int64_t workspace_floats, int M,
                               int N, int K, int dtype, void* stream) {
  int chunk = 0;
  const int splits = gemm_tn_plan(M, N, K, &chunk);
  if (!gemm_tn8_ok(M, N, K)) return fail(LATTE_ERR_INVALID, "gemm_tn_colsum: the column sums ride on the 8-wave kernel only (M % 64, N % 128, K % 128)");
  if ((int64_t)splits * ((int64_t)N * K + N) > workspace_floats) return fail(LATTE_ERR_INVALID, "gemm_tn_colsum: workspace too small");
  float* cs = workspace + (size_t)splits * N * K;
  if (int rc = launch_gemm_tn((const half_t*)dY, (const half_t*)X, workspace, M, N, K, chunk, dtype, (hipStream_t)stream, cs)) return rc;
  if (int rc = launch_split_reduce(workspace, splits, (size_t)N * K, (size_t)N * K, dW, 0, (hipStream_t)stream)) return rc;
  return launch_split_reduce(cs, splits, (size_t)N, (size_t)N, colsum, 0, (hipStream_t)stream);
}

int latte_debug_ln_modulate(float* x, void* y, const float* shift, const float* scale, int mod_stride, int M, int D,
                            int rows_per_sample, const float* temp_embed, int T, int F, int dtype, void* stream) {
  return launch_ln_modulate(x, x, (half_t*)y, shift, scale, mod_stride, M, D, rows_per_sample, temp_embed, T, F, dtype,
                            (hipStream_t)stream);
}

int latte_debug_gated_add_ln(const float* x_in, const void* y, const float* gate, int gate_stride, float* x_out, void* xn,
                             const float* shift, const float* scale, int mod_stride, int M, int D, int rows_per_sample,
                             const float* temp_embed, int T, int F, int dtype, void* stream) {
  if (M <= 0 || rows_per_sample <= 0 || M % rows_per_sample || (temp_embed && (T <= 0 || F <= 0)))
    return fail(LATTE_ERR_INVALID, "gated_add_ln: need whole samples (M % rows_per_sample == 0) and T, F > 0 with temp_embed");
  return launch_gated_add_ln(x_in, (const half_t*)y, gate, gate_stride, x_out, (half_t*)xn, shift, scale, mod_stride, M, D,
                             rows_per_sample, temp_embed, T, F, dtype, (hipStream_t)stream);
}

// the kernels' partial rows: one per 4 runs of train_rows_per_run(rps) rows (rps % 32 == 0: 32 rows), nsum rows of D floats each
static int64_t train_partial_floats(int M, int D, int rps, int nsum) {
  return (int64_t)(M / (4 * train_rows_per_run(rps))) * nsum * D;
}

int latte_debug_ln_bwd(const void* dy, const float* x, const float* scale, int mod_stride, const float* dx_in, float* dx_out,
                       float* dshift, float* dscale, int out_stride, int M, int D, int rows_per_sample, const void* y2,
                       const float* gate2, int gate2_stride, void* dy2, float* gpartial, float* workspace, int64_t workspace_floats,
                       int dtype, void* stream) {
  if (M <= 0 || rows_per_sample <= 0 || M % rows_per_sample || D <= 0)
    return fail(LATTE_ERR_INVALID, "ln_bwd: need whole samples (M % rows_per_sample == 0)");
  if (!dshift != !dscale) return fail(LATTE_ERR_INVALID, "ln_bwd: dshift and dscale are finalized together");
  if (train_partial_floats(M, D, rows_per_sample, 2) > workspace_floats) return fail(LATTE_ERR_INVALID, "ln_bwd: workspace too small");
  return launch_ln_bwd((const half_t*)dy, x, scale, mod_stride, dx_in, dx_out, workspace, dshift, dscale, out_stride, M, D,
                       rows_per_sample, dtype, (hipStream_t)stream, (const half_t*)y2, gate2, gate2_stride, (half_t*)dy2, gpartial);
}

int latte_debug_gate_bwd(const float* dx, const void* y, const float* gate, int gate_stride, void* dy, float* partial,
                         int64_t partial_floats, float* dgate, int out_stride, int M, int D, int rows_per_sample, int bias_partial,
                         int dtype, void* stream) {
  if (M <= 0 || rows_per_sample <= 0 || M % rows_per_sample || D <= 0 || (bias_partial != 0 && bias_partial != 1))
    return fail(LATTE_ERR_INVALID, "gate_bwd: need whole samples (M % rows_per_sample == 0), bias_partial 0 or 1");
  if (train_partial_floats(M, D, rows_per_sample, 1 + bias_partial) > partial_floats)
    return fail(LATTE_ERR_INVALID, "gate_bwd: partial buffer too small");
  return launch_gate_bwd(dx, (const half_t*)y, gate, gate_stride, (half_t*)dy, partial, dgate, out_stride, M, D, rows_per_sample, dtype,
                         (hipStream_t)stream, bias_partial);
}

// ---- the training step's gradient writers: argument checks + the trainer's own launchers, unchanged
static bool bad_mode(int accumulate) { return accumulate != 0 && accumulate != 1; }

int latte_debug_split_reduce(const float* partial, int splits, int64_t stride, int64_t n, float* out, int accumulate,
                             const float* inv_scale_dev, void* stream) {
  if (!partial || !out || splits < 1 || n < 1 || stride < n || bad_mode(accumulate))
    return fail(LATTE_ERR_INVALID, "split_reduce: need splits >= 1, 1 <= n <= stride, accumulate 0 or 1");
  return launch_split_reduce(partial, splits, (size_t)stride, (size_t)n, out, accumulate, (hipStream_t)stream, inv_scale_dev);
}

int latte_debug_colsum_half(const void* in, int M, int C, float* workspace, int64_t workspace_floats, float* out_or_null, int accumulate,
                            int dtype, const float* inv_scale_dev, void* stream) {
  if (!in || !workspace || M < 1 || C < 1 || bad_mode(accumulate)) return fail(LATTE_ERR_INVALID, "colsum_half: bad arguments");
  if ((int64_t)colsum_chunks(M) * C > workspace_floats) return fail(LATTE_ERR_INVALID, "colsum_half: workspace too small");
  return launch_colsum_half((const half_t*)in, M, C, workspace, out_or_null, accumulate, dtype, (hipStream_t)stream, inv_scale_dev);
}

int latte_debug_rows_sum(const float* in, int B, int64_t stride, int N, float* out, int accumulate, const float* inv_scale_dev, void* stream) {
  if (!in || !out || B < 1 || N < 1 || stride < N || bad_mode(accumulate))
    return fail(LATTE_ERR_INVALID, "rows_sum: need B >= 1, 1 <= N <= stride, accumulate 0 or 1");
  return launch_rows_sum(in, B, (long)stride, N, out, accumulate, (hipStream_t)stream, inv_scale_dev);
}

int latte_debug_naive_gemm(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, float* C, int64_t scm,
                           int64_t scn, int M, int N, int K, float alpha, int accumulate, int splits, float* ws, int64_t ws_floats,
                           const float* inv_scale_dev, void* stream) {
  if (!A || !B || !C || M < 1 || N < 1 || K < 1 || splits < 1 || bad_mode(accumulate) || sam < 0 || sak < 0 || sbk < 0 || sbn < 0 ||
      scm < 0 || scn < 0)
    return fail(LATTE_ERR_INVALID, "naive_gemm: bad arguments");
  if (splits > 1 && ws && (int64_t)splits * M * N > ws_floats) return fail(LATTE_ERR_INVALID, "naive_gemm: workspace too small");
  return launch_naive_gemm(A, (long)sam, (long)sak, B, (long)sbk, (long)sbn, C, (long)scm, (long)scn, M, N, K, alpha, accumulate,
                           (hipStream_t)stream, splits, ws, inv_scale_dev);
}

int latte_debug_embedding_bwd(const float* dc, const int64_t* idx, float* dtable, int B, int D, const float* inv_scale_dev, void* stream) {
  if (!dc || !idx || !dtable || B < 1 || D < 1) return fail(LATTE_ERR_INVALID, "embedding_bwd: bad arguments");
  return launch_embedding_bwd(dc, idx, dtable, B, D, (hipStream_t)stream, inv_scale_dev);
}

int latte_debug_silu_bwd(const float* dout, const float* pre, float* din, int64_t n, int accumulate, void* stream) {
  if (!dout || !pre || !din || n < 1 || bad_mode(accumulate)) return fail(LATTE_ERR_INVALID, "silu_bwd: bad arguments");
  return launch_silu_bwd(dout, pre, din, (size_t)n, accumulate, (hipStream_t)stream);
}

// ---- the optimiser step and the trainer's layout / pointwise helpers
static bool misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }
static bool bad_dtype(int dtype) { return dtype != LATTE_DTYPE_BF16 && dtype != LATTE_DTYPE_F16; }

int latte_debug_sumsq_blocks(void) { return sumsq_blocks(); }

int latte_debug_grad_norm(const float* g, int64_t n, double* partial, float max_norm, int clip, float* stats, float* scaler_or_null,
                          void* stream) {
  if (!g || !partial || !stats || n < 1 || bad_mode(clip) || misaligned(g, 4) || misaligned(partial, 8))
    return fail(LATTE_ERR_INVALID, "grad_norm: bad arguments");
  return launch_grad_norm(g, (size_t)n, partial, max_norm, clip, stats, scaler_or_null, (hipStream_t)stream);
}

int latte_debug_adamw_ema(float* p, float* g, float* m, float* v, float* ema_or_null, int64_t n, float lr, float b1, float b2, float eps,
                          float wd, int step, float ema_decay, const float* stats_or_null, const float* step_dev_or_null, void* stream) {
  if (!p || !g || !m || !v || n < 1) return fail(LATTE_ERR_INVALID, "adamw_ema: bad arguments");
  if (step < 0 || (step == 0 && !step_dev_or_null))
    return fail(LATTE_ERR_INVALID, "adamw_ema: step counts from 1 (0: the device-side count, which must then be given)");
  return launch_adamw_ema(p, g, m, v, ema_or_null, (size_t)n, lr, b1, b2, eps, wd, step, ema_decay, stats_or_null, step_dev_or_null,
                          (hipStream_t)stream);
}

int latte_debug_gated_add(const float* x_in, const void* y, const float* gate, int gate_stride, float* x_out, int M, int D,
                          int rows_per_sample, int dtype, void* stream) {
  if (!x_in || !y || !gate || !x_out || M < 1 || D < 1 || rows_per_sample < 1 || gate_stride < D || gate_stride % 4 || misaligned(x_in, 16) ||
      misaligned(x_out, 16) || misaligned(gate, 16) || misaligned(y, 8))
    return fail(LATTE_ERR_INVALID, "gated_add: bad arguments (rows_per_sample > 0, gate_stride >= D and % 4 == 0, 16-byte aligned rows)");
  return launch_gated_add(x_in, (const half_t*)y, gate, gate_stride, x_out, M, D, rows_per_sample, dtype, (hipStream_t)stream);
}

int latte_debug_gelu(const void* u, const void* dh_or_null, void* out, int64_t n, int bwd, int dtype, void* stream) {
  if (!u || !out || n < 1 || n % 4 || bad_mode(bwd) || (bwd && !dh_or_null) || misaligned(u, 8) || misaligned(out, 8) ||
      misaligned(dh_or_null, 8))
    return fail(LATTE_ERR_INVALID, "gelu: bad arguments (n % 4 == 0, dh in the backward form, 8-byte aligned buffers)");
  if (bwd) return launch_gelu_bwd((const half_t*)u, (const half_t*)dh_or_null, (half_t*)out, (size_t)n, dtype, (hipStream_t)stream);
  return launch_gelu_fwd((const half_t*)u, (half_t*)out, (size_t)n, dtype, (hipStream_t)stream);
}

int latte_debug_tfreq(const int64_t* t, float* out, int B, void* stream) {
  if (!t || !out || B < 1) return fail(LATTE_ERR_INVALID, "tfreq: bad arguments");
  return launch_tfreq(t, out, B, (hipStream_t)stream);
}

int latte_debug_gather_i64(const int64_t* table, const int64_t* idx, int64_t* out, int n, void* stream) {
  if (!table || !idx || !out || n < 1) return fail(LATTE_ERR_INVALID, "gather_i64: bad arguments");
  return launch_gather_i64(table, idx, out, n, (hipStream_t)stream);
}

int latte_debug_joint_split(const float* x, const float* noise, const int64_t* t, float* x_video, float* noise_video, float* x_image,
                            float* noise_image, int64_t* t_image, int B, int F, int N, int64_t per, void* stream) {
  if (!x || !noise || !t || !x_video || !noise_video || !x_image || !noise_image || !t_image || B < 1 || F < 1 || N < 1 || per < 1)
    return fail(LATTE_ERR_INVALID, "joint_split: bad arguments");
  return launch_joint_split(x, noise, t, x_video, noise_video, x_image, noise_image, t_image, B, F, N, (size_t)per, (hipStream_t)stream);
}

int latte_debug_joint_merge(const float* terms_video, const float* terms_image, float* terms_out, const float* out_video, const float* out_image,
                            float* out_joint, int B, int F, int N, int64_t per, void* stream) {
  if (!terms_video || !terms_image || !terms_out || B < 1 || F < 1 || N < 1 || (out_joint && (!out_video || !out_image || per < 1)))
    return fail(LATTE_ERR_INVALID, "joint_merge: bad arguments");
  return launch_joint_merge(terms_video, terms_image, terms_out, out_video, out_image, out_joint, B, F, N, (size_t)per, (hipStream_t)stream);
}

static bool bad_patch_shape(int BF, int G, int p, int C) {
  return BF < 1 || G < 1 || p < 1 || C < 1 || (int64_t)p * p * C > 0x7fffffff || (int64_t)G * p > 0x7fffffff;
}
int latte_debug_unpatchify_bwd(const float* dout, float* dtok, int BF, int G, int p, int Cout, void* stream) {
  if (!dout || !dtok || bad_patch_shape(BF, G, p, Cout)) return fail(LATTE_ERR_INVALID, "unpatchify_bwd: bad arguments");
  return launch_unpatchify_bwd(dout, dtok, BF, G, p, Cout, (hipStream_t)stream);
}

int latte_debug_im2col_patch(const float* x, float* pix, int BF, int G, int p, int C, void* stream) {
  if (!x || !pix || bad_patch_shape(BF, G, p, C)) return fail(LATTE_ERR_INVALID, "im2col_patch: bad arguments");
  return launch_im2col_patch(x, pix, BF, G, p, C, (hipStream_t)stream);
}

int latte_debug_add_rows(float* dst, const float* src, int64_t n, void* stream) {
  if (!dst || !src || n < 1) return fail(LATTE_ERR_INVALID, "add_rows: bad arguments");
  return launch_add_rows(dst, src, (size_t)n, (hipStream_t)stream);
}

int latte_debug_scale_f32_dev(float* p, const float* s_dev, int inverse, int64_t n, void* stream) {
  if (!p || !s_dev || n < 1 || bad_mode(inverse)) return fail(LATTE_ERR_INVALID, "scale_f32_dev: bad arguments");
  return launch_scale_f32_dev(p, s_dev, inverse, (size_t)n, (hipStream_t)stream);
}

int latte_debug_silu_rows(const float* in, float* out, int64_t n, void* stream) {
  if (!in || !out || n < 1) return fail(LATTE_ERR_INVALID, "silu_rows: bad arguments");
  return launch_silu_rows(in, out, (size_t)n, (hipStream_t)stream);
}

int latte_debug_transpose_f32(const float* in, float* out, int rows, int cols, void* stream) {
  if (!in || !out || rows < 1 || cols < 1 || in == out) return fail(LATTE_ERR_INVALID, "transpose_f32: bad arguments (not in place)");
  return launch_transpose_f32(in, out, rows, cols, (hipStream_t)stream);
}

int latte_debug_widen(const void* in, float* out, int64_t n, int dtype, void* stream) {
  if (!in || !out || n < 1 || bad_dtype(dtype)) return fail(LATTE_ERR_INVALID, "widen: bad arguments");
  return launch_convert_h16_to_f32((const half_t*)in, out, n, dtype, (hipStream_t)stream);
}

int latte_debug_stage_finalize(const float* const* mod_src, const int* mod_nsum, const int* mod_which, int n_mod, int rows_per_sample,
                               int B, int D, float* dmod, int dmod_stride, const float* csilu, float* dW, float* db, int n_bias,
                               const float* const* bias_src, const int* bias_rows, const int* bias_stride, const int* bias_cols,
                               float* const* bias_out, const float* scaler_dev, int accumulate, void* stream) {
  if (n_mod < 0 || n_mod > 6 || n_bias < 0 || n_bias > 4)
    return fail(LATTE_ERR_INVALID, "stage_finalize: at most 6 modulation chunks and 4 bias sums");
  if (B < 1 || D < 1 || rows_per_sample < 1 || bad_mode(accumulate) || (n_mod && (!mod_src || !mod_nsum || !mod_which || !dmod || !csilu ||
      !dW || !db || dmod_stride < n_mod * D)) || (n_bias && (!bias_src || !bias_rows || !bias_stride || !bias_cols || !bias_out)))
    return fail(LATTE_ERR_INVALID, "stage_finalize: bad arguments");
  StageFinArgs a{};
  for (int c = 0; c < n_mod; ++c) {
    if (!mod_src[c] || mod_nsum[c] < 1 || mod_which[c] < 0 || mod_which[c] >= mod_nsum[c])
      return fail(LATTE_ERR_INVALID, "stage_finalize: modulation chunk needs a source and 0 <= which < nsum");
    a.mod_src[c] = mod_src[c]; a.mod_nsum[c] = mod_nsum[c]; a.mod_which[c] = mod_which[c];
  }
  for (int s = 0; s < n_bias; ++s) {
    if (!bias_src[s] || !bias_out[s] || bias_rows[s] < 1 || bias_cols[s] < 1 || bias_stride[s] < bias_cols[s])
      return fail(LATTE_ERR_INVALID, "stage_finalize: bias sum needs buffers, rows >= 1 and 1 <= cols <= stride");
    a.bias_src[s] = bias_src[s]; a.bias_rows[s] = bias_rows[s]; a.bias_stride[s] = bias_stride[s]; a.bias_cols[s] = bias_cols[s];
    a.bias_out[s] = bias_out[s];
  }
  a.n_mod = n_mod; a.rows_per_sample = rows_per_sample; a.B = B; a.D = D; a.dmod = dmod; a.dmod_stride = dmod_stride; a.csilu = csilu;
  a.dW = dW; a.db = db; a.n_bias = n_bias; a.scaler = scaler_dev; a.accumulate = accumulate;
  return launch_stage_finalize(a, (hipStream_t)stream);
}

int latte_debug_adaln_dc(const float* dmod, int nmod, int B, const float* w_blocks, int64_t blk_stride, int depth, int rows6,
                         const float* w_final, int D, float* ws, int64_t ws_floats, float* dc, void* stream) {
  if (!dmod || !w_blocks || !w_final || !ws || !dc || B < 1 || D < 1 || depth < 0 || rows6 < 1 || nmod < 1 ||
      (int64_t)depth * rows6 > nmod || blk_stride < (int64_t)rows6 * D)
    return fail(LATTE_ERR_INVALID, "adaln_dc: need depth * rows6 <= nmod and blk_stride >= rows6 * D");
  if ((int64_t)adaln_dc_splits(nmod) * B * D > ws_floats) return fail(LATTE_ERR_INVALID, "adaln_dc: workspace too small");
  return launch_adaln_dc(dmod, nmod, B, w_blocks, (long)blk_stride, depth, rows6, w_final, D, ws, dc, (hipStream_t)stream);
}

int latte_debug_narrow_outer(const float* nar, int P, const void* wide, int wide_half, int D, int M, float* dW, int64_t so_p, int64_t so_k,
                             float* nsum_out, float* wsum_out, float* ws, int64_t ws_floats, int dtype, const float* inv_scale_dev,
                             int accumulate, void* stream) {
  if (!nar || !wide || !dW || !ws || M < 1 || P < 1 || D < 1 || bad_mode(accumulate) ||
      !((so_p == D && so_k == 1) || (so_p == 1 && so_k == P)))
    return fail(LATTE_ERR_INVALID, "narrow_outer: bad arguments (output layouts: (so_p, so_k) = (D, 1) or (1, P))");
  if ((int64_t)narrow_blocks(M) * ((int64_t)P * D + P + D) > ws_floats) return fail(LATTE_ERR_INVALID, "narrow_outer: workspace too small");
  return launch_narrow_outer(nar, P, wide, wide_half, D, M, dW, (long)so_p, (long)so_k, nsum_out, wsum_out, ws, dtype, inv_scale_dev,
                             (hipStream_t)stream, accumulate);
}

int latte_debug_narrow_dx(const float* nar, int P, const float* W, int D, int M, void* out, int dtype, void* stream) {
  if (!nar || !W || !out || M < 1) return fail(LATTE_ERR_INVALID, "narrow_dx: bad arguments");
  return launch_narrow_dx(nar, P, W, D, M, (half_t*)out, dtype, (hipStream_t)stream);
}

int latte_debug_patch_embed_dgrad(const float* dx, const float* W, float* out, int BF, int G, int p, int C, int D, const float* inv_scale_dev,
                                  void* stream) {
  if (!dx || !W || !out || bad_patch_shape(BF, G, p, C) || D < 1) return fail(LATTE_ERR_INVALID, "patch_embed_dgrad: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (patch_embed_dgrad_fast(p, C, D)) return launch_patch_embed_dgrad(dx, W, out, BF, G, p, C, D, nullptr, inv_scale_dev, st);
  float* ws = nullptr;   // the wide form's [BF G^2][C p^2] product
  LATTE_HIP(hipMalloc((void**)&ws, (size_t)BF * G * G * C * p * p * sizeof(float)));
  const int rc = launch_patch_embed_dgrad(dx, W, out, BF, G, p, C, D, ws, inv_scale_dev, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(ws);
  return rc;
}

int latte_debug_pack_weights(const float* const* w_ptrs, const int* N, const int* K, void* const* wn_ptrs, void* const* wt_ptrs, int blocks,
                             int dtype, void* stream) {
  if (!w_ptrs || !N || !K || !wn_ptrs || !wt_ptrs || blocks < 1) return fail(LATTE_ERR_INVALID, "pack_weights: bad arguments");
  PackPlan pl{};
  int t0 = 0;
  for (int j = 0; j < 4; ++j) {   // tiles of the four linears of one block, as latte_trainer_create lays them out
    if (N[j] < 1 || K[j] < 1) return fail(LATTE_ERR_INVALID, "pack_weights: bad shape");
    pl.tile0[j] = t0;
    t0 += ((N[j] + 31) / 32) * ((K[j] + 31) / 32);
  }
  pl.tiles_per_block = t0;
  std::vector<PackDesc> h((size_t)blocks * 4);
  for (int i = 0; i < blocks * 4; ++i) {
    if (!w_ptrs[i] || !wn_ptrs[i] || !wt_ptrs[i]) return fail(LATTE_ERR_INVALID, "pack_weights: null tensor");
    h[i] = PackDesc{w_ptrs[i], (half_t*)wn_ptrs[i], (half_t*)wt_ptrs[i], N[i & 3], K[i & 3]};
  }
  hipStream_t st = (hipStream_t)stream;
  PackDesc* descs = nullptr;
  LATTE_HIP(hipMalloc((void**)&descs, h.size() * sizeof(PackDesc)));
  int rc = LATTE_OK;
  if (hipMemcpy(descs, h.data(), h.size() * sizeof(PackDesc), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(LATTE_ERR_HIP, "pack_weights: table upload failed");
  if (!rc) rc = launch_pack_weights(descs, blocks, pl, dtype, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(descs);
  return rc;
}

int latte_debug_pack_weights_lora(const float* const* w_ptrs, const int* N, const int* K, void* const* wn_ptrs, void* const* wt_ptrs,
                                  float* const* wf_ptrs, const float* const* a_ptrs, const float* const* b_ptrs, int blocks, int rank,
                                  float s, int dtype, void* stream) {
  if (!w_ptrs || !N || !K || !a_ptrs || !b_ptrs || blocks < 1 || (!wf_ptrs && (!wn_ptrs || !wt_ptrs)))
    return fail(LATTE_ERR_INVALID, "pack_weights_lora: bad arguments");
  PackPlan pl{};
  int t0 = 0;
  for (int j = 0; j < 4; ++j) {
    if (N[j] < 1 || K[j] < 1) return fail(LATTE_ERR_INVALID, "pack_weights_lora: bad shape");
    pl.tile0[j] = t0;
    t0 += ((N[j] + 31) / 32) * ((K[j] + 31) / 32);
  }
  pl.tiles_per_block = t0;
  std::vector<LoraPackDesc> h((size_t)blocks * 4);
  for (int i = 0; i < blocks * 4; ++i) {
    if (!w_ptrs[i] || (wf_ptrs ? !wf_ptrs[i] : (!wn_ptrs[i] || !wt_ptrs[i])) || !a_ptrs[i] != !b_ptrs[i])
      return fail(LATTE_ERR_INVALID, "pack_weights_lora: null tensor");
    h[i] = LoraPackDesc{w_ptrs[i], wf_ptrs ? nullptr : (half_t*)wn_ptrs[i], wf_ptrs ? nullptr : (half_t*)wt_ptrs[i],
                        wf_ptrs ? wf_ptrs[i] : nullptr, N[i & 3], K[i & 3], a_ptrs[i], b_ptrs[i], nullptr, nullptr};
  }
  hipStream_t st = (hipStream_t)stream;
  LoraPackDesc* descs = nullptr;
  LATTE_HIP(hipMalloc((void**)&descs, h.size() * sizeof(LoraPackDesc)));
  int rc = LATTE_OK;
  if (hipMemcpy(descs, h.data(), h.size() * sizeof(LoraPackDesc), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(LATTE_ERR_HIP, "pack_weights_lora: table upload failed");
  if (!rc) rc = launch_pack_weights_lora(descs, blocks, pl, rank, s, dtype, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(descs);
  return rc;
}

int latte_debug_lora_down(const void* big, const void* wd, void* out, int M, int Kbig, int rank, float scale, int dtype, void* stream) {
  if (!big || !wd || !out) return fail(LATTE_ERR_INVALID, "lora_down: null argument");
  return launch_lora_down((const half_t*)big, (const half_t*)wd, (half_t*)out, M, Kbig, rank, scale, dtype, (hipStream_t)stream);
}

int latte_debug_lora_outer_plan(int M, int Kbig, int* rows_per_chunk) {
  if (M < 64 || Kbig < 128 || !rows_per_chunk) return fail(LATTE_ERR_INVALID, "lora_outer_plan: bad arguments");
  return lora_outer_plan(M, Kbig, rows_per_chunk);
}

int latte_debug_lora_outer(const void* small, const void* big, float* out, float* workspace, int64_t workspace_floats, int M, int Kbig,
                           int rank, int rows_per_chunk, int kr, int accumulate, const float* inv_scale_dev, int dtype, void* stream) {
  if (!small || !big || !out || !workspace || rows_per_chunk <= 0 || M <= 0 || rank <= 0 || Kbig <= 0)
    return fail(LATTE_ERR_INVALID, "lora_outer: bad arguments");
  const int chunks = (M + rows_per_chunk - 1) / rows_per_chunk;
  const size_t n = (size_t)rank * Kbig;
  if ((int64_t)(chunks * n) > workspace_floats) return fail(LATTE_ERR_INVALID, "lora_outer: workspace too small");
  if (int rc = launch_lora_outer((const half_t*)small, (const half_t*)big, workspace, M, Kbig, rank, rows_per_chunk, kr, dtype,
                                 (hipStream_t)stream)) return rc;
  return launch_split_reduce(workspace, chunks, n, n, out, accumulate ? 1 : 0, (hipStream_t)stream, inv_scale_dev);
}

int latte_debug_pack_weight(const float* w, void* wn, void* wt, int N, int K, int dtype, void* stream) {
  if (!w || N < 1 || K < 1) return fail(LATTE_ERR_INVALID, "pack_weight: bad arguments");
  return launch_pack_weight(w, (half_t*)wn, (half_t*)wt, N, K, dtype, (hipStream_t)stream);
}

int latte_debug_loss_grad(const latte_schedule* s, int loss_type, const float* x_start, const float* x_t, const float* noise,
                          const float* model_out, const int64_t* t, int batch, int frames, int channels, int hw, float* dmodel_out,
                          void* stream) {
  if (!s || !x_start || !x_t || !noise || !model_out || !t || !dmodel_out || batch <= 0 || frames <= 0 || channels <= 0 || hw <= 0)
    return fail(LATTE_ERR_INVALID, "loss_grad: bad arguments");
  if (loss_type != 0 && loss_type != 1) return fail(LATTE_ERR_INVALID, "loss_grad: loss_type must be 0 MSE or 1 RESCALED_MSE");
  const float* tab = nullptr;
  if (int rc = schedule_device_tables(s, &tab, (hipStream_t)stream)) return rc;
  const float vb_scale = loss_type == 1 ? (float)(s->num_timesteps / 1000.0) : 1.0f;   // as latte_trainer_forward_backward
  return launch_loss_grad(tab, s->num_timesteps, s->mean_type, s->var_type, x_start, x_t, noise, model_out, t, batch, frames, channels,
                          hw, vb_scale, dmodel_out, (hipStream_t)stream);
}

int latte_debug_convert(const float* in, void* out, int64_t n, int dtype, void* stream) {
  return launch_convert_f32_to_h16(in, (half_t*)out, n, dtype, (hipStream_t)stream);
}

int latte_debug_fill_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
  return launch_fill_normal(out, (size_t)n, seed, offset, (hipStream_t)stream);
}

int latte_debug_conv3x3(const void* in, const float* w, const float* bias, const void* res, void* out, int N, int H, int W,
                        int Cin, int Cout, int ups, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  half_t *wp = nullptr, *zeros = nullptr;
  LATTE_HIP(hipMalloc((void**)&wp, (size_t)Cout * Cin * 9 * 2));
  LATTE_HIP(hipMalloc((void**)&zeros, 64));
  LATTE_HIP(hipMemsetAsync(zeros, 0, 64, st));
  int rc = launch_pack_conv_w(w, wp, Cout, Cin, dtype, st);
  if (!rc) rc = launch_conv3x3((const half_t*)in, wp, bias, (const half_t*)res, (half_t*)out, zeros, N, H, W, Cin, Cout, ups, dtype, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(wp);
  (void)hipFree(zeros);
  return rc;
}

/* The decoder's fp32-stream forms: out32 = conv(in) + bias (+ res32), and GroupNorm of an fp32 input. */
// The 3-tap form of the convolution kernels (the temporal Conv3d (3,1,1) of AutoencoderKLTemporalDecoder on the "image" [T frames][HW
// pixels]): in half [T, HW, Cin], w_packed half [Cout, 3 * Cin] (k = ky * Cin + ci), fp32 residual / output [T, HW, Cout].
int latte_debug_conv3rows_f32(const void* in, const void* w_packed, const float* bias, const float* res32, float* out32, int T, int HW,
                              int Cin, int Cout, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  half_t* zeros = nullptr;
  LATTE_HIP(hipMalloc((void**)&zeros, 64));
  LATTE_HIP(hipMemsetAsync(zeros, 0, 64, st));
  int rc = launch_conv3x3((const half_t*)in, (const half_t*)w_packed, bias, nullptr, nullptr, zeros, 1, T, HW, Cin, Cout, 0, dtype, st, res32, out32, 1);
  (void)hipStreamSynchronize(st);
  (void)hipFree(zeros);
  return rc;
}

int latte_debug_conv3x3_f32(const void* in, const float* w, const float* bias, const float* res32, float* out32, int N, int H,
                            int W, int Cin, int Cout, int ups, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  half_t *wp = nullptr, *zeros = nullptr;
  LATTE_HIP(hipMalloc((void**)&wp, (size_t)Cout * Cin * 9 * 2));
  LATTE_HIP(hipMalloc((void**)&zeros, 64));
  LATTE_HIP(hipMemsetAsync(zeros, 0, 64, st));
  int rc = launch_pack_conv_w(w, wp, Cout, Cin, dtype, st);
  if (!rc) rc = launch_conv3x3((const half_t*)in, wp, bias, nullptr, nullptr, zeros, N, H, W, Cin, Cout, ups, dtype, st, res32, out32);
  (void)hipStreamSynchronize(st);
  (void)hipFree(wp);
  (void)hipFree(zeros);
  return rc;
}

int latte_debug_conv3x3_down_f32(const void* in, const float* w, const float* bias, const float* res32, float* out32, int N, int Hin,
                                 int Win, int Cin, int Cout, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  half_t *wp = nullptr, *zeros = nullptr;
  LATTE_HIP(hipMalloc((void**)&wp, (size_t)Cout * Cin * 9 * 2));
  LATTE_HIP(hipMalloc((void**)&zeros, 64));
  LATTE_HIP(hipMemsetAsync(zeros, 0, 64, st));
  int rc = launch_pack_conv_w(w, wp, Cout, Cin, dtype, st);
  if (!rc) rc = launch_conv3x3((const half_t*)in, wp, bias, nullptr, nullptr, zeros, N, Hin, Win, Cin, Cout, 0, dtype, st, res32, out32, 0, 1);
  (void)hipStreamSynchronize(st);
  (void)hipFree(wp);
  (void)hipFree(zeros);
  return rc;
}

int latte_debug_vae_enc_conv_in(const void* x, int in_mode, const float* w, const float* bias, float* out, int N, int H, int W, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  float* wt = nullptr;
  LATTE_HIP(hipMalloc((void**)&wt, (size_t)27 * 128 * 4));
  int rc = launch_pack_small_w(w, wt, 128, 3, 1, st);
  if (!rc) rc = launch_enc_conv_in(x, in_mode, wt, bias, out, N, H, W, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(wt);
  return rc;
}

int latte_debug_vae_enc_tail(const void* x, const void* x_lo, const float* w, const float* b, const float* qw, const float* qb, float* moments,
                             int N, int H, int W, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  constexpr int C = 512;
  float *raw = nullptr, *wf = nullptr, *bf = nullptr;
  LATTE_HIP(hipMalloc((void**)&raw, (size_t)8 * 9 * C * 4));
  LATTE_HIP(hipMalloc((void**)&wf, (size_t)8 * 9 * C * 4));
  LATTE_HIP(hipMalloc((void**)&bf, 64));
  int rc = launch_pack_small_w(w, raw, 8, C, 0, st);
  if (!rc) rc = launch_fold_quant_conv(raw, b, qw, qb, wf, bf, 9 * C, st);
  if (!rc) rc = launch_enc_conv_out((const half_t*)x, (const half_t*)x_lo, wf, bf, moments, N, H, W, C, LATTE_DTYPE_F16, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(raw);
  (void)hipFree(wf);
  (void)hipFree(bf);
  return rc;
}

int latte_debug_groupnorm_f32(const float* x, void* y, const float* gamma, const float* beta, int N, int HW, int C, int silu,
                              int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  float *partial = nullptr, *stats = nullptr;
  LATTE_HIP(hipMalloc((void**)&partial, (size_t)N * groupnorm_max_slabs() * 64 * 4));
  LATTE_HIP(hipMalloc((void**)&stats, (size_t)N * 64 * 4));
  int rc = launch_groupnorm(x, 1, (half_t*)y, gamma, beta, partial, stats, N, HW, C, silu, dtype, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(partial);
  (void)hipFree(stats);
  return rc;
}

int latte_debug_groupnorm(const void* x, void* y, const float* gamma, const float* beta, int N, int HW, int C, int silu,
                          int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  float *partial = nullptr, *stats = nullptr;
  LATTE_HIP(hipMalloc((void**)&partial, (size_t)N * groupnorm_max_slabs() * 64 * 4));
  LATTE_HIP(hipMalloc((void**)&stats, (size_t)N * 64 * 4));
  int rc = launch_groupnorm(x, 0, (half_t*)y, gamma, beta, partial, stats, N, HW, C, silu, dtype, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(partial);
  (void)hipFree(stats);
  return rc;
}

// ---- the VAE's GroupNorm with its defaulted arguments, and the small kernels of csrc/vae.hip: argument checks + the engines' own
// launchers, unchanged (f16 half buffers throughout: the VAE launchers refuse bf16)
int latte_debug_groupnorm_ex(const void* x, int x_is_f32, void* y, void* y_lo_or_null, const float* gamma, const float* beta, int N, int HW,
                             int C, int silu, float eps, int max_slabs, float* stats_out_or_null, int dtype, void* stream) {
  if (!x || !y || !gamma || !beta || N < 1 || HW < 1 || bad_mode(x_is_f32) || bad_mode(silu) || !(eps > 0.0f) || misaligned(x, 16) ||
      misaligned(y, 16) || misaligned(y_lo_or_null, 16) || misaligned(gamma, 16) || misaligned(beta, 16) || (int64_t)N * HW > 0x7fffffff)
    return fail(LATTE_ERR_INVALID, "groupnorm_ex: bad arguments (x_is_f32 and silu 0 or 1, eps > 0, 16-byte aligned buffers)");
  if (C != 128 && C != 256 && C != 512) return fail(LATTE_ERR_INVALID, "groupnorm_ex: C must be 128, 256 or 512");
  if (dtype != LATTE_DTYPE_F16) return fail(LATTE_ERR_INVALID, "groupnorm_ex: the VAE kernels are built for f16 operands only");
  if (max_slabs < 1) return fail(LATTE_ERR_INVALID, "groupnorm_ex: max_slabs must be at least 1");
  if (max_slabs > groupnorm_max_slabs() * 64 || (max_slabs > groupnorm_max_slabs() && N != 1))
    return fail(LATTE_ERR_INVALID, "groupnorm_ex: max_slabs beyond groupnorm_max_slabs() is the one-sample form (N == 1), at most 64 times it");
  hipStream_t st = (hipStream_t)stream;
  float *partial = nullptr, *stats = nullptr;
  LATTE_HIP(hipMalloc((void**)&partial, (size_t)N * max_slabs * 64 * 4));
  LATTE_HIP(hipMalloc((void**)&stats, (size_t)N * 64 * 4));
  int rc = launch_groupnorm(x, x_is_f32, (half_t*)y, gamma, beta, partial, stats, N, HW, C, silu, dtype, st, eps, max_slabs, (half_t*)y_lo_or_null);
  if (!rc && stats_out_or_null &&
      hipMemcpyAsync(stats_out_or_null, stats, (size_t)N * 64 * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
    rc = fail(LATTE_ERR_HIP, "groupnorm_ex: statistics copy failed");
  (void)hipStreamSynchronize(st);
  (void)hipFree(partial);
  (void)hipFree(stats);
  return rc;
}

int latte_debug_vae_post_quant(const float* z, const float* w, const float* b, float* out, int N, int hw, float z_scale, void* stream) {
  if (!z || !w || !b || !out || N < 1 || hw < 1 || (int64_t)N * hw > 0x7fffffff / 4 || misaligned(out, 16))
    return fail(LATTE_ERR_INVALID, "vae_post_quant: bad arguments (out 16-byte aligned)");
  return launch_post_quant(z, w, b, out, N, hw, z_scale, (hipStream_t)stream);
}

int latte_debug_vae_conv_in(const float* x, const float* w, const float* bias, float* out, int N, int H, int W, int Cout, void* stream) {
  if (!x || !w || !bias || !out || N < 1 || H < 1 || W < 1 || (int64_t)N * H * W > 0x7fffffff || misaligned(out, 8))
    return fail(LATTE_ERR_INVALID, "vae_conv_in: bad arguments");
  if (Cout < 2 || Cout % 2) return fail(LATTE_ERR_INVALID, "vae_conv_in: Cout must be even and at least 2");
  hipStream_t st = (hipStream_t)stream;
  float* wt = nullptr;
  LATTE_HIP(hipMalloc((void**)&wt, (size_t)36 * Cout * 4));
  int rc = launch_pack_small_w(w, wt, Cout, 4, 1, st);
  if (!rc) rc = launch_conv_in(x, wt, bias, out, N, H, W, Cout, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(wt);
  return rc;
}

int latte_debug_vae_conv_out(const void* x, const void* x_lo_or_null, const float* w, const float* bias, void* out, int N, int H, int W, int C,
                             int out_mode, void* stream) {
  if (!x || !w || !bias || !out || N < 1 || H < 1 || W < 1 || (int64_t)N * H * W > 0x7fffffff / 3 || misaligned(x, 16) ||
      misaligned(x_lo_or_null, 16))
    return fail(LATTE_ERR_INVALID, "vae_conv_out: bad arguments (x and x_lo 16-byte aligned)");
  if (C < 8 || C % 8) return fail(LATTE_ERR_INVALID, "vae_conv_out: C must be a positive multiple of 8");
  if ((int64_t)27 * C * (int64_t)sizeof(float) > 65536)
    return fail(LATTE_ERR_INVALID, "vae_conv_out: 27 C floats of weights exceed the default dynamic LDS limit (64 KiB)");
  if (bad_mode(out_mode)) return fail(LATTE_ERR_INVALID, "vae_conv_out: out_mode must be 0 (fp32 NCHW) or 1 (uint8 NHWC)");
  hipStream_t st = (hipStream_t)stream;
  float* wt = nullptr;
  LATTE_HIP(hipMalloc((void**)&wt, (size_t)27 * C * 4));
  int rc = launch_pack_small_w(w, wt, 3, C, 0, st);
  if (!rc) rc = launch_conv_out((const half_t*)x, wt, bias, out, N, H, W, C, out_mode, LATTE_DTYPE_F16, st, (const half_t*)x_lo_or_null);
  (void)hipStreamSynchronize(st);
  (void)hipFree(wt);
  return rc;
}

int latte_debug_vae_softmax_rows(const float* s, void* p, int rows, int L, float scale, void* stream) {
  if (!s || !p || rows < 1) return fail(LATTE_ERR_INVALID, "vae_softmax_rows: bad arguments");
  if (L < 64 || L % 64 || L > 4096) return fail(LATTE_ERR_INVALID, "vae_softmax_rows: need L % 64 == 0 and 64 <= L <= 4096");
  return launch_softmax_rows(s, (half_t*)p, rows, L, scale, LATTE_DTYPE_F16, (hipStream_t)stream);
}

int latte_debug_vae_time_conv_out(const float* in, const float* w, const float* bias, void* out, int T, int HW, int out_mode, void* stream) {
  if (!in || !w || !bias || !out || T < 1 || HW < 1) return fail(LATTE_ERR_INVALID, "vae_time_conv_out: bad arguments");
  if (bad_mode(out_mode)) return fail(LATTE_ERR_INVALID, "vae_time_conv_out: out_mode must be 0 (fp32 NCHW) or 1 (uint8 NHWC)");
  return launch_time_conv_out(in, w, bias, out, T, HW, out_mode, (hipStream_t)stream);
}

int latte_debug_vae_pack_conv_t(const float* w, const float* mix_or_null, void* out, void* out_lo_or_null, int Cout, int Cin, void* stream) {
  if (!w || !out || Cout < 1 || Cin < 1) return fail(LATTE_ERR_INVALID, "vae_pack_conv_t: bad arguments");
  return launch_pack_conv_t(w, (half_t*)out, Cout, Cin, mix_or_null, LATTE_DTYPE_F16, (hipStream_t)stream, (half_t*)out_lo_or_null);
}

int latte_debug_vae_scale_by_sigmoid(const float* in, float* out, int n, const float* mix, void* stream) {
  if (!in || !out || !mix || n < 1) return fail(LATTE_ERR_INVALID, "vae_scale_by_sigmoid: bad arguments");
  return launch_scale_by_sigmoid(in, out, n, mix, (hipStream_t)stream);
}

int latte_debug_vae_pack_conv_w(const float* w, void* out, void* out_lo_or_null, int Cout, int Cin, void* stream) {
  if (!w || !out || Cout < 1 || Cin < 1) return fail(LATTE_ERR_INVALID, "vae_pack_conv_w: bad arguments");
  return launch_pack_conv_w(w, (half_t*)out, Cout, Cin, LATTE_DTYPE_F16, (hipStream_t)stream, (half_t*)out_lo_or_null);
}

int latte_debug_convert_split(const float* in, void* out, void* out_lo, int64_t n, void* stream) {
  if (!in || !out || !out_lo || n < 1) return fail(LATTE_ERR_INVALID, "convert_split: bad arguments");
  return launch_convert_f32_to_h16_split(in, (half_t*)out, (half_t*)out_lo, n, LATTE_DTYPE_F16, (hipStream_t)stream);
}

int latte_debug_set_choice(const char* name, int value) {
  if (set_debug_choice(name, value) != 0)
    return fail(LATTE_ERR_INVALID, std::string("latte_debug_set_choice: unknown name or value not offered by this build: ") + (name ? name : "(null)"));
  return LATTE_OK;
}

int latte_debug_tr16_probe(uint16_t* out, void* stream) {
  hipLaunchKernelGGL(tr16_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out);
  LATTE_HIP(hipGetLastError());
  return LATTE_OK;
}

}  // extern "C"
