// The one body of the denoiser block (block.h).  Host code only: every launch goes through the launchers of common.h.
#include <cmath>

#include "block.h"

namespace latte {

namespace {

// Gated read-modify-write GEMM x += gate * (A W^T + bias) (attention out-projection, fc2; latte.py:179-180).  At small batches
// its 256 x 192 output tiles fill a fraction of the 256 CUs (B = 1 at XL/2: 96 tiles, fc2 78 us per launch against 33 us at the
// B = 8 rate): when at least two splits of a DEEP contraction fit on the chip, the GEMM runs as `s` partial products (tile
// variant 5, grid.y = s, fp32 slabs in split_ws) and gated_split_reduce adds them to the residual stream in slab order.
// Measured inside the XL/2 forward at B = 1 (same box): fc2 (K = 4608) 77.6 -> 68.2 us including the reduction, the out-projection
// (K = 1152) 30.6 -> 39.0 us -- the reduction pass costs more than half of a 18-K-tile GEMM, hence the >= 32 K tiles per split.
// (A stream-K decomposition of the 12-wave kernel with in-launch hand-over of the partial products was built and measured
// slower than this at every small-batch shape: DESIGN.md section 8.)
int gated_split_choice(const BlockCtx& e, int M, int N, int K, int variant) {
  if (!e.split_ws || variant != 0 || e.gated_split_k == 1 || N % 192 || K % 64) return 1;
  if (e.gated_split_k == 0 && gemm_small_tile_ok(M, N, K)) return 1;   // one 128 x 144 tile per CU beats the split (launch_gemm)
  const int tiles = ((M + 255) / 256) * (N / 192), nk = K / 64;
  if (e.gated_split_k >= 2) {
    const int s = e.gated_split_k;
    return (nk % s == 0 && (int64_t)s * M * N <= SPLIT_WS_FLOATS) ? s : 1;
  }
  for (int s = 4; s >= 2; --s)
    if (tiles * s <= 256 && nk % s == 0 && nk / s >= 32 && (int64_t)s * M * N <= SPLIT_WS_FLOATS) return s;
  return 1;
}
// the gated GEMM of this shape runs on the rolling 12-wave kernel, whose epilogue can add the temporal embedding (GemmArgs::te)
bool gated_gemm_takes_te(const BlockCtx& e, int M, int N, int K, int variant) {
  if (gated_split_choice(e, M, N, K, variant) != 1) return false;
  return (variant ? variant : gemm_resolve_variant(M, N, K, EPI_GATE_RES_F32)) == 11;
}
int gated_gemm(const BlockCtx& e, const GemmArgs& g, int variant, hipStream_t st) {
  if (g.A8) return launch_gemm(g, EPI_GATE_RES_F32, e.dt, 0, st);   // fp8 correction pass: the rolling 12-wave kernel carries it
  const int s = gated_split_choice(e, g.M, g.N, g.K, variant);
  if (s == 1) return launch_gemm(g, EPI_GATE_RES_F32, e.dt, variant, st);
  GemmArgs p = g;
  p.bias = e.zero_bias;
  p.gate = nullptr;
  p.out = e.split_ws;
  p.k_chunk = g.K / s;
  p.split_stride = (long)g.M * g.N;
  if (int rc = launch_gemm(p, EPI_BIAS_F32, e.dt, 5, st)) return rc;
  return launch_gated_split_reduce((float*)g.out, e.split_ws, s, (size_t)g.M * g.N, g.bias, g.gate, g.gate_stride,
                                   g.rows_per_sample, g.M, g.N, st);
}

// what every GEMM of a block starts from
GemmArgs block_gemm(const BlockCtx& c) {
  GemmArgs g{};
  g.M = c.B * c.F * c.T; g.rows_per_sample = c.F * c.T; g.gate_stride = c.mod_stride; g.rmw_mode = c.rmw_mode; g.stream_policy = c.stream_policy;
  return g;
}

}  // namespace

int alloc_block_linears(DeviceArena& arena, BlockLinears& w, int D, int Hm) {
  int rc;
  if ((rc = arena.alloc(&w.qkv_w, (size_t)3 * D * D)) || (rc = arena.alloc(&w.proj_w, (size_t)D * D)) ||
      (rc = arena.alloc(&w.fc1_w, (size_t)Hm * D)) || (rc = arena.alloc(&w.fc2_w, (size_t)D * Hm)) ||
      (rc = arena.alloc(&w.qkv_b, (size_t)3 * D)) || (rc = arena.alloc(&w.proj_b, (size_t)D)) ||
      (rc = arena.alloc(&w.fc1_b, (size_t)Hm)) || (rc = arena.alloc(&w.fc2_b, (size_t)D))) return rc;
  return LATTE_OK;
}

bool block_fc2_takes_te(const BlockCtx& c) { return gated_gemm_takes_te(c, c.B * c.F * c.T, c.D, c.Hm, c.gemm_variant_of[3]); }

int block_attention(BlockCtx& c, const BlockLinears& w, int i, const float* mb, hipStream_t st) {
  const bool spatial = (i % 2) == 0;  // latte.py:345-346
  const int B = c.B, F = c.F, T = c.T, D = c.D, dt = c.dt, gsplit = c.gsplit;
  const int M = B * F * T, rps = F * T;
  Timer tm{c.prof, st};
  int rc;
  bool split_proj = false;   // this block's attention output leaves the fused kernel as a split pair
  // x + temp_embed once, after the first spatial block (latte.py:357-358): in that block's fc2 epilogue where fc2 runs on the
  // rolling 12-wave kernel (every element of x is in a register there), else in this LayerNorm pass, which then rewrites x
  const float* te = (i == 1 && !c.te_in_fc2) ? c.temp : nullptr;
  if ((rc = launch_ln_modulate(c.xres, c.xres, c.xn, mb, mb + D, c.mod_stride, M, D, rps, te, T, F, dt, st))) return rc;
  tm.mark(C_LN);
  GemmArgs g = block_gemm(c);
  const half_t* attn_out = c.xn;
  const float attn_scale = 1.0f / std::sqrt((float)c.hd);
  if (((c.fuse_qkv_attn >> (spatial ? 0 : 1)) & 1) && qkv_attention_fusable(D, c.heads, c.hd, F, T, spatial ? 0 : 1, M)) {
    // qkv projection + attention core in one kernel (q / k / v of a head only in LDS); the output goes to the (otherwise idle)
    // qkv buffer viewed as [rows, D], because xn is still being read by other units of the same launch
    QkvAttnArgs qa{};
    qa.xn = c.xn; qa.w = w.qkv_w; qa.bias = w.qkv_b; qa.out = c.qkv; qa.B = B; qa.F = F; qa.T = T; qa.D = D;
    qa.heads = c.heads; qa.hd = c.hd; qa.mode = spatial ? 0 : 1; qa.scale = attn_scale;
    qa.flags = ((c.fuse_qkv_attn >> 2) & 7) ^ 7;   // option bits 2-4 switch the default schedule features OFF (A/B hook)
    split_proj = gsplit & 5;
    qa.out_split = (gsplit & 4) ? 2 : (gsplit & 1);   // 1: [rows, 2 D] = [hi | lo] inside the [rows, 3 D] qkv buffer; 2: + fp8 remainder
    qa.out8 = c.lo8;
    qa.stream_policy = c.stream_policy;
    c.guided_split_active |= gsplit & 5;
    if ((rc = launch_qkv_attention(qa, dt, st))) return rc;
    tm.mark(spatial ? C_QKVATTN_S : C_QKVATTN_T);
    attn_out = c.qkv;
  } else {
    g.A = c.xn; g.W = w.qkv_w; g.bias = w.qkv_b; g.out = c.qkv; g.N = 3 * D; g.K = D;
    if ((rc = launch_gemm(g, EPI_BIAS_H16, dt, c.gemm_variant_of[0], st))) return rc;
    tm.mark(C_QKV);
    AttnArgs a{};
    a.qkv = c.qkv; a.out = c.xn; a.heads = c.heads; a.hd = c.hd; a.D = D;
    a.sample_stride = rps; a.scale = attn_scale;
    seq_layout(a, spatial, B, F, T);
    if (gsplit & 4) {   // the un-fused attention kernels carry the fp8 remainder too (round 6); the f16-pair form (bit 0) exists in the fused kernel only
      a.out8 = c.lo8;
      split_proj = true;
      c.guided_split_active |= 4;
    }
    if ((rc = launch_attention(a, dt, st))) return rc;
    tm.mark(spatial ? C_ATTN_S : C_ATTN_T);
  }
  g.A = attn_out; g.W = w.proj_w; g.bias = w.proj_b; g.out = c.xres; g.gate = mb + 2 * D; g.N = D; g.K = D; g.tag = 0;
  if (split_proj && (gsplit & 4)) { g.A8 = c.lo8; g.W8 = w.proj_w8; }          // o_hi . W^T + o_lo8 . W8^T in one launch
  else if (split_proj) { g.W = w.proj_w2; g.K = 2 * D; }                          // [o_hi | o_lo] . [W | W]^T
  if ((rc = gated_gemm(c, g, c.gemm_variant_of[1], st))) return rc;
  tm.mark(C_PROJ);
  return LATTE_OK;
}

int block_mlp(BlockCtx& c, const BlockLinears& w, int i, const float* mb, hipStream_t st) {
  const int F = c.F, T = c.T, D = c.D, dt = c.dt, gsplit = c.gsplit;
  const int M = c.B * F * T, rps = F * T;
  Timer tm{c.prof, st};
  int rc;
  const int split_fc1 = (gsplit & 16) ? 3 : (gsplit & 8) ? 2 : (gsplit & 2) ? 1 : 0;
  if (split_fc1 == 3) rc = launch_ln_modulate_split4(c.xres, c.xn, c.lo4, c.lo4s, mb + 3 * D, mb + 4 * D, c.mod_stride, M, D, rps, dt, st);
  else rc = launch_ln_modulate(c.xres, c.xres, split_fc1 == 1 ? c.xn2 : c.xn, mb + 3 * D, mb + 4 * D, c.mod_stride, M, D, rps, nullptr, T, F, dt, st,
                               split_fc1, c.lo8);
  if (rc) return rc;
  tm.mark(C_LN);
  GemmArgs g = block_gemm(c);
  g.A = c.xn; g.W = w.fc1_w; g.bias = w.fc1_b; g.out = c.hbuf; g.N = c.Hm; g.K = D;
  if (split_fc1 == 1) { g.A = c.xn2; g.W = w.fc1_w2; g.K = 2 * D; }
  if (split_fc1 == 2) { g.A8 = c.lo8; g.W8 = w.fc1_w8; }
  if (split_fc1 == 3) { g.A4 = c.lo4; g.A4s = c.lo4s; g.W4 = w.fc1_w4; g.W4s = w.fc1_w4s; }
  if ((rc = launch_gemm(g, EPI_BIAS_GELU_H16, dt, c.gemm_variant_of[2], st))) return rc;
  tm.mark(C_FC1);
  g = block_gemm(c);
  g.A = c.hbuf; g.W = w.fc2_w; g.bias = w.fc2_b; g.out = c.xres; g.gate = mb + 5 * D; g.N = D; g.K = c.Hm; g.tag = 1;
  if (i == 0 && c.te_in_fc2) { g.te = c.temp; g.te_T = T; g.te_F = F; }
  if ((rc = gated_gemm(c, g, c.gemm_variant_of[3], st))) return rc;
  tm.mark(C_FC2);
  return LATTE_OK;
}

}  // namespace latte
