// The transformer block of the denoisers (latte.py:163-181; latte_t2v.py BasicTransformerBlock_), once: LN-modulate, fused QKV + attention
// (or qkv GEMM + attention), gated out-projection | LN-modulate, fc1, gated fc2.  engine.cpp and t2v_engine.cpp own their block loops
// and what lies around the block (conditioning, patch embed, cross-attention, head); a forward fills one BlockCtx and calls
// block_attention / block_mlp per block.
#pragma once
#include "event_profile.h"
#include "weight_store.h"

namespace latte {

// kernel classes of latte_profile_forward (the Python profile tables index by these values)
enum { C_QKV = 0, C_PROJ, C_FC1, C_FC2, C_ATTN_S, C_ATTN_T, C_LN, C_COND, C_PATCH, C_FINAL, C_QKVATTN_S, C_QKVATTN_T, C_NONE = -1 };
struct Timer {  // optional per-launch HIP events (latte_profile_forward)
  EventProfile* p;
  hipStream_t st;
  void mark(int cls) {
    if (p) p->mark(cls, st);
  }
};

struct BlockLinears {
  half_t *qkv_w, *proj_w, *fc1_w, *fc2_w;
  float *qkv_b, *proj_b, *fc1_b, *fc2_b;
  half_t *proj_w2 = nullptr, *fc1_w2 = nullptr;   // [N, 2 K] = [W | W]: the weight of a split-operand linear (guided_split bits 0 / 1), built lazily
  unsigned char *fc1_w4 = nullptr, *fc1_w4s = nullptr;    // fp4 image of fc1's weight + its row scales (guided_split bit 4; GemmArgs::W4 / W4s)
  unsigned char *proj_w8 = nullptr, *fc1_w8 = nullptr;   // [N, K] e4m3(W 2^LO8_W_SHIFT): the weight of a GEMM's fp8 correction pass (bits 2 / 3)
};
// the four weights and four biases (zero-filled); the derived copies stay with the engine that uses them
int alloc_block_linears(DeviceArena& arena, BlockLinears& w, int D, int Hm);

constexpr int64_t SPLIT_WS_FLOATS = 256ll * 256 * 192;   // BlockCtx::split_ws: s * tiles <= 256 tiles of 256 x 192

// What one forward fixes for all of its blocks
struct BlockCtx {
  int B, F, T, D, heads, hd, Hm, dt;
  float* xres;                // fp32 residual stream [B F T, D]
  half_t *xn, *qkv, *hbuf;    // [rows, D], [rows, 3 D], [rows, Hm]
  int mod_stride;             // row stride of the modulation rows (0 = one row shared by every sample)
  const float* temp;          // temp_embed [F, D], added once behind block 0; nullptr = never
  bool te_in_fc2;             // block 0's fc2 epilogue adds it (block_fc2_takes_te), else block 1's first LayerNorm pass
  int fuse_qkv_attn;          // bit 0 spatial / bit 1 temporal blocks fused where the shape allows; bits 2-4: QkvAttnArgs::flags off
  int gemm_variant_of[4];     // qkv, proj, fc1, fc2: the tile variant launch_gemm gets (0 = per-shape choice)
  int gated_split_k;          // 0 = rule of gated_split_choice, 1 = never split, 2..4 = force
  int rmw_mode;               // GemmArgs::rmw_mode of the two gated GEMMs
  int stream_policy;          // StreamPolicy bits of this forward
  float *split_ws, *zero_bias;   // split-K workspace (SPLIT_WS_FLOATS) and a zero bias row; nullptr = never split
  int gsplit;                 // resolved guided_split bits (engine.cpp: run_forward), with their operand buffers:
  half_t* xn2;                // [rows, 2 D]
  unsigned char *lo8, *lo4, *lo4s;
  int guided_split_active;    // out: the bits some block really ran are OR-ed in
  EventProfile* prof;         // may be nullptr
};

// the shape of fc2 runs on the rolling 12-wave kernel, whose epilogue can add temp_embed (needs everything but temp / te_in_fc2 filled)
bool block_fc2_takes_te(const BlockCtx& c);
// Block i (even = spatial, odd = temporal); mb: its six modulation rows shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp.
// block_attention: LN-modulate ... gated out-projection; block_mlp: LN-modulate ... gated fc2.
int block_attention(BlockCtx& c, const BlockLinears& w, int i, const float* mb, hipStream_t st);
int block_mlp(BlockCtx& c, const BlockLinears& w, int i, const float* mb, hipStream_t st);

}  // namespace latte
