// Producer-wave GEMM (round 2):  C[M,N] = A[M,K] · W[N,K]^T, 256 x 192 tile, TWELVE waves per workgroup.
//
// Same operand layout, LDS image (source-side swizzle), persistent XCD-chunked tile walk and segment schedule as
// gemm_pps_kernel (gemm.hip), with ONE change of structure: the operand DMA is not issued by the MFMA waves.
// What round 1 measured: a `buffer_load ... lds` holds the wave that issues it for 26-105 shader
// clocks, so in the 8-wave kernel every K tile serialises [64 MFMAs | 12 DMA issues | 24 fragment reads] inside group 0's
// waves and the matrix pipe idles for a third of the period; a DMA wave NEXT TO MFMA waves does not slow them at all
// (`latte_debug_dma_probe` modes 7-9: 16.4 clocks per MFMA beside 4 streaming DMA waves).  So:
//   * waves 0-7  = consumers, 2 groups x 4 (output rows 0-127 / 128-255, 48 columns each): fragment reads + MFMAs + epilogue;
//   * waves 8-11 = producers, one per SIMD (a workgroup's waves are placed on the SIMDs cyclically, so waves w, w + 4, w + 8
//     share one): they only issue the LDS DMA of K tile u + 1 while the consumers work on K tile u, confirm it with counted
//     `vmcnt` and take part in the workgroup barriers.
// Three waves per SIMD means 168 VGPRs per wave (512 / 3, one allocation for the whole kernel), which is why the tile is
// 256 x 192 (96 accumulators) and the fragments of the second half of a K tile are read INSIDE the compute segment, each
// A fragment into the registers its first-half twin has just left: 96 + 24 (B, both halves) + 32 (A) = 152.
//
// Barrier-delimited intervals (barrier b ends interval I(b); P = the barrier after the pipeline fill):
//   group 0:   L(u) in I(2u),   C(u) in I(2u+1)          L(u): B(u) both halves + A(u) first half  -> registers
//   group 1:   L(u) in I(2u+1), C(u) in I(2u+2)          C(u): 48 MFMAs, the 8 second-half A reads between them
//   producers (LDS rings: THREE A stages, two B stages -- with two A stages the producers of the K = 4608 GEMM waited 745 clocks
//   per K tile for an A operand that comes from HBM / the Infinity Cache with one K tile of look-ahead):
//              I(2v)   issue B(v+1) and A rows 0-127 of K tile v+2, then vmcnt(18): everything of K tile v has landed;
//              I(2v+1) issue A rows 128-255 of K tile v+2, then vmcnt(8): B(v+1) (and the older A(v+1)) have landed.
// The K-tile counter runs across tile boundaries, so the producers never drain; a consumer group runs its epilogue
// around the barrier that ends its last compute segment (group 1 before, group 0 after it), as in gemm_pps_kernel.
#include <type_traits>

#include "common.h"
#include "mfma_util.h"

namespace latte {
namespace {

// In-place accumulate, pinned by inline assembly: with the fragments carried around the loop (rolling kernel) the register
// allocator otherwise moves accumulators into fragment registers that have just been freed and ends up spilling three of
// them per K tile.  The compiler's hazard recogniser does not look inside: no VALU / memory instruction may read an
// accumulator within 11 wait states of the MFMA that wrote it (the kernel issues two `s_nop 15` before its epilogue), and a
// fragment register is only ever overwritten by an LDS read, which has no hazard against an MFMA reading it as SrcA / SrcB.
template <int DT>
__device__ __forceinline__ void mfma16_ip(f32x4& c, const u32x4& a, const u32x4& b) {
  if constexpr (DT == LATTE_DTYPE_BF16)
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
  else
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}

// first product of an accumulator: C = 0 (inline constant) instead of a zeroed register set
template <int DT>
__device__ __forceinline__ void mfma16_first(f32x4& c, const u32x4& a, const u32x4& b) {
  if constexpr (DT == LATTE_DTYPE_BF16)
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=v"(c) : "v"(a), "v"(b));
  else
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=v"(c) : "v"(a), "v"(b));
}

// Correction pass of the rolling kernel (GemmArgs::A8 / W8): one block-scaled fp8 MFMA = K = 128 of the contraction, in place like
// mfma16_ip.  Operand maps established on the GPU against a CPU emulation by tools/mx_probe.hip (profiles/r6_mx_probe.log): lane l
// supplies row (l & 15) and the 32 consecutive bytes k = 32 (l >> 4) ... + 31 of its operand in 8 VGPRs, byte op_sel (0 here) of the
// lane's scale register is the E8M0 scale of those 32 elements, C / D as every 16 x 16 MFMA.  The kernel feeds it the two 16-byte
// fragment reads of the half-precision K loop (chunk (l >> 4) and chunk 4 + (l >> 4) of a 128-byte LDS row) as ONE 32-byte operand:
// both operands then hold the same 32 bytes-of-K per lane group, so the instruction contracts over a permutation of K -- the sum is
// the same.  16 passes: the accumulator must not be read by a VALU within 19 wait states (the epilogue's two s_nop 15 cover it).
typedef __attribute__((ext_vector_type(8))) unsigned int u32x8;
__device__ __forceinline__ u32x8 cat8(const u32x4& lo, const u32x4& hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); }
__device__ __forceinline__ void mfma8_ip(f32x4& c, const u32x8& a, const u32x8& b, unsigned sa, unsigned sb) {
  asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]" : "+v"(c) : "v"(a), "v"(b), "v"(sa), "v"(sb));
}

// `src` of lane l ^ 8 for the lanes of the 4-lane banks in BANKS (bit b = lanes 4 b ... 4 b + 3 of every row of 16), `old` elsewhere:
// a DPP rotation by 8 inside each row of 16 lanes.  (Written per scalar: with the element of a vector as the builtin's operand
// the compiler kept one exchange of four.)
template <int BANKS>
__device__ __forceinline__ float ror8(float old, float src) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), 0x128, 0xf, BANKS, false));
}

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

template <int EPI, int DT, int TAG>
__global__ void __launch_bounds__(768) gemm_pw_kernel(GemmArgs g) {
  constexpr int BM = 256, BN = 192, FN = 3, WTN = 48;
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128;
  constexpr int NA = 3;                         // LDS rings: 3 A stages (96 KB) at offset 0, 2 B stages (48 KB) behind them
  constexpr int B_BASE = NA * A_BYTES;
  constexpr int AH_INSTR = 4, BG_INSTR = 6;   // per producer wave: 128 A rows / (4 waves x 8 rows), 192 W rows / (4 x 8)
  constexpr int GROUP_M = 8;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int K = g.K;
  const unsigned row_bytes = (unsigned)K * 2u;

  // ---- this workgroup's tile sequence (identical to gemm_pps_kernel)
  const int tiles_m = (g.M + BM - 1) / BM, tiles_n = g.N / BN, nwg = tiles_m * tiles_n;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per = gridDim.x >> 3;
  const int q = nwg >> 3, r = nwg & 7;
  const int chunk0 = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  const int cnt = q + (xcd < r ? 1 : 0);
  if (slot >= cnt) return;
  const int group_m = g.group_m > 0 ? g.group_m : GROUP_M;
  auto decode = [&](int wg, int& tm, int& tn) {
    const int per_group = group_m * tiles_n;
    const int group = wg / per_group;
    const int first_m = group * group_m;
    const int gsz = min(tiles_m - first_m, group_m);
    const int in_group = wg - group * per_group;
    tm = first_m + in_group % gsz;
    tn = in_group / gsz;
  };
  const int nk = K / 64;
  const int ntile = (cnt - slot + per - 1) / per;   // tiles this workgroup walks
  if (wave >= 8) {
    // ================================ producer ================================
    const int pw = wave - 8;
    const __amdgpu_buffer_rsrc_t rsA =
        __builtin_amdgcn_make_buffer_rsrc((void*)g.A, 0, (unsigned)tiles_m * BM * row_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)g.W, 0, (unsigned)g.N * row_bytes, 0x00020000);
    const int lrow = lane >> 3, cpos = lane & 7;
    // row (lane >> 3) of an 8-row group, 16-byte chunk (lane & 7) ^ swizzle(row); rows pw*8 + 32 j: 32 j does not move the swizzle
    const unsigned voff = (unsigned)lrow * row_bytes + (unsigned)((cpos ^ (((pw * 8 + lrow) >> 1) & 7)) * 16);
    unsigned step32 = 32u * row_bytes;
    asm volatile("" : "+s"(step32));
    auto dma_a = [&](int half, int tm_, int kt, int stg) {
      char* sA = smem + stg * A_BYTES + half * 128 * 128 + pw * 1024;
      const unsigned so = (unsigned)(tm_ * BM + half * 128 + pw * 8) * row_bytes + (unsigned)kt * 128u;
#pragma unroll
      for (int j = 0; j < AH_INSTR; ++j) bload_lds16(rsA, sA + j * 4 * 1024, voff, so + (unsigned)j * step32);
    };
    auto dma_b = [&](int tn_, int kt, int stg) {
      char* sB = smem + B_BASE + stg * B_BYTES + pw * 1024;
      const unsigned so = (unsigned)(tn_ * BN + pw * 8) * row_bytes + (unsigned)kt * 128u;
#pragma unroll
      for (int j = 0; j < BG_INSTR; ++j) bload_lds16(rsB, sB + j * 4 * 1024, voff, so + (unsigned)j * step32);
    };
    // Two walkers over the K tiles of this workgroup's tile sequence: `b` (for B) is one K tile ahead of the consumers,
    // `a` (for A, the operand that streams from HBM in the long-K GEMMs) two.
    struct Walk { int pos, tm, tn, kt; };
    auto advance = [&](Walk& w) {
      if (++w.kt == nk) {
        w.kt = 0;
        w.pos += per;
        if (w.pos < cnt) decode(chunk0 + w.pos, w.tm, w.tn);
      }
    };
    Walk wb{slot, 0, 0, 0};
    decode(chunk0 + slot, wb.tm, wb.tn);
    Walk wa = wb;
    const int U = ntile * nk;
    // pipeline fill: K tile 0 complete, A of K tile 1
    dma_b(wb.tn, 0, 0);
    dma_a(0, wa.tm, 0, 0);
    dma_a(1, wa.tm, 0, 0);
    advance(wa);
    advance(wb);                       // wb -> K tile 1
    if (U > 1) { dma_a(0, wa.tm, wa.kt, 1); dma_a(1, wa.tm, wa.kt, 1); }
    advance(wa);                       // wa -> K tile 2
    if (U > 1) wait_vm<2 * AH_INSTR>(); else wait_vm<0>();
    __builtin_amdgcn_s_barrier();   // P
    int sa = 2, sb = 1;             // ring slots of K tile v + 2 (A) and v + 1 (B)
    for (int v = 0; v < U; ++v) {
      const bool more_b = v + 1 < U, more_a = v + 2 < U;
      // I(2v): B(v+1), A rows 0-127 of K tile v+2; then everything of K tile v must have landed
      if (more_b) dma_b(wb.tn, wb.kt, sb);
      if (more_a) dma_a(0, wa.tm, wa.kt, sa);
      // newer than K tile v: A(v+1) 8, B(v+1) 6, A0(v+2) 4
      if (more_a) wait_vm<2 * AH_INSTR + BG_INSTR + AH_INSTR>(); else wait_vm<0>();
      __builtin_amdgcn_s_barrier();
      // I(2v+1): A rows 128-255 of K tile v+2; then B(v+1) (and with it A(v+1), which is older) must have landed
      if (more_a) dma_a(1, wa.tm, wa.kt, sa);
      if (more_a) wait_vm<2 * AH_INSTR>(); else wait_vm<0>();
      __builtin_amdgcn_s_barrier();
      advance(wa);
      advance(wb);
      sa = sa == NA - 1 ? 0 : sa + 1;
      sb ^= 1;
    }
    __builtin_amdgcn_s_barrier();   // barrier 2U
    return;
  }

  // ================================ consumer ================================
  const int grp = wave >> 2, wn = wave & 3;
  const int sw = (lane >> 1) & 7;
  const int chunkb = ((lane >> 4) ^ sw) * 16;
  const int a_off = (grp * 128 + (lane & 15)) * 128 + chunkb;
  const int b_off = B_BASE + (wn * WTN + (lane & 15)) * 128 + chunkb;

  f32x4 acc[8][FN];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // Epilogue of tile (tm_, tn_) for this wave's 128 x 48 sub-tile, then clear the accumulators.
  auto epilogue = [&](int tm_, int tn_) {
    int le = lane;
    asm volatile("" : "+v"(le));   // opaque: keeps every lane-derived epilogue index out of the K loop's live set
    const int fr = le & 15;
    const int ncol = tn_ * BN + wn * WTN + (le >> 4) * 4;
    const int mbase = tm_ * BM + grp * 128 + fr;
    if constexpr (EPI == EPI_GATE_RES_F32) {
      // res[m, n] += gate[sample, n] * (acc + bias); residual loads run two fragments ahead of the stores (gemm.hip)
      if ((g.rows_per_sample % BM) == 0) {
        float* const outp = (float*)g.out;
        const float* gr = g.gate + (size_t)((tm_ * BM) / g.rows_per_sample) * g.gate_stride + ncol;
        float4 b4[FN], g1[FN];
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          b4[j] = *(const float4*)(g.bias + ncol + j * 16);
          g1[j] = *(const float4*)(gr + j * 16);
        }
        constexpr int NF = 8 * FN, AHEAD = 2;
        auto frag_ptr = [&](int f) -> float* {
          const int mc = min(mbase + (f / FN) * 16, g.M - 1);
          return outp + (size_t)mc * g.N + ncol + (f % FN) * 16;
        };
        float4 qa[AHEAD];
#pragma unroll
        for (int a = 0; a < AHEAD; ++a) qa[a] = *(const float4*)frag_ptr(a);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          float4 rr = qa[f % AHEAD];
          if (f + AHEAD < NF) qa[f % AHEAD] = *(const float4*)frag_ptr(f + AHEAD);
          asm volatile("" ::: "memory");
          const int i = f / FN, j = f % FN;
          rr.x += g1[j].x * (acc[i][j][0] + b4[j].x);
          rr.y += g1[j].y * (acc[i][j][1] + b4[j].y);
          rr.z += g1[j].z * (acc[i][j][2] + b4[j].z);
          rr.w += g1[j].w * (acc[i][j][3] + b4[j].w);
          if (mbase + i * 16 < g.M) *(float4*)(outp + (size_t)(mbase + i * 16) * g.N + ncol + j * 16) = rr;
          acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = mbase + i * 16;
      if (m < g.M) {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int n = ncol + j * 16;
          const float4 b4 = *(const float4*)(g.bias + n);
          float v0 = acc[i][j][0] + b4.x, v1 = acc[i][j][1] + b4.y, v2 = acc[i][j][2] + b4.z, v3 = acc[i][j][3] + b4.w;
          const size_t o = (size_t)m * g.N + n;
          if constexpr (EPI == EPI_GATE_RES_F32) {
            const float4 g4 = *(const float4*)(g.gate + (size_t)(m / g.rows_per_sample) * g.gate_stride + n);
            float4* dst = (float4*)((float*)g.out + o);
            float4 rr = *dst;
            rr.x += g4.x * v0; rr.y += g4.y * v1; rr.z += g4.z * v2; rr.w += g4.w * v3;
            *dst = rr;
          } else if constexpr (EPI == EPI_BIAS_F32) {
            *(float4*)((float*)g.out + o) = make_float4(v0, v1, v2, v3);
          } else {
            if constexpr (EPI == EPI_BIAS_GELU_H16) {
              auto gelu = [](float x) {
                const float p = __builtin_fmaf(x * x, -0.10294324f, -2.3022082f);
                return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(p * x));
              };
              v0 = gelu(v0); v1 = gelu(v1); v2 = gelu(v2); v3 = gelu(v3);
            }
            const u32x2 p = {pack2<DT>(v0, v1), pack2<DT>(v2, v3)};
            *(u32x2*)((half_t*)g.out + o) = p;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  };

  int pos = slot, tm, tn;
  decode(chunk0 + pos, tm, tn);
  __builtin_amdgcn_s_barrier();                 // P: K tile 0 has landed
  if (grp == 1) __builtin_amdgcn_s_barrier();   // barrier 0: group 1 runs one segment behind

  int it = 0, ia = 0;   // K-tile counter of the walk, its A ring slot (it % 3)
  for (;;) {
    for (int kt = 0; kt < nk; ++kt, ++it) {
      const bool last = kt + 1 == nk;
      const char* sbufA = smem + ia * A_BYTES;
      const char* sbufB = smem + (it & 1) * B_BYTES;
      ia = ia == NA - 1 ? 0 : ia + 1;
      u32x4 bf[2][FN], af[8];
      // ---- L(u)
#pragma unroll
      for (int j = 0; j < FN; ++j) bf[0][j] = *(const u32x4*)(sbufB + (b_off + j * 2048));
#pragma unroll
      for (int i = 0; i < 8; ++i) af[i] = *(const u32x4*)(sbufA + (a_off + i * 2048));
#pragma unroll
      for (int j = 0; j < FN; ++j) bf[1][j] = *(const u32x4*)(sbufB + ((b_off + j * 2048) ^ 64));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // ---- C(u)
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = mfma16<DT>(bf[0][j], af[i], acc[i][j]);
        // second-half fragment of the same rows into the registers the MFMAs above have just read
        af[i] = *(const u32x4*)(sbufA + ((a_off + i * 2048) ^ 64));
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = mfma16<DT>(bf[1][j], af[i], acc[i][j]);
      }
      __builtin_amdgcn_s_setprio(0);
      if (grp == 1 && last) epilogue(tm, tn);
      __builtin_amdgcn_s_barrier();
      if (grp == 0 && last) epilogue(tm, tn);
    }
    pos += per;
    if (pos >= cnt) break;
    decode(chunk0 + pos, tm, tn);
  }
  if (grp == 0) __builtin_amdgcn_s_barrier();   // barrier 2U (group 1 spent it up front)
}


// ------------------------------------------------------------------------------------------------
// Rolling variant (variant 11): the same 12-wave workgroup, but NO load segment at all.  The trace of variant 10 shows what is
// left once the MFMA waves stop issuing DMA: the two consumer groups still hand the matrix pipe to each other through two
// barriers per K tile (~190 clocks each, 20 % of the period) because a group's fragment reads sit in their own segment.  Here
// every consumer wave keeps its MFMA stream going and reads the fragments of the NEXT half K tile (32 deep) between the MFMAs
// of the current one, each A fragment into the registers the MFMAs just issued have left (B fragments are double-buffered:
// 24 registers) -- a software pipeline one half-step deep that costs no register beyond variant 10's 56.  Both groups run in
// lock step (two waves per SIMD share the matrix pipe; a read is consumed ~24 own MFMAs after it was issued), and ONE barrier
// per K tile -- placed 6 MFMAs into the second half-step, when every read of stage u has been issued long ago -- tells the
// producers that stage u may be overwritten and the consumers that stage u + 1 has landed.
//   consumer, K tile u:  h0: MFMAs on first-half fragments | second-half A fragments of u roll in
//                        h1: 6 MFMAs, lgkmcnt(0), barrier B_u, B first half of u+1, 18 MFMAs | first-half A fragments of u+1
//                            roll in (lagging two fragment rows), then B second half of u+1
//   producer:            ... vmcnt(8) [stage u+1 landed], barrier B_u, issue B(u+2) and A(u+3)      (3 A stages, 2 B stages)
// At a tile boundary the pipeline is drained (no look-ahead reads in the last half-step: the epilogue needs the registers)
// and refilled from stage u + 1 after the epilogue.
// LO (round 6): behind the K / 64 half-precision K tiles of an output tile the walk continues over K / 128 "virtual" K tiles of the
// fp8 correction operands A8 / W8 (GemmArgs) -- a 128-byte row piece of an fp8 operand is K = 128, so a correction K tile has the
// byte geometry, the LDS image, the swizzle and the DMA pieces of a half-precision one; the producers only switch descriptor and row
// pitch, the consumers run lo_tile() (24 MFMAs of 16 passes on the same fragment reads) instead of ktile() (48 of 8 passes).
// RS: access shape of the gated epilogue's residual traffic (GemmArgs::rmw_mode): 0 = one 16 x 16 fragment per instruction,
// 1 = the whole 128-byte line of the wave's span in 8-row instructions (see the epilogue).  TAG = 2: fc2 + temporal embedding.
// ANT (GemmArgs::stream_policy, SP_FC2_A / SP_PROJ_A by call site; LO == 0 only): the producers' A-operand DMA carries the `nt`
// hint -- A is a once-used activation stream, the weights keep the default policy (every XCD re-reads them every round).
template <int EPI, int DT, int TAG, int LO = 0, int RS = 0, int ANT = 0>
__global__ void __launch_bounds__(768) gemm_pwr_kernel(GemmArgs g) {
  constexpr int BM = 256, BN = 192, FN = 3, WTN = 48;
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128;
  constexpr int NA = 3;
  constexpr int B_BASE = NA * A_BYTES;
  constexpr int AH_INSTR = 4, BG_INSTR = 6;
  constexpr int GROUP_M = 8;
  constexpr int PATCH_BYTES = 16 * 112;   // wave-private epilogue patch (half-precision outputs): 16 rows, pitch 112 B

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int K = g.K;
  const unsigned row_bytes = (unsigned)K * 2u;

  const int tiles_m = (g.M + BM - 1) / BM, tiles_n = g.N / BN, nwg = tiles_m * tiles_n;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per = gridDim.x >> 3;
  const int q = nwg >> 3, r = nwg & 7;
  const int chunk0 = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  const int cnt = q + (xcd < r ? 1 : 0);
  if (slot >= cnt) return;
  const int group_m = g.group_m > 0 ? g.group_m : GROUP_M;
  auto decode = [&](int wg, int& tm, int& tn) {
    const int per_group = group_m * tiles_n;
    const int group = wg / per_group;
    const int first_m = group * group_m;
    const int gsz = min(tiles_m - first_m, group_m);
    const int in_group = wg - group * per_group;
    tm = first_m + in_group % gsz;
    tn = in_group / gsz;
  };
  const int nk = K / 64;
  const int nk8 = LO >= 2 ? (K + 255) / 256 : LO ? K / 128 : 0;   // correction K tiles behind the nk half-precision ones (fp4: K = 256 per 128 row bytes)
  const int nkt = nk + nk8;                       // K tiles of the walk per output tile
  const int ntile = (cnt - slot + per - 1) / per;
  if (wave >= 8) {
    // ================================ producer ================================
    const int pw = wave - 8;
    const __amdgpu_buffer_rsrc_t rsA =
        __builtin_amdgcn_make_buffer_rsrc((void*)g.A, 0, (unsigned)tiles_m * BM * row_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)g.W, 0, (unsigned)g.N * row_bytes, 0x00020000);
    const int lrow = lane >> 3, cpos = lane & 7;
    const unsigned voff = (unsigned)lrow * row_bytes + (unsigned)((cpos ^ (((pw * 8 + lrow) >> 1) & 7)) * 16);
    unsigned step32 = 32u * row_bytes;
    asm volatile("" : "+s"(step32));
    // correction operands: rows of K bytes
    const unsigned row_bytes8 = LO >= 2 ? (unsigned)((K + 255) / 256 * 128) : (unsigned)K;   // fp4: two codes per byte, rows padded to K % 256 == 0
    const __amdgpu_buffer_rsrc_t rsA8 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(LO >= 2 ? (const void*)g.A4 : LO ? (const void*)g.A8 : (const void*)g.A), 0, (unsigned)tiles_m * BM * row_bytes8, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB8 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(LO >= 2 ? (const void*)g.W4 : LO ? (const void*)g.W8 : (const void*)g.W), 0, (unsigned)g.N * row_bytes8, 0x00020000);
    const unsigned voff8 = (unsigned)lrow * row_bytes8 + (unsigned)((cpos ^ (((pw * 8 + lrow) >> 1) & 7)) * 16);
    unsigned step32_8 = 32u * row_bytes8;
    asm volatile("" : "+s"(step32_8));
    auto dma_a = [&](int tm_, int kt, int stg) {   // all 256 rows: row-groups pw + 4 j, j = 0..7
      char* sA = smem + stg * A_BYTES + pw * 1024;
      if (LO && kt >= nk) {
        const unsigned so = (unsigned)(tm_ * BM + pw * 8) * row_bytes8 + (unsigned)(kt - nk) * 128u;
#pragma unroll
        for (int j = 0; j < 2 * AH_INSTR; ++j) bload_lds16(rsA8, sA + j * 4 * 1024, voff8, so + (unsigned)j * step32_8);
        return;
      }
      const unsigned so = (unsigned)(tm_ * BM + pw * 8) * row_bytes + (unsigned)kt * 128u;
#pragma unroll
      for (int j = 0; j < 2 * AH_INSTR; ++j) bload_lds16<ANT ? 2 : 0>(rsA, sA + j * 4 * 1024, voff, so + (unsigned)j * step32);
    };
    auto dma_b = [&](int tn_, int kt, int stg) {
      char* sB = smem + B_BASE + stg * B_BYTES + pw * 1024;
      if (LO && kt >= nk) {
        const unsigned so = (unsigned)(tn_ * BN + pw * 8) * row_bytes8 + (unsigned)(kt - nk) * 128u;
#pragma unroll
        for (int j = 0; j < BG_INSTR; ++j) bload_lds16(rsB8, sB + j * 4 * 1024, voff8, so + (unsigned)j * step32_8);
        return;
      }
      const unsigned so = (unsigned)(tn_ * BN + pw * 8) * row_bytes + (unsigned)kt * 128u;
#pragma unroll
      for (int j = 0; j < BG_INSTR; ++j) bload_lds16(rsB, sB + j * 4 * 1024, voff, so + (unsigned)j * step32);
    };
    struct Walk { int pos, tm, tn, kt; };
    auto advance = [&](Walk& w) {
      if (++w.kt == nkt) {
        w.kt = 0;
        w.pos += per;
        if (w.pos < cnt) decode(chunk0 + w.pos, w.tm, w.tn);
      }
    };
    const int U = ntile * nkt;
    Walk wb{slot, 0, 0, 0};
    decode(chunk0 + slot, wb.tm, wb.tn);
    Walk wa = wb;
    // pipeline fill, issue order  B0 A0 | B1 A1 | A2   (U >= 2: K >= 128)
    dma_b(wb.tn, wb.kt, 0); advance(wb);
    dma_a(wa.tm, wa.kt, 0); advance(wa);
    dma_b(wb.tn, wb.kt, 1); advance(wb);
    dma_a(wa.tm, wa.kt, 1); advance(wa);
    if (U > 2) { dma_a(wa.tm, wa.kt, 2); wait_vm<BG_INSTR + 4 * AH_INSTR>(); } else { wait_vm<BG_INSTR + 2 * AH_INSTR>(); }
    advance(wa);                    // wa -> K tile 3, wb -> K tile 2
    __builtin_amdgcn_s_barrier();   // P: K tile 0 has landed
    int sa = 0, sb = 0;             // ring slots of K tile u + 3 (A: (u + 3) % 3 = u % 3) and u + 2 (B: u & 1)
    for (int u = 0; u < U; ++u) {
      // stage u + 1 must have landed; the only younger DMA is A(u+2)
      if (u + 2 < U) wait_vm<2 * AH_INSTR>(); else wait_vm<0>();
      __builtin_amdgcn_s_barrier();   // B_u: stage u is free
      if (u + 2 < U) dma_b(wb.tn, wb.kt, sb);
      if (u + 3 < U) dma_a(wa.tm, wa.kt, sa);
      advance(wa);
      advance(wb);
      sa = sa == NA - 1 ? 0 : sa + 1;
      sb ^= 1;
    }
    return;
  }

  // ================================ consumer ================================
  const int grp = wave >> 2, wn = wave & 3;
  const int sw = (lane >> 1) & 7;
  const int chunkb = ((lane >> 4) ^ sw) * 16;
  const int a_off = (grp * 128 + (lane & 15)) * 128 + chunkb;
  const int b_off = B_BASE + (wn * WTN + (lane & 15)) * 128 + chunkb;

  f32x4 acc[8][FN];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto epilogue = [&](int tm_, int tn_) {
    int le = lane;
    asm volatile("" : "+v"(le));
    const int fr = le & 15;
    const int ncol = tn_ * BN + wn * WTN + (le >> 4) * 4;
    const int mbase = tm_ * BM + grp * 128 + fr;
    if constexpr (EPI == EPI_BIAS_H16 || EPI == EPI_BIAS_GELU_H16 || EPI == EPI_BIAS_GELU_DUAL_H16 || EPI == EPI_DGELU_H16) {
      // Half-precision outputs: a fragment row (16 rows x 48 columns = 96 B per row) goes through a wave-private LDS patch
      // (pitch 112 B, behind the operand rings) so that the global stores are 16 B per lane on contiguous 96-byte row
      // segments: 1.5 store instructions per fragment row instead of 3 with 8 B per lane on 32-byte pieces.
      // Training forms (round 6): EPI_BIAS_GELU_DUAL_H16 stores u and, through the same patch a second time, gelu(u) to g.aux;
      // EPI_DGELU_H16 multiplies by gelu'(u) with u read from g.aux (8 B per lane: the fragment's own elements).
      char* patch = smem + B_BASE + 2 * B_BYTES + wave * PATCH_BYTES;
      const int ncol0 = tn_ * BN + wn * WTN;
      const int gq = le >> 4;
      float4 b4[FN];
#pragma unroll
      for (int j = 0; j < FN; ++j) b4[j] = *(const float4*)(g.bias + ncol0 + j * 16 + gq * 4);
      const int r0 = le / 6, p0 = le - r0 * 6;               // piece le      -> (row, 16-byte piece) of the 16 x 6 grid
      const int r1 = (le + 64) / 6, p1 = (le + 64) - r1 * 6; // piece le + 64 (lanes 0-31)
      half_t* const outp = (half_t*)g.out;
      const int mrow0 = tm_ * BM + grp * 128;
      auto gelu = [](float x) {
        const float p = __builtin_fmaf(x * x, -0.10294324f, -2.3022082f);
        return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(p * x));
      };
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        u32x2 side[FN];   // DUAL: gelu(u) of this fragment row, DGELU: its u
        if constexpr (EPI == EPI_DGELU_H16) {
          const int mu = min(mrow0 + i * 16 + fr, g.M - 1);
#pragma unroll
          for (int j = 0; j < FN; ++j) side[j] = *(const u32x2*)(g.aux + (size_t)mu * g.N + ncol0 + j * 16 + gq * 4);
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          float v0 = acc[i][j][0] + b4[j].x, v1 = acc[i][j][1] + b4[j].y, v2 = acc[i][j][2] + b4[j].z, v3 = acc[i][j][3] + b4[j].w;
          if constexpr (EPI == EPI_BIAS_GELU_H16) {
            v0 = gelu(v0); v1 = gelu(v1); v2 = gelu(v2); v3 = gelu(v3);
          }
          if constexpr (EPI == EPI_DGELU_H16) {   // train.hip: gelu_kernel<BWD>, the same arithmetic on the unrounded product
            float x[4];
            unpack2<DT>(side[j][0], x[0], x[1]);
            unpack2<DT>(side[j][1], x[2], x[3]);
            auto dgelu = [](float xx) {
              const float p = __builtin_fmaf(xx * xx, -0.10294324f, -2.3022082f);
              const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(p * xx));
              const float du = 0.7978845608f * (1.0f + 0.134145f * xx * xx);
              return sg + xx * sg * (1.0f - sg) * 2.0f * du;
            };
            v0 *= dgelu(x[0]); v1 *= dgelu(x[1]); v2 *= dgelu(x[2]); v3 *= dgelu(x[3]);
          }
          const u32x2 pk = {pack2<DT>(v0, v1), pack2<DT>(v2, v3)};
          *(u32x2*)(patch + fr * 112 + j * 32 + gq * 8) = pk;
          if constexpr (EPI == EPI_BIAS_GELU_DUAL_H16) {   // the GELU of the ROUNDED pre-activation (what gelu_kernel<FWD> computes from u)
            float x[4];
            unpack2<DT>(pk[0], x[0], x[1]);
            unpack2<DT>(pk[1], x[2], x[3]);
            side[j] = (u32x2){pack2<DT>(gelu(x[0]), gelu(x[1])), pack2<DT>(gelu(x[2]), gelu(x[3]))};
          }
          acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        const int m0_ = mrow0 + i * 16 + r0, m1_ = mrow0 + i * 16 + r1;
        {
          const u32x4 w0 = *(const u32x4*)(patch + r0 * 112 + p0 * 16);
          if (m0_ < g.M) *(u32x4*)(outp + (size_t)m0_ * g.N + ncol0 + p0 * 8) = w0;
          if (le < 32) {
            const u32x4 w1 = *(const u32x4*)(patch + r1 * 112 + p1 * 16);
            if (m1_ < g.M) *(u32x4*)(outp + (size_t)m1_ * g.N + ncol0 + p1 * 8) = w1;
          }
        }
        if constexpr (EPI == EPI_BIAS_GELU_DUAL_H16) {   // second trip through the patch (LDS operations of a wave execute in order)
#pragma unroll
          for (int j = 0; j < FN; ++j) *(u32x2*)(patch + fr * 112 + j * 32 + gq * 8) = side[j];
          const u32x4 w0 = *(const u32x4*)(patch + r0 * 112 + p0 * 16);
          if (m0_ < g.M) *(u32x4*)(g.aux + (size_t)m0_ * g.N + ncol0 + p0 * 8) = w0;
          if (le < 32) {
            const u32x4 w1 = *(const u32x4*)(patch + r1 * 112 + p1 * 16);
            if (m1_ < g.M) *(u32x4*)(g.aux + (size_t)m1_ * g.N + ncol0 + p1 * 8) = w1;
          }
        }
      }
      return;
    }
    // TAG == 2: the temporal position embedding of row m's frame (GemmArgs::te), added BEHIND the gated update -- the two
    // fp32 operations of the former pair [this epilogue | x + temp_embed inside the next LayerNorm pass], in that order
    auto te_ptr = [&](int m_clamped, int n) -> const float* {
      return g.te + (size_t)((m_clamped / g.te_T) % g.te_F) * g.N + n;
    };
    // (TAG = 2 exists fragment-wise only: with the embedding's addresses the line-wise form spilled 24 B per lane; it is one launch per forward.)
    static_assert(!(TAG == 2 && RS == 1), "the temporal-embedding epilogue has the fragment-wise form only");
    if constexpr (EPI == EPI_GATE_RES_F32 && RS == 1) {
      // Line-wise residual accesses (GemmArgs::rmw_mode = 1; tools/rmw_shape_probe.hip, profiles/r7_rmw_shape_probe.log).  A wave's
      // 48 columns are 192 B of a row = one whole 128-byte line + half of a line shared with the neighbouring wave (the half comes
      // first in the odd waves).  The two fragments that make up the whole line swap halves between lanes l and l ^ 8 (one DPP
      // row rotation by 8 per register), after which lane (fr, gq) holds columns 16 (fr >> 3) + 4 gq ... + 3 of the line for the
      // rows (fr & 7) and 8 + (fr & 7) of the fragment row: two instructions of 8 rows x 128 B instead of two of 16 rows x 64 B.
      // The third fragment keeps the fragment-wise access.  Only acc + bias travels: every element is still
      // fma(gate, acc + bias, res) in fp32, so the bits are those of the fragment-wise form.
      if ((g.rows_per_sample % BM) == 0) {
        float* const outp = (float*)g.out;
        const bool odd = wn & 1;
        const int gq = le >> 4;
        const int n0 = tn_ * BN + wn * WTN;
        const int nline = n0 + (odd ? 16 : 0) + ((fr >> 3) * 4 + gq) * 4;
        const int nhalf = n0 + (odd ? 0 : 32) + gq * 4;
        const int mline = tm_ * BM + grp * 128 + (fr & 7);
        const float* gs = g.gate + (size_t)((tm_ * BM) / g.rows_per_sample) * g.gate_stride;
        const float4 gl = *(const float4*)(gs + nline), gh = *(const float4*)(gs + nhalf);
        float4 b4[FN];
#pragma unroll
        for (int j = 0; j < FN; ++j) b4[j] = *(const float4*)(g.bias + ncol + j * 16);
        constexpr int NQ = 8 * 3, AHEAD = 2;   // access q: fragment row q / 3; q % 3 = rows 0-7 | rows 8-15 of the line, the half line
        auto row_of = [&](int q) -> int { return (q % 3 == 2 ? mbase : mline + (q % 3) * 8) + (q / 3) * 16; };
        auto col_of = [&](int q) -> int { return q % 3 == 2 ? nhalf : nline; };
        float4 qa[AHEAD];
        auto load = [&](int q) {
          const int mc = min(row_of(q), g.M - 1);
          qa[q % AHEAD] = *(const float4*)(outp + (size_t)mc * g.N + col_of(q));
        };
#pragma unroll
        for (int a = 0; a < AHEAD; ++a) load(a);
        f32x4 t[3];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          float4 rr = qa[q % AHEAD];
          if (q + AHEAD < NQ) load(q + AHEAD);
          asm volatile("" ::: "memory");
          const int i = q / 3, k = q % 3;
          if (k == 0) {
            f32x4 s[FN];
#pragma unroll
            for (int j = 0; j < FN; ++j) {
              s[j] = (f32x4){acc[i][j][0] + b4[j].x, acc[i][j][1] + b4[j].y, acc[i][j][2] + b4[j].z, acc[i][j][3] + b4[j].w};
              acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            const f32x4 l0 = odd ? s[1] : s[0], l1 = odd ? s[2] : s[1];
            t[2] = odd ? s[0] : s[2];
            // lanes 8-15 of every 16 take the line's second fragment of lane - 8, lanes 0-7 its first fragment of lane + 8
            t[0] = (f32x4){ror8<0xC>(l0[0], l1[0]), ror8<0xC>(l0[1], l1[1]), ror8<0xC>(l0[2], l1[2]), ror8<0xC>(l0[3], l1[3])};
            t[1] = (f32x4){ror8<0x3>(l1[0], l0[0]), ror8<0x3>(l1[1], l0[1]), ror8<0x3>(l1[2], l0[2]), ror8<0x3>(l1[3], l0[3])};
          }
          const float4 gg = k == 2 ? gh : gl;
          rr.x = __builtin_fmaf(gg.x, t[k][0], rr.x);
          rr.y = __builtin_fmaf(gg.y, t[k][1], rr.y);
          rr.z = __builtin_fmaf(gg.z, t[k][2], rr.z);
          rr.w = __builtin_fmaf(gg.w, t[k][3], rr.w);
          if (row_of(q) < g.M) *(float4*)(outp + (size_t)row_of(q) * g.N + col_of(q)) = rr;
        }
        return;
      }
    }
    if constexpr (EPI == EPI_GATE_RES_F32 && RS == 0) {
      if ((g.rows_per_sample % BM) == 0) {
        float* const outp = (float*)g.out;
        const float* gr = g.gate + (size_t)((tm_ * BM) / g.rows_per_sample) * g.gate_stride + ncol;
        float4 b4[FN], g1[FN];
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          b4[j] = *(const float4*)(g.bias + ncol + j * 16);
          g1[j] = *(const float4*)(gr + j * 16);
        }
        constexpr int NF = 8 * FN, AHEAD = 2;
        auto frag_ptr = [&](int f) -> float* {
          const int mc = min(mbase + (f / FN) * 16, g.M - 1);
          return outp + (size_t)mc * g.N + ncol + (f % FN) * 16;
        };
        float4 qa[AHEAD], qe[AHEAD];
        auto load_te = [&](int f) {
          if constexpr (TAG == 2) qe[f % AHEAD] = *(const float4*)te_ptr(min(mbase + (f / FN) * 16, g.M - 1), ncol + (f % FN) * 16);
        };
#pragma unroll
        for (int a = 0; a < AHEAD; ++a) { qa[a] = *(const float4*)frag_ptr(a); load_te(a); }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          float4 rr = qa[f % AHEAD];
          float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
          if constexpr (TAG == 2) e4 = qe[f % AHEAD];
          if (f + AHEAD < NF) { qa[f % AHEAD] = *(const float4*)frag_ptr(f + AHEAD); load_te(f + AHEAD); }
          asm volatile("" ::: "memory");
          const int i = f / FN, j = f % FN;
          rr.x += g1[j].x * (acc[i][j][0] + b4[j].x);
          rr.y += g1[j].y * (acc[i][j][1] + b4[j].y);
          rr.z += g1[j].z * (acc[i][j][2] + b4[j].z);
          rr.w += g1[j].w * (acc[i][j][3] + b4[j].w);
          if constexpr (TAG == 2) { rr.x += e4.x; rr.y += e4.y; rr.z += e4.z; rr.w += e4.w; }
          if (mbase + i * 16 < g.M) *(float4*)(outp + (size_t)(mbase + i * 16) * g.N + ncol + j * 16) = rr;
          acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = mbase + i * 16;
      if (m < g.M) {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int n = ncol + j * 16;
          const float4 b4 = *(const float4*)(g.bias + n);
          float v0 = acc[i][j][0] + b4.x, v1 = acc[i][j][1] + b4.y, v2 = acc[i][j][2] + b4.z, v3 = acc[i][j][3] + b4.w;
          const size_t o = (size_t)m * g.N + n;
          if constexpr (EPI == EPI_GATE_RES_F32) {
            const float4 g4 = *(const float4*)(g.gate + (size_t)(m / g.rows_per_sample) * g.gate_stride + n);
            float4* dst = (float4*)((float*)g.out + o);
            float4 rr = *dst;
            rr.x += g4.x * v0; rr.y += g4.y * v1; rr.z += g4.z * v2; rr.w += g4.w * v3;
            if constexpr (TAG == 2) {
              const float4 e4 = *(const float4*)te_ptr(m, n);
              rr.x += e4.x; rr.y += e4.y; rr.z += e4.z; rr.w += e4.w;
            }
            *dst = rr;
          } else if constexpr (EPI == EPI_BIAS_F32) {
            *(float4*)((float*)g.out + o) = make_float4(v0, v1, v2, v3);
          } else {
            if constexpr (EPI == EPI_BIAS_GELU_H16) {
              auto gelu = [](float x) {
                const float p = __builtin_fmaf(x * x, -0.10294324f, -2.3022082f);
                return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(p * x));
              };
              v0 = gelu(v0); v1 = gelu(v1); v2 = gelu(v2); v3 = gelu(v3);
            }
            const u32x2 p = {pack2<DT>(v0, v1), pack2<DT>(v2, v3)};
            *(u32x2*)((half_t*)g.out + o) = p;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  };

  u32x4 bf[2][FN], af[8];
  auto fill = [&](const char* sA, const char* sB) {   // the complete first half-step and the B fragments of the second
#pragma unroll
    for (int j = 0; j < FN; ++j) bf[0][j] = *(const u32x4*)(sB + (b_off + j * 2048));
#pragma unroll
    for (int i = 0; i < 8; ++i) af[i] = *(const u32x4*)(sA + (a_off + i * 2048));
#pragma unroll
    for (int j = 0; j < FN; ++j) bf[1][j] = *(const u32x4*)(sB + ((b_off + j * 2048) ^ 64));
  };

  int pos = slot, tm, tn;
  decode(chunk0 + pos, tm, tn);
  __builtin_amdgcn_s_barrier();   // P: K tile 0 has landed
  fill(smem, smem);

  // One K tile of the pipeline; LOOK = read the fragments of stage u + 1 while the second half-step computes.
  // ROLL_IN is true.  It is named in ktile's LOOK conditions because the closure then holds a reference to it, as it did to the measurement
  // switch that stood there, and without that member the compiler schedules the fp4 (LO = 2 / 3) instantiations differently
  // (tools/isa_diff.py); whoever next changes this kernel's code on purpose can drop it.
  constexpr bool ROLL_IN = true;
  auto ktile = [&](const char* sA, const char* sAn, const char* sBn, auto look) {
    constexpr bool LOOK = decltype(look)::value;
    // ---- h0(u): first-half MFMAs, second-half A fragments roll in
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int j = 0; j < FN; ++j) mfma16_ip<DT>(acc[i][j], bf[0][j], af[i]);
      af[i] = *(const u32x4*)(sA + ((a_off + i * 2048) ^ 64));
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- h1(u), fragment rows 0-1; then every read of stage u has completed: B_u
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < FN; ++j) mfma16_ip<DT>(acc[i][j], bf[1][j], af[i]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (LOOK && ROLL_IN) {
#pragma unroll
      for (int j = 0; j < FN; ++j) bf[0][j] = *(const u32x4*)(sBn + (b_off + j * 2048));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 2; i < 8; ++i) {
#pragma unroll
      for (int j = 0; j < FN; ++j) mfma16_ip<DT>(acc[i][j], bf[1][j], af[i]);
      if constexpr (LOOK && ROLL_IN) af[i - 2] = *(const u32x4*)(sAn + (a_off + (i - 2) * 2048));
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (LOOK && ROLL_IN) {
      af[6] = *(const u32x4*)(sAn + (a_off + 6 * 2048));
      af[7] = *(const u32x4*)(sAn + (a_off + 7 * 2048));
#pragma unroll
      for (int j = 0; j < FN; ++j) bf[1][j] = *(const u32x4*)(sBn + ((b_off + j * 2048) ^ 64));
    }
  };

  // ---- correction K tiles (LO): the B pairs of the tile in b8, the A pairs in a ring of four (a8[i & 3] = fragment row i); same
  // one-barrier protocol as ktile(): every read of stage u has returned in front of B_u, stage u + 1 is read behind it.
  //   rows 0-3: 3 MFMAs each, the pair of row i + 4 rolls into the ring slot just read | rows 4-5 | lgkmcnt(0), B_u |
  //   rows 6-7, with LOOK the pairs of stage u + 1 roll in behind the MFMAs that free their registers (A rows 0-3, then B)
  u32x8 b8[FN], a8[4];
  unsigned sc_w = 0, sc_a = 0;
  if constexpr (LO == 1) {
    sc_w = 127u - LO8_W_SHIFT;
    sc_a = 127u - LO8_A_SHIFT;
    asm volatile("" : "+v"(sc_w), "+v"(sc_a));
  }
  auto pair_a = [&](const char* sA, int i) {
    return cat8(*(const u32x4*)(sA + (a_off + i * 2048)), *(const u32x4*)(sA + ((a_off + i * 2048) ^ 64)));
  };
  auto pair_b = [&](const char* sB, int j) {
    return cat8(*(const u32x4*)(sB + (b_off + j * 2048)), *(const u32x4*)(sB + ((b_off + j * 2048) ^ 64)));
  };
  auto lo_fill = [&](const char* sA, const char* sB) {
#pragma unroll
    for (int j = 0; j < FN; ++j) b8[j] = pair_b(sB, j);
#pragma unroll
    for (int i = 0; i < 4; ++i) a8[i] = pair_a(sA, i);
  };
  auto lo_tile = [&](const char* sA, const char* sAn, const char* sBn, auto look) {
    constexpr bool LOOK = decltype(look)::value;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < FN; ++j) mfma8_ip(acc[i][j], b8[j], a8[i], sc_w, sc_a);
      a8[i] = pair_a(sA, i + 4);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 4; i < 6; ++i) {
#pragma unroll
      for (int j = 0; j < FN; ++j) mfma8_ip(acc[i][j], b8[j], a8[i & 3], sc_w, sc_a);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (LOOK) {
      a8[0] = pair_a(sAn, 0);
      a8[1] = pair_a(sAn, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < FN; ++j) mfma8_ip(acc[6][j], b8[j], a8[2], sc_w, sc_a);
    if constexpr (LOOK) a8[2] = pair_a(sAn, 2);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      mfma8_ip(acc[7][j], b8[j], a8[3], sc_w, sc_a);
      if constexpr (LOOK) b8[j] = pair_b(sBn, j);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (LOOK) a8[3] = pair_a(sAn, 3);
  };

  // ---- FP4 correction K tiles (LO == 2, round 6): a K tile is 128 row bytes = K 256; the two 16-byte reads of a fragment row are two
  // operands of v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz = blgp = 4: 4 passes, layout H0 of tools/mx_probe.hip -- lane (row, g) holds the 32
  // consecutive K of chunk g), so a stage is walked as two HALVES (chunks 0-3, then 4-7) with half-size register sets; the scale operand
  // of a lane is the E8M0 byte of ITS row (GemmArgs::A4s / W4s), eight + three per tile, packed four to a register and shifted into byte 0.
  u32x4 b4[FN], a4[4];
  unsigned sa_pk[2] = {0u, 0u}, sw_pk = 0u;
  auto rd_a4 = [&](const char* sA, int i, int h) { return *(const u32x4*)(sA + ((a_off + i * 2048) ^ (h << 6))); };
  auto rd_b4 = [&](const char* sB, int j, int h) { return *(const u32x4*)(sB + ((b_off + j * 2048) ^ (h << 6))); };
  auto mfma4_ip = [](f32x4& c, const u32x4& a, const u32x4& b, unsigned sa_, unsigned sb_) {
    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0] cbsz:4 blgp:4"
                 : "+v"(c) : "v"(a), "v"(b), "v"(sa_), "v"(sb_));
  };
  auto lo4_scales = [&](int tm_, int tn_) {
    if constexpr (LO >= 2) {
      const int r = lane & 15;
      const unsigned char* as = g.A4s + (size_t)tm_ * BM + grp * 128 + r;
      const unsigned char* ws = g.W4s + (size_t)tn_ * BN + wn * WTN + r;
      sa_pk[0] = (unsigned)as[0] | ((unsigned)as[16] << 8) | ((unsigned)as[32] << 16) | ((unsigned)as[48] << 24);
      sa_pk[1] = (unsigned)as[64] | ((unsigned)as[80] << 8) | ((unsigned)as[96] << 16) | ((unsigned)as[112] << 24);
      sw_pk = (unsigned)ws[0] | ((unsigned)ws[16] << 8) | ((unsigned)ws[32] << 16);
    }
  };
  auto lo4_fill = [&](const char* sA, const char* sB) {
#pragma unroll
    for (int j = 0; j < FN; ++j) b4[j] = rd_b4(sB, j, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) a4[i] = rd_a4(sA, i, 0);
  };
  // LO == 3: the last fp4 tile of a row whose codes end inside its first half (0 < K % 256 <= 128: K = 1152) walks half 0 only -- a
  // COMPILE-TIME choice (the launcher picks the instantiation): as a run-time branch it cost 532 bytes of scratch per lane (behind the
  // branch the register allocator no longer keeps the in-place accumulators where they are) and +340 us per fc1 launch.
  auto lo4_tail = [&](const char* sA) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < FN; ++j) mfma4_ip(acc[i][j], b4[j], a4[i], sw_pk >> (8 * j), sa_pk[0] >> (8 * i));
      a4[i] = rd_a4(sA, i + 4, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 4; i < 8; ++i) {
#pragma unroll
      for (int j = 0; j < FN; ++j) mfma4_ip(acc[i][j], b4[j], a4[i & 3], sw_pk >> (8 * j), sa_pk[1] >> (8 * (i & 3)));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };
  auto lo4_tile = [&](const char* sA, const char* sB, const char* sAn, const char* sBn, auto look) {
    constexpr bool LOOK = decltype(look)::value;
    // half 0: rows 0-3 (rows 4-7 of the half roll in), rows 4-7 (rows 0-3 of half 1 roll in; B of half 1 behind row 7's MFMAs)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < FN; ++j) mfma4_ip(acc[i][j], b4[j], a4[i], sw_pk >> (8 * j), sa_pk[0] >> (8 * i));
      a4[i] = rd_a4(sA, i + 4, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 4; i < 8; ++i) {
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        mfma4_ip(acc[i][j], b4[j], a4[i & 3], sw_pk >> (8 * j), sa_pk[1] >> (8 * (i & 3)));
        if (i == 7) b4[j] = rd_b4(sB, j, 1);
      }
      a4[i & 3] = rd_a4(sA, i - 4, 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    // half 1: as the fp8 tile -- rows 0-3 | rows 4-5 | lgkmcnt(0), B_u | rows 6-7 with the look-ahead of stage u + 1 (half 0)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < FN; ++j) mfma4_ip(acc[i][j], b4[j], a4[i], sw_pk >> (8 * j), sa_pk[0] >> (8 * i));
      a4[i] = rd_a4(sA, i + 4, 1);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 4; i < 6; ++i) {
#pragma unroll
      for (int j = 0; j < FN; ++j) mfma4_ip(acc[i][j], b4[j], a4[i & 3], sw_pk >> (8 * j), sa_pk[1] >> (8 * (i & 3)));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (LOOK) {
      a4[0] = rd_a4(sAn, 0, 0);
      a4[1] = rd_a4(sAn, 1, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < FN; ++j) mfma4_ip(acc[6][j], b4[j], a4[2], sw_pk >> (8 * j), sa_pk[1] >> 16);
    if constexpr (LOOK) a4[2] = rd_a4(sAn, 2, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      mfma4_ip(acc[7][j], b4[j], a4[3], sw_pk >> (8 * j), sa_pk[1] >> 24);
      if constexpr (LOOK) b4[j] = rd_b4(sBn, j, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (LOOK) a4[3] = rd_a4(sAn, 3, 0);
  };

  int it = 0, ia = 0;
  for (;;) {
    for (int kt = 0; kt + 1 < nk; ++kt, ++it) {
      const char* sA = smem + ia * A_BYTES;
      ia = ia == NA - 1 ? 0 : ia + 1;
      ktile(sA, smem + ia * A_BYTES, smem + ((it + 1) & 1) * B_BYTES, std::true_type{});
    }
    {  // last K tile of the output tile: drain, epilogue, refill from stage u + 1 (landed at B_u)
      const char* sA = smem + ia * A_BYTES;
      ia = ia == NA - 1 ? 0 : ia + 1;
      ktile(sA, nullptr, nullptr, std::false_type{});
      ++it;
      if constexpr (LO >= 2) {   // the fp4 correction K tiles (see lo4_tile)
        lo4_scales(tm, tn);
        lo4_fill(smem + ia * A_BYTES, smem + (it & 1) * B_BYTES);
        for (int k8 = 0; k8 + 1 < nk8; ++k8, ++it) {
          const char* sA8 = smem + ia * A_BYTES;
          ia = ia == NA - 1 ? 0 : ia + 1;
          lo4_tile(sA8, smem + (it & 1) * B_BYTES, smem + ia * A_BYTES, smem + ((it + 1) & 1) * B_BYTES, std::true_type{});
        }
        const char* sA8 = smem + ia * A_BYTES;
        ia = ia == NA - 1 ? 0 : ia + 1;
        if constexpr (LO == 3) lo4_tail(sA8);
        else lo4_tile(sA8, smem + (it & 1) * B_BYTES, nullptr, nullptr, std::false_type{});
        ++it;
      } else if constexpr (LO) {   // the correction K tiles: stage `it` landed at the barrier of the tile above
        lo_fill(smem + ia * A_BYTES, smem + (it & 1) * B_BYTES);
        for (int k8 = 0; k8 + 1 < nk8; ++k8, ++it) {
          const char* sA8 = smem + ia * A_BYTES;
          ia = ia == NA - 1 ? 0 : ia + 1;
          lo_tile(sA8, smem + ia * A_BYTES, smem + ((it + 1) & 1) * B_BYTES, std::true_type{});
        }
        const char* sA8 = smem + ia * A_BYTES;
        ia = ia == NA - 1 ? 0 : ia + 1;
        lo_tile(sA8, nullptr, nullptr, std::false_type{});
        ++it;
      }
      asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // MFMA results -> VALU reads (see mfma16_ip)
      epilogue(tm, tn);
    }
    pos += per;
    if (pos >= cnt) break;
    decode(chunk0 + pos, tm, tn);
    fill(smem + ia * A_BYTES, smem + (it & 1) * B_BYTES);
  }
}


// ------------------------------------------------------------------------------------------------

// roll != 0: the rolling schedule (variant 11), else the two-segment one (variant 10)
// the rolling kernel's gated-residual instantiations: residual access shape (GemmArgs::rmw_mode) x call site / correction pass
// and, for the plain (LO == 0) forms, the policy of the A-operand stream (GemmArgs::stream_policy: fc2's bit for TAG 1, the
// out-projection's for TAG 0)
template <int DT, int TAG, int LO>
int launch_pwr_gated(const GemmArgs& a, dim3 grid, dim3 block, int lds, hipStream_t st) {
  if constexpr (LO == 0) {
    if (a.stream_policy & (TAG ? SP_FC2_A : SP_PROJ_A)) {
      if (a.rmw_mode) return launch_lds<gemm_pwr_kernel<EPI_GATE_RES_F32, DT, TAG, LO, 1, 1>>(grid, block, lds, st, a);
      return launch_lds<gemm_pwr_kernel<EPI_GATE_RES_F32, DT, TAG, LO, 0, 1>>(grid, block, lds, st, a);
    }
  }
  if (a.rmw_mode) return launch_lds<gemm_pwr_kernel<EPI_GATE_RES_F32, DT, TAG, LO, 1>>(grid, block, lds, st, a);
  return launch_lds<gemm_pwr_kernel<EPI_GATE_RES_F32, DT, TAG, LO, 0>>(grid, block, lds, st, a);
}

template <int EPI, int DT, int TAG>
int launch_pw_roll(const GemmArgs& a, int roll, dim3 grid, dim3 block, int lds, hipStream_t st) {
  if constexpr (EPI == EPI_GATE_RES_F32) {
    if (roll) return launch_pwr_gated<DT, TAG, 0>(a, grid, block, lds, st);
  } else {
    if (roll) return launch_lds<gemm_pwr_kernel<EPI, DT, TAG>>(grid, block, lds, st, a);
  }
  return launch_lds<gemm_pw_kernel<EPI, DT, TAG>>(grid, block, lds, st, a);
}

template <int DT>
int launch_pw_dt(const GemmArgs& a, int epi, int roll, hipStream_t st) {
  constexpr int LDS = 3 * 256 * 128 + 2 * 192 * 128 + 8 * 16 * 112;   // A ring + B ring + epilogue patches (rolling kernel)
  const int tiles = ((a.M + 255) / 256) * (a.N / 192);
  const int nblk = tiles >= 256 ? 256 : (tiles + 7) / 8 * 8;
  dim3 grid(nblk), block(768);
  if ((a.A4 || a.A8) && a.te) return fail(LATTE_ERR_INVALID, "gemm: GemmArgs::te has no correction-pass form");
  if (a.A4) {   // fp4 correction pass (GemmArgs::A4 / W4 + row scales): the rolling kernel's LO = 2 instantiations
    if (!roll || !a.W4 || !a.A4s || !a.W4s || !(epi == EPI_GATE_RES_F32 || epi == EPI_BIAS_GELU_H16) || DT != LATTE_DTYPE_F16)
      return fail(LATTE_ERR_INVALID, "gemm: the fp4 correction pass needs the rolling kernel, f16 operands, both code images with their row scales, and the gated / GELU epilogue");
    if constexpr (DT == LATTE_DTYPE_F16) {
      const bool half_tail = (a.K & 255) != 0 && (a.K & 255) <= 128;   // the last code tile ends inside its first half: LO = 3
      if (epi == EPI_GATE_RES_F32)
        return half_tail ? launch_pwr_gated<DT, 0, 3>(a, grid, block, LDS, st) : launch_pwr_gated<DT, 0, 2>(a, grid, block, LDS, st);
      return half_tail ? launch_lds<gemm_pwr_kernel<EPI_BIAS_GELU_H16, DT, 0, 3>>(grid, block, LDS, st, a)
                       : launch_lds<gemm_pwr_kernel<EPI_BIAS_GELU_H16, DT, 0, 2>>(grid, block, LDS, st, a);
    }
    return LATTE_OK;   // (not reached: bf16 was refused above)
  }
  if (a.A8) {   // correction pass (GemmArgs::A8 / W8): the rolling kernel's LO instantiations, out-projection and fc1 of guided calls
    if (!roll || !a.W8 || a.K % 128 != 0 || !(epi == EPI_GATE_RES_F32 || epi == EPI_BIAS_GELU_H16) || DT != LATTE_DTYPE_F16)
      return fail(LATTE_ERR_INVALID, "gemm (correction pass): rolling kernel, f16 operands, K % 128 == 0, gated-residual or GELU epilogue only");
    if constexpr (DT == LATTE_DTYPE_F16) {
      if (epi == EPI_GATE_RES_F32) return launch_pwr_gated<DT, 0, 1>(a, grid, block, LDS, st);
      return launch_lds<gemm_pwr_kernel<EPI_BIAS_GELU_H16, DT, 0, 1>>(grid, block, LDS, st, a);
    }
    return LATTE_OK;   // (not reached: bf16 was refused above)
  }
  switch (epi) {
    case EPI_GATE_RES_F32:
      if (a.te) {   // fc2 + temporal embedding (GemmArgs::te): the rolling kernel's TAG = 2 instantiations
        if (!roll || a.te_T <= 0 || a.te_F <= 0) return fail(LATTE_ERR_INVALID, "gemm (producer-wave kernel): GemmArgs::te needs the rolling kernel and te_T, te_F > 0");
        if (a.stream_policy & SP_FC2_A) return launch_lds<gemm_pwr_kernel<EPI_GATE_RES_F32, DT, 2, 0, 0, 1>>(grid, block, LDS, st, a);
        return launch_lds<gemm_pwr_kernel<EPI_GATE_RES_F32, DT, 2, 0, 0>>(grid, block, LDS, st, a);
      }
      if (a.tag == 1) return launch_pw_roll<EPI_GATE_RES_F32, DT, 1>(a, roll, grid, block, LDS, st);
      return launch_pw_roll<EPI_GATE_RES_F32, DT, 0>(a, roll, grid, block, LDS, st);
    case EPI_BIAS_F32: return launch_pw_roll<EPI_BIAS_F32, DT, 0>(a, roll, grid, block, LDS, st);
    case EPI_BIAS_H16: return launch_pw_roll<EPI_BIAS_H16, DT, 0>(a, roll, grid, block, LDS, st);
    case EPI_BIAS_GELU_H16: return launch_pw_roll<EPI_BIAS_GELU_H16, DT, 0>(a, roll, grid, block, LDS, st);
    case EPI_BIAS_GELU_DUAL_H16:
    case EPI_DGELU_H16:   // training epilogues: rolling kernel only
      if (!roll || !a.aux) return fail(LATTE_ERR_INVALID, "gemm (producer-wave kernel): the GELU training epilogues need the rolling kernel and GemmArgs::aux");
      if (epi == EPI_BIAS_GELU_DUAL_H16) return launch_lds<gemm_pwr_kernel<EPI_BIAS_GELU_DUAL_H16, DT, 0>>(grid, block, LDS, st, a);
      return launch_lds<gemm_pwr_kernel<EPI_DGELU_H16, DT, 0>>(grid, block, LDS, st, a);
    default: return fail(LATTE_ERR_INVALID, "gemm (producer-wave kernel): unknown epilogue");
  }
}

}  // namespace

bool gemm_lo4_ok(int M, int N, int K) {
  return M > 0 && N % 192 == 0 && K % 64 == 0 && K >= 128 && (uint64_t)((M + 255) / 256 * 256) * K * 2 < (1ull << 32) &&
         (uint64_t)N * K * 2 < (1ull << 32);
}
bool gemm_lo8_ok(int M, int N, int K) {
  return M > 0 && N % 192 == 0 && K % 128 == 0 && K >= 128 && (uint64_t)((M + 255) / 256 * 256) * K * 2 < (1ull << 32) &&
         (uint64_t)N * K * 2 < (1ull << 32);
}

// variant 10: limits of the 32-bit buffer offsets and K >= 128 as for the persistent kernel; whole 192-wide tile columns
int launch_gemm_pw(const GemmArgs& a, int epi, int dtype, int roll, hipStream_t st) {
  if (a.N % 192 != 0 || a.K % 64 != 0 || a.K < 128 || a.M <= 0)
    return fail(LATTE_ERR_INVALID, "gemm (producer-wave kernel): need N % 192 == 0, K % 64 == 0, K >= 128");
  if ((uint64_t)((a.M + 255) / 256 * 256) * a.K * 2 >= (1ull << 32) || (uint64_t)a.N * a.K * 2 >= (1ull << 32))
    return fail(LATTE_ERR_INVALID, "gemm (producer-wave kernel): operand exceeds the 4 GiB buffer-offset range");
  if (dtype == LATTE_DTYPE_BF16) return launch_pw_dt<LATTE_DTYPE_BF16>(a, epi, roll, st);
  if (dtype == LATTE_DTYPE_F16) return launch_pw_dt<LATTE_DTYPE_F16>(a, epi, roll, st);
  return fail(LATTE_ERR_INVALID, "gemm: unknown dtype");
}

}  // namespace latte
