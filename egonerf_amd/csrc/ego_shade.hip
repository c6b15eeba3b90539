// libegonerf_hip.so, part 2: appearance lookup -> basis -> positional encoding -> MLP_Fea, on the
// fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 FMA chains, so parity with the reference's
// fp32 Linear layers is rounding-order only).
//
// The work mapping (a wave owns a tile of 32 samples, lane l serves sample l & 31 and half l >> 5) and the K order per lane half
// that the packers bake into the weights are described in ego_tuned.h.
//
// W1/W2/W3/biases (150.5 KB packed) live in LDS for the whole persistent workgroup (8 waves = 2 per
// SIMD, so one wave's gather overlaps the other's MFMA chain); the basis fragments stream from L2.
#include "ego_tuned.h"
#include "variants.h"
#include "ego_generic.h"
#include "ego_march.h"

namespace {

enum { MODE_SHADE = 0, MODE_APP = 1, MODE_MLP = 2 };

struct ShadeArgs {
  DevCoords c;
  DevField F;
  const float* packed;
  const float* rays;  // MODE_SHADE: [N][6]
  const float* z;     // MODE_SHADE: [N][S]
  const float* coords;  // MODE_SHADE, optional: [N][S][4] = (r^, theta^, phi^, is_yang) from ego_march_density
  const float* c7n;   // MODE_APP: [M][7]
  const float* feat;  // MODE_MLP: [M][27]
  const float* dirs;  // MODE_MLP: [M][3]
  float* out;         // rgb [M][3] or feat [M][27]
  uint16_t* dump_x;   // training forward (MODE_SHADE, f16x3): activations kept for the backward pass, lane-contiguous
  uint16_t* dump_h1;  //   [M][160] X, [M][128] relu(H1), [M][128] relu(H2) as halves [tile][k-step][lane][8]; [M][144] v fp32 (include/egonerf_hip.h)
  uint16_t* dump_h2;
  float* dump_v;
  float* dump_fe;       // [tile][quad 0..3][lane][4]: the lane's 16 feature slots (basis output), fp32: the backward re-derives the encodings from them
  uint32_t* dump_bits;  // [tile][layer 0: h1, 1: h2][lane][2]: bit 16 (mt & 1) + r of word mt >> 1 <=> post-ReLU unit (mt, r) of the lane > 0
  const uint8_t* tile_active;  // optional [n_tiles]: 0 = every weight of the tile is zero, skip it
  // FOLD (ego_shade_composite): compositing in the kernel's epilogue instead of per-sample colours
  const float* comp_w;    // [N][S] weights
  const float* comp_bg;   // [N] background weight (with an envmap)
  const float* envmap;    // emission or null
  int32_t envmap_h;
  float* rgb_map;         // [N][3]
  float* depth;           // [N] or null
  float* bg_map;          // [N][3] or null
  float* env_map;         // [N][3] or null
  int64_t M;
  int32_t S;
  // COMPACT (ego_shade_live): lane j of tile t shades sample live[32 t + j] of [N][S]; the tile count follows from *n_live (device)
  const int32_t* live;
  const int32_t* n_live;
};

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// The gather/basis phase runs in 6 stages (plane ST>>1, channel quads 3*(ST&1)..+2 of this lane's 24-channel half):
// 18 x 16-byte loads in flight per lane per stage, 12 products, 12 basis k-steps.
constexpr int STQ = 3;                 // float4 quads per stage
constexpr int STV = STQ * 4;           // products per stage

template <int ST>
__device__ __forceinline__ void gather_stage(const DevField& F, const VMTaps& t, int g, int h, float v[STV]) {
#pragma clang fp contract(fast)  // built with -ffp-contract=off; interpolation may use FMAs
  constexpr int I = ST >> 1, Q0 = STQ * (ST & 1);
  const Lin1 X = t.ax[vm_plane_x(I)], Y = t.ax[vm_plane_y(I)], Ln = t.ax[vm_line_ax(I)];
  const int W = F.res[vm_plane_x(I)];
  const float* P = (g ? F.plane[1][I] : F.plane[0][I]) + 4 * h + 8 * Q0;
  const float* L = (g ? F.line[1][I] : F.line[0][I]) + 4 * h + 8 * Q0;
  const f32x4* p00 = (const f32x4*)(P + (Y.i0 * W + X.i0) * APP_C);
  const f32x4* p01 = (const f32x4*)(P + (Y.i0 * W + X.i1) * APP_C);
  const f32x4* p10 = (const f32x4*)(P + (Y.i1 * W + X.i0) * APP_C);
  const f32x4* p11 = (const f32x4*)(P + (Y.i1 * W + X.i1) * APP_C);
  const f32x4* l0 = (const f32x4*)(L + Ln.i0 * APP_C);
  const f32x4* l1 = (const f32x4*)(L + Ln.i1 * APP_C);
  const float w00 = __fmul_rn(Y.w0, X.w0), w01 = __fmul_rn(Y.w0, X.w1);
  const float w10 = __fmul_rn(Y.w1, X.w0), w11 = __fmul_rn(Y.w1, X.w1);
#pragma unroll
  for (int q = 0; q < STQ; ++q) {
    const f32x4 pv = p00[2 * q] * w00 + p01[2 * q] * w01 + p10[2 * q] * w10 + p11[2 * q] * w11;
    const f32x4 lv = l0[2 * q] * Ln.w0 + l1[2 * q] * Ln.w1;
    const f32x4 m = pv * lv;
    v[q * 4 + 0] = m.x; v[q * 4 + 1] = m.y; v[q * 4 + 2] = m.z; v[q * 4 + 3] = m.w;
  }
}

// basis A fragments of stage ST for grid gsel (streamed from L2, fetched one stage ahead of their MFMAs)
template <int ST>
__device__ __forceinline__ void basis_load(const f32x4* __restrict__ BAS, int lane, int gsel, f32x4 a[STQ]) {
#pragma unroll
  for (int q = 0; q < STQ; ++q) a[q] = BAS[(gsel * (KS_BASIS / 4) + ST * STQ + q) * 64 + lane];
}

__device__ __forceinline__ void basis_mfma(const f32x4 a[STQ], const float v[STV], bool keep, f32x16& fe) {
#pragma unroll
  for (int q = 0; q < STQ; ++q) {
    fe = MFMA(a[q].x, keep ? v[q * 4 + 0] : 0.f, fe);
    fe = MFMA(a[q].y, keep ? v[q * 4 + 1] : 0.f, fe);
    fe = MFMA(a[q].z, keep ? v[q * 4 + 2] : 0.f, fe);
    fe = MFMA(a[q].w, keep ? v[q * 4 + 3] : 0.f, fe);
  }
}

// a wave that straddles the yin/yang border (rare: ~0.8 crossings per 512-sample ray) runs the second weight set
// with the first grid's samples zeroed on the B side (a lane only feeds its own output column)
template <int ST>
__device__ __forceinline__ void basis_mixed(const f32x4* __restrict__ BAS, int lane, int g, const float v[STV], f32x16& fe) {
  f32x4 a[STQ];
  basis_load<ST>(BAS, lane, 1, a);
  basis_mfma(a, v, g != 0, fe);
}

// a layer's accumulators start from its bias: B = [4 m][2 h][16 r] as float4 quads (OFF_B1 / OFF_B2 of the LDS image), hw = the lane half.
// A macro, used by k_shade and k_shade_h: as a function it hands the kernels another address form and seven of k_shade_h's instances change
#define EGO_LOAD_BIAS(B, ACC)                                                                                      \
  _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) _Pragma("unroll") for (int q = 0; q < 4; ++q) {                \
    const f32x4 b = (B)[(mt * 2 + hw) * 4 + q];                                                                    \
    ACC[mt][q * 4 + 0] = b.x; ACC[mt][q * 4 + 1] = b.y; ACC[mt][q * 4 + 2] = b.z; ACC[mt][q * 4 + 3] = b.w;        \
  }

template <int MODE, bool COMPACT = false>
__global__ __launch_bounds__(512) void k_shade(ShadeArgs A) {
  static_assert(!COMPACT || MODE == MODE_SHADE, "the live-sample list is an input of the shade only");
  __shared__ __attribute__((aligned(16))) float lds[(MODE == MODE_APP ? 0 : LDS_W_FLOATS) + (MODE == MODE_MLP ? 4 : LUT_MAX)];
  float* lut = lds + (MODE == MODE_APP ? 0 : LDS_W_FLOATS);
  if (MODE != MODE_APP) {
    const f32x4* src = (const f32x4*)A.packed;
    f32x4* dst = (f32x4*)lds;
    for (int i = threadIdx.x; i < LDS_W_FLOATS / 4; i += 512) dst[i] = src[i];
  }
  if (MODE == MODE_SHADE)
    for (int i = threadIdx.x; i < A.c.n_lut; i += 512) lut[i] = A.c.r_lut[i];
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  // waves w and w+4 share a SIMD and would otherwise run their gather and MFMA phases in lockstep (equal sharing
  // of the matrix pipe keeps them synchronised); a static priority for one of them staggers the phases
  if (wave >= 4) __builtin_amdgcn_s_setprio(1);
  const int32_t n_live = COMPACT ? *A.n_live : 0;
  const int64_t n_tiles = ((COMPACT ? (int64_t)n_live : A.M) + 31) >> 5;
  const f32x4* W1 = (const f32x4*)(lds + OFF_W1);
  const f32x4* W2 = (const f32x4*)(lds + OFF_W2);
  const f32x4* B1 = (const f32x4*)(lds + OFF_B1);
  const f32x4* B2 = (const f32x4*)(lds + OFF_B2);
  const f32x4* W3 = (const f32x4*)(lds + OFF_W3);
  const f32x4* BAS = (const f32x4*)(A.packed + OFF_BASIS);

  for (int64_t tile = (int64_t)blockIdx.x * 8 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 8) {
    if (MODE == MODE_SHADE && !COMPACT && A.tile_active && !A.tile_active[tile]) continue;
    // LDS weights are loop-invariant: without an opaque per-iteration index LICM hoists all 240
    // ds_read_b128 out of the tile loop and spills them to scratch
    int lw = lane;
    asm volatile("" : "+v"(lw));
    const int hw = lw >> 5;
    const int64_t m_raw = tile * 32 + j;
    const bool valid = m_raw < (COMPACT ? (int64_t)n_live : A.M);
    // COMPACT: the list entry (a lane past the end repeats the last live sample and writes nothing)
    const int64_t m = COMPACT ? (int64_t)A.live[valid ? m_raw : n_live - 1] : valid ? m_raw : A.M - 1;

    f32x16 fe;  // basis output: register r holds feature 2r + h
    float vd0 = 0.f, vd1 = 0.f, vd2 = 0.f;
    if (MODE == MODE_MLP) {
      const float* fp = A.feat + m * APP_DIM;
#pragma unroll
      for (int r = 0; r < 16; ++r) fe[r] = (r < NSLOT && 2 * r + h < APP_DIM) ? fp[min(2 * r + h, APP_DIM - 1)] : 0.f;
      vd0 = A.dirs[m * 3]; vd1 = A.dirs[m * 3 + 1]; vd2 = A.dirs[m * 3 + 2];
    } else {
      float a_r, a_th, a_ph;
      int g;
      if (MODE == MODE_APP) {
        const float* p = A.c7n + m * 7;
        g = (p[6] == 0.f) ? 0 : 1;
        const int b = g ? 3 : 0;
        a_r = p[b]; a_th = p[b + 1]; a_ph = p[b + 2];
      } else {
        const uint32_t ray = (uint32_t)m / (uint32_t)A.S;
        const float* R = A.rays + (int64_t)ray * 6;
        const float zz = A.z[m];
        vd0 = R[3]; vd1 = R[4]; vd2 = R[5];
        const float px = __fadd_rn(R[0], __fmul_rn(vd0, zz)), py = __fadd_rn(R[1], __fmul_rn(vd1, zz)),
                    pz = __fadd_rn(R[2], __fmul_rn(vd2, zz));
        const YinYang y = yinyang_from_xyz(px, py, pz, A.c);
        g = y.yang;
        a_r = normalize_r(y.r, lut, A.c.n_lut, A.c.n_r);
        a_th = normalize_ang(y.th, A.c.th_near, A.c.th_inv);
        a_ph = normalize_ang(y.ph, A.c.ph_near, A.c.ph_inv);
      }
      const bool any_yin = __ballot(g == 0) != 0ull, any_yang = __ballot(g != 0) != 0ull;
      const VMTaps taps = vm_setup(a_r, a_th, a_ph, A.F.res);
#pragma unroll
      for (int r = 0; r < 16; ++r) fe[r] = 0.f;
      // software pipeline over the 6 stages; sched_barriers keep the scheduler from hoisting every load to the top
      {
        const bool mixed = any_yin && any_yang;
        const int gu = any_yin ? 0 : 1;              // weight set of the first pass
        const bool keep = !mixed || g == 0;          // first pass keeps yin lanes only when the wave is mixed
        float vA[STV], vB[STV];
        f32x4 aA[STQ], aB[STQ];
        basis_load<0>(BAS, lane, gu, aA);
        gather_stage<0>(A.F, taps, g, h, vA);
        __builtin_amdgcn_sched_barrier(0);
#define EGO_STAGE(ST, vN, aN, vP, aP)                         \
        basis_load<ST>(BAS, lane, gu, aN);                    \
        gather_stage<ST>(A.F, taps, g, h, vN);                \
        basis_mfma(aP, vP, keep, fe);                         \
        if (mixed) basis_mixed<ST - 1>(BAS, lane, g, vP, fe); \
        __builtin_amdgcn_sched_barrier(0);
        EGO_STAGE(1, vB, aB, vA, aA)
        EGO_STAGE(2, vA, aA, vB, aB)
        EGO_STAGE(3, vB, aB, vA, aA)
        EGO_STAGE(4, vA, aA, vB, aB)
        EGO_STAGE(5, vB, aB, vA, aA)
#undef EGO_STAGE
        basis_mfma(aB, vB, keep, fe);
        if (mixed) basis_mixed<5>(BAS, lane, g, vB, fe);
      }
    }

    if (MODE == MODE_APP) {
      if (valid) {
        float* o = A.out + m * APP_DIM;
#pragma unroll
        for (int r = 0; r < NSLOT; ++r)
          if (2 * r + h < APP_DIM) o[2 * r + h] = fe[r];
      }
      continue;
    }

    // ---- view-direction slots (3 raw + 12 encodings, 8 per lane half) -------------------------------
    float vw[8];
    view_slots<EncF32>(vd0, vd1, vd2, h, vw);

    // ---- layer 1: 150 -> 128.  K-outer: four accumulators (one per 32-unit M-tile) stay live, the
    // B operand of k-step kk is produced right before it is consumed -------------------------------
    f32x16 H[4];
    EGO_LOAD_BIAS(B1, H)
    {
      f32x4 a[4];
      float s1 = 0.f, c1 = 0.f, s2 = 0.f, c2 = 0.f;
#pragma unroll
      for (int kk = 0; kk < KS1; ++kk) {
        if ((kk & 3) == 0) {
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) a[mt] = W1[((kk >> 2) * 4 + mt) * 64 + lw];
        }
        const float x = layer1_value<EncF32>(kk, fe, vw, s1, c1, s2, c2);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) H[mt] = MFMA(a[mt][kk & 3], x, H[mt]);
      }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) H[mt][r] = relu_f(H[mt][r]);

    // ---- layer 2: 128 -> 128 (K-outer again), then layer 3: 128 -> 3 on the VALU -----------------------
    f32x16 G[4];
    EGO_LOAD_BIAS(B2, G)
    {
      f32x4 a[4];
#pragma unroll
      for (int kk = 0; kk < KS2; ++kk) {
        if ((kk & 3) == 0) {
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) a[mt] = W2[((kk >> 2) * 4 + mt) * 64 + lw];
        }
        const float x = H[kk >> 4][kk & 15];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) G[mt] = MFMA(a[mt][kk & 3], x, G[mt]);
      }
    }
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const f32x4 w = W3[(mt * 2 + hw) * 16 + r];
        const float hv = relu_f(G[mt][r]);
        o0 = fmaf(hv, w.x, o0); o1 = fmaf(hv, w.y, o1); o2 = fmaf(hv, w.z, o2);
      }
    o0 += __shfl_xor(o0, 32, 64);
    o1 += __shfl_xor(o1, 32, 64);
    o2 += __shfl_xor(o2, 32, 64);
    if (valid && h == 0) {
      const float* b3 = lds + OFF_B3;
      float* o = A.out + m * 3;
      o[0] = sigmoidf(o0 + b3[0]);
      o[1] = sigmoidf(o1 + b3[1]);
      o[2] = sigmoidf(o2 + b3[2]);
    }
  }
}


// =================================================================================================================
// f16x3 variant of k_shade: same dataflow, but every matrix product runs as three v_mfma_f32_32x32x16_f16
// (w_hi*x_hi + w_lo*x_hi + w_hi*x_lo, fp32 accumulate; the dropped lo*lo term and the 22-bit operands leave ~2^-21
// relative error, i.e. fp32-grade: 2.4e-7 max |dRGB| vs 1.4e-7 for the fp32 MFMA path on the oracle's inputs).
// fp16 subnormals are honoured by the instruction on gfx950 (tools/mfma_probe.hip), which the small x_lo terms need.
// 6 matrix-pipe cycles per K instead of 32.
// =================================================================================================================

// bit 16 (mt & 1) + r of word mt >> 1 is set iff unit (mt, r) of this lane is > 0 (relu'(0) = 0 like torch's threshold backward)
__device__ __forceinline__ u32x2 relu_bits(const f32x16 (&H)[4]) {
  u32x2 b = {0u, 0u};
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) b[mt >> 1] |= (H[mt][r] > 0.f ? 1u : 0u) << (16 * (mt & 1) + r);
  return b;
}

// ---- f16f8 arithmetic: main term in fp16, both correction terms in one block-scaled fp8 MFMA per pair of k-steps -------------
typedef int v8i __attribute__((ext_vector_type(8)));
typedef short v2s __attribute__((ext_vector_type(2)));
#define MFMA8(a, b, c) __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4((a), (b), (c), 0, 0, 0, 116 /* A block scale 2^-11 */, 0, 127)

// 8 values of one k-step -> fp16 main operand (returned) + this step's 16 bytes of the pair's fp8 operand b8:
// bytes [8 odd .. 8 odd + 7] = e4m3(x), bytes [16 + 8 odd .. ] = e4m3((x - fp16(x)) * 2^11)
__device__ __forceinline__ h8 split8_f8(const float x[8], v8i& b8, int odd) {
  u32x4 hi;
  uint32_t xh[2], xl[2];
  float neg1 = -1.0f;
  asm("" : "+v"(neg1));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float a = x[2 * q], b = x[2 * q + 1];
    // round-to-nearest fp16 (v_cvt_pk_f16_f32) rather than the truncating v_cvt_pkrtz of the three-term split: it halves the
    // residual, and with it the error the 4-bit fp8 copy of the residual leaves
    typedef float f2v __attribute__((ext_vector_type(2)));
    typedef _Float16 h2v __attribute__((ext_vector_type(2)));
    const h2v hp = __builtin_convertvector(f2v{a, b}, h2v);
    hi[q] = __builtin_bit_cast(uint32_t, hp);
    const float ra = __builtin_fmaf((float)hp[0], neg1, a), rb = __builtin_fmaf((float)hp[1], neg1, b);
    if ((q & 1) == 0) {
      // the low-half conversion keeps the other half of its destination, which the high-half conversion of the next value pair
      // overwrites: seed the destination with a value that is about to die (the operands themselves) rather than with a zero,
      // which costs a v_mov per operand register
      xh[q >> 1] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, __builtin_bit_cast(int, b), false);
      xl[q >> 1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(__builtin_bit_cast(v2s, rb), ra, rb, 1.0f / 2048.0f, false));
    } else {
      xh[q >> 1] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, (int)xh[q >> 1], true);
      xl[q >> 1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(__builtin_bit_cast(v2s, xl[q >> 1]), ra, rb,
                                                                                         1.0f / 2048.0f, true));
    }
  }
  b8[2 * odd] = (int)xh[0]; b8[2 * odd + 1] = (int)xh[1];
  b8[4 + 2 * odd] = (int)xl[0]; b8[4 + 2 * odd + 1] = (int)xl[1];
  return __builtin_bit_cast(h8, hi);
}

__device__ __forceinline__ v8i load_a8(const u32x4* __restrict__ WF, int pair, int mt, int lane) {
  const u32x4 p0 = WF[((pair * 4 + mt) * 2 + 0) * 64 + lane], p1 = WF[((pair * 4 + mt) * 2 + 1) * 64 + lane];
  return v8i{(int)p0.x, (int)p0.y, (int)p0.z, (int)p0.w, (int)p1.x, (int)p1.y, (int)p1.z, (int)p1.w};
}

// ---- f16f6 arithmetic (layout: k_pack_mlp_f6) ------------------------------------------------------------------------------------------
typedef int v16i __attribute__((ext_vector_type(16)));
typedef _Float16 h32 __attribute__((ext_vector_type(32)));
#define MFMA6(a, b, c, sa, opa, sb) __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4((a), (b), (c), 2, 2, (opa), (sa), 0, (sb))

// one k-step's 8 values -> packed fp16 main operand (also written to dwords 4 s .. 4 s + 3 of the group's hp), the 8 exact residuals
// x - fp16(x), and the running maximum of |x| over the group
// mmask (a constant after unrolling): bit e set = value e takes part in the maximum (layer 1 knows that its sines and cosines are bounded by 1)
__device__ __forceinline__ h8 split8_f6(const float x[8], uint32_t* hp, float* res, float& amax, int mmask = 0xff) {
  u32x4 hi;
  float neg1 = -1.0f;
  asm("" : "+v"(neg1));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float a = x[2 * q], b = x[2 * q + 1];
    typedef float f2v __attribute__((ext_vector_type(2)));
    typedef _Float16 h2v __attribute__((ext_vector_type(2)));
    const h2v hpv = __builtin_convertvector(f2v{a, b}, h2v);
    hi[q] = __builtin_bit_cast(uint32_t, hpv);
    hp[q] = hi[q];
    res[2 * q] = __builtin_fmaf((float)hpv[0], neg1, a);
    res[2 * q + 1] = __builtin_fmaf((float)hpv[1], neg1, b);
    const bool ma = (mmask >> (2 * q)) & 1, mb = (mmask >> (2 * q + 1)) & 1;
    if (ma && mb) amax = fmaxf(fmaxf(fabsf(a), fabsf(b)), amax);
    else if (ma) amax = fmaxf(fabsf(a), amax);
    else if (mb) amax = fmaxf(fabsf(b), amax);
  }
  return __builtin_bit_cast(h8, hi);
}

// The 32-value conversions run in passes and write their destination registers while later passes still read the scale and the
// sources: with the scale, or any but the first registers of a source tuple, in a destination register the result is wrong
// (tools/fp6_overlap_probe.hip, profiles/r04/fp6_overlap_probe.txt) - and this compiler's register allocator produces exactly such
// overlaps for the builtins (their definitions carry no early-clobber; keeping the operands live past the builtin does not help,
// the allocator copies tuples).  So the two conversions are issued through inline asm with an early-clobber destination.  What the
// compiler's hazard recogniser cannot see into is covered inside the block: one wait state before (a VALU result feeding the
// conversion) and two after it (conversion result -> MFMA operand needs one: tools/fp6_raw_probe.hip).
typedef uint32_t u32x6 __attribute__((ext_vector_type(6)));
__device__ __forceinline__ u32x6 cvt_pk32_fp6_f16(const v16i& halves, float scale) {
  u32x6 r;
  asm("s_nop 0\n\tv_cvt_scalef32_pk32_fp6_f16 %0, %1, %2\n\ts_nop 1" : "=&v"(r) : "v"(halves), "v"(scale));
  return r;
}
__device__ __forceinline__ u32x6 cvt_2xpk16_fp6_f32_dup(const f32x16& a, float scale) {   // both sources = a
  u32x6 r;
  asm("s_nop 0\n\tv_cvt_scalef32_2xpk16_fp6_f32 %0, %1, %1, %2\n\ts_nop 1" : "=&v"(r) : "v"(a), "v"(scale));
  return r;
}
__device__ __forceinline__ u32x6 cvt_2xpk16_fp6_f32(const f32x16& a, const f32x16& b, float scale) {
  u32x6 r;
  asm("s_nop 0\n\tv_cvt_scalef32_2xpk16_fp6_f32 %0, %1, %2, %3\n\ts_nop 1" : "=&v"(r) : "v"(a), "v"(b), "v"(scale));
  return r;
}

struct B6 {
  v8i x, r;   // fp6 operands of the two correction terms (dwords 6, 7 unused)
  int sb;     // B's block scale byte (biased exponent of the group's largest |x|)
};

__device__ __forceinline__ void f6_scales(float amax, int& eb, float& sx, float& sr) {
  uint32_t e = __float_as_uint(amax) >> 23;
  e = e < 14u ? 14u : e;
  eb = (int)e;
  sx = __uint_as_float((e - 2u) << 23);
  sr = __uint_as_float((e - 13u) << 23);
}

// full group: hp = the 16 packed-half dwords of its 32 values, res = their 32 residuals in value order
__device__ __forceinline__ B6 group6(const uint32_t hp[16], const float res[32], float amax) {
  B6 o;
  float sx, sr;
  f6_scales(amax, o.sb, sx, sr);
  v16i hv;
  f32x16 ra, rb;
#pragma unroll
  for (int i = 0; i < 16; ++i) { hv[i] = (int)hp[i]; ra[i] = res[i]; rb[i] = res[16 + i]; }
  const u32x6 x6 = cvt_pk32_fp6_f16(hv, sx);
  const u32x6 r6 = cvt_2xpk16_fp6_f32(ra, rb, sr);
  o.x = __builtin_bit_cast(v8i, __builtin_shufflevector(x6, x6, 0, 1, 2, 3, 4, 5, -1, -1));
  o.r = __builtin_bit_cast(v8i, __builtin_shufflevector(r6, r6, 0, 1, 2, 3, 4, 5, -1, -1));
  return o;
}

// half group (layer 1's last: 16 values): both operands through the interleaving conversion with the values as BOTH sources - the odd
// elements meet zero weights (f6_value), and no tuple of zeros has to be materialised
__device__ __forceinline__ B6 group6_half(const float xv[16], const float res[16], float amax) {
  B6 o;
  float sx, sr;
  f6_scales(amax, o.sb, sx, sr);
  f32x16 xa, ra;
#pragma unroll
  for (int i = 0; i < 16; ++i) { xa[i] = xv[i]; ra[i] = res[i]; }
  const u32x6 x6 = cvt_2xpk16_fp6_f32_dup(xa, sx);
  const u32x6 r6 = cvt_2xpk16_fp6_f32_dup(ra, sr);
  o.x = __builtin_bit_cast(v8i, __builtin_shufflevector(x6, x6, 0, 1, 2, 3, 4, 5, -1, -1));
  o.r = __builtin_bit_cast(v8i, __builtin_shufflevector(r6, r6, 0, 1, 2, 3, 4, 5, -1, -1));
  return o;
}

// Per-lane LDS byte offsets into the f16f6 image (opaque to the compiler, so that a read is `base + 16-bit immediate` and not an
// address computation of its own): one base per 64 KB window of the 16-byte-stride part, one for the scale bytes
struct F6Bases {
  uint32_t o16[3], o8s;   // lane * 16 + 64 KB * w, lane * 8 + 4 F6I_SC
};
__device__ __forceinline__ F6Bases f6_bases(int lane) {
  F6Bases b;
  b.o16[0] = (uint32_t)lane * 16u; b.o16[1] = (uint32_t)lane * 16u + 65536u; b.o16[2] = (uint32_t)lane * 16u + 131072u;
  b.o8s = (uint32_t)lane * 8u + 4u * F6I_SC;
  asm volatile("" : "+v"(b.o16[0]), "+v"(b.o16[1]), "+v"(b.o16[2]), "+v"(b.o8s));
  return b;
}
// slot: 32-bit slot index of lane 0's element (a constant after unrolling)
__device__ __forceinline__ u32x4 f6_ld128(const float* lds, const F6Bases& b, int slot) {
  const int w = (slot * 4) >> 16;
  return *(const u32x4*)((const char*)lds + (slot * 4 - 65536 * w) + b.o16[w]);
}
__device__ __forceinline__ h8 f6_hi(const float* lds, const F6Bases& b, bool l2, int step, int mt) {
  return __builtin_bit_cast(h8, f6_ld128(lds, b, (l2 ? F6I_HI2 : F6I_HI1) + (step * 4 + mt) * 256));
}

// dwords 6, 7 of the builtin's operand type are not read by the fp6 form of the instruction and stay undefined
__device__ __forceinline__ v8i a6_operand(const u32x4& head, const u32x4& tails, int term) {
  return term == 0 ? __builtin_bit_cast(v8i, __builtin_shufflevector(head, tails, 0, 1, 2, 3, 4, 5, -1, -1))
                   : __builtin_bit_cast(v8i, __builtin_shufflevector(head, tails, 0, 1, 2, 3, 6, 7, -1, -1));
}

__device__ __forceinline__ void group_mfma6(const float* lds, const F6Bases& fb, bool l2, int grp, const B6& b, f32x16 (&H)[4]) {
  const u32x2 sa = *(const u32x2*)((const char*)lds + ((l2 ? G6_1 : 0) + grp) * 512 + fb.o8s);   // byte mt of .x: term 0's block scales, of .y: term 1's
  const int q = (l2 ? F6I_Q2 : F6I_Q1) + grp * 4 * 768;
  u32x4 hd[4], tl[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) { hd[mt] = f6_ld128(lds, fb, q + mt * 768); tl[mt] = f6_ld128(lds, fb, q + mt * 768 + 512); }
  H[0] = MFMA6(a6_operand(hd[0], tl[0], 0), b.x, H[0], (int)sa.x, 0, b.sb);
  H[1] = MFMA6(a6_operand(hd[1], tl[1], 0), b.x, H[1], (int)sa.x, 1, b.sb);
  H[2] = MFMA6(a6_operand(hd[2], tl[2], 0), b.x, H[2], (int)sa.x, 2, b.sb);
  H[3] = MFMA6(a6_operand(hd[3], tl[3], 0), b.x, H[3], (int)sa.x, 3, b.sb);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) hd[mt] = f6_ld128(lds, fb, q + mt * 768 + 256);
  H[0] = MFMA6(a6_operand(hd[0], tl[0], 1), b.r, H[0], (int)sa.y, 0, b.sb);
  H[1] = MFMA6(a6_operand(hd[1], tl[1], 1), b.r, H[1], (int)sa.y, 1, b.sb);
  H[2] = MFMA6(a6_operand(hd[2], tl[2], 1), b.r, H[2], (int)sa.y, 2, b.sb);
  H[3] = MFMA6(a6_operand(hd[3], tl[3], 1), b.r, H[3], (int)sa.y, 3, b.sb);
}

// ---- one MLP layer of k_shade_h per arithmetic (K-outer: KH1 / KH2 steps of 8 values per lane half, the four accumulators ACC stay
// live).  LAYER (1 or 2) picks the step count and the LDS region; SRC(step, xs) fills the step's eight values; `step` is a constant
// after unrolling everywhere.  Macros, expanded in k_shade_h and speaking of its locals (lds, lw, lane, tile, valid, A, DUMP):
// these kernels are tuned to the register, and as functions the bodies reach them in another instruction order (the layer-2
// fragment loads of f16x3 came out reversed) and their code changes.
// The two operand sources: the layer-1 generator (ego_tuned.h) over the kernel's fe / vw / s1 .. c2, and registers of layer 1's H
#define EGO_X_LAYER1(step, xs)                                              \
  _Pragma("unroll") for (int e = 0; e < 8; ++e) {                           \
    const int kk = (step) * 8 + e;                                          \
    if (layer1_slot_head(kk)) EncHw::enc(fe[kk / 5], s1, c1, s2, c2);       \
    xs[e] = EGO_LAYER1_PICK(kk, fe[kk / 5], s1, c1, s2, c2, vw);            \
  }
#define EGO_X_LAYER2(step, xs) \
  _Pragma("unroll") for (int e = 0; e < 8; ++e) xs[e] = H[((step) * 8 + e) >> 4][((step) * 8 + e) & 15];

// f16x3: A fragments [step][m-tile][hi|lo][lane] of the current / next k-step (LDS reads issued one step ahead).  The x dump of the
// training forward ([tile][k-step][lane][8 halves]) is optional (r05): ego_weight_grad_x re-derives x from the feature slots and
// the view direction
#define EGO_MLP_LAYER_F16X3(LAYER, W, ACC, SRC)                                                                                  \
  {                                                                                                                              \
    constexpr int KH = (LAYER) == 1 ? KH1 : KH2;                                                                                 \
    h8 ah[4], al[4], nh[4], nl[4];                                                                                               \
    _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) {                                                                           \
      nh[mt] = __builtin_bit_cast(h8, (W)[(mt * 2 + 0) * 64 + lw]);                                                              \
      nl[mt] = __builtin_bit_cast(h8, (W)[(mt * 2 + 1) * 64 + lw]);                                                              \
    }                                                                                                                            \
    _Pragma("unroll") for (int step = 0; step < KH; ++step) {                                                                    \
      float xs[8];                                                                                                               \
      SRC(step, xs);                                                                                                             \
      const HL b = split8(xs, true);                                                                                             \
      if (DUMP && (LAYER) == 1 && valid && A.dump_x)                                                                             \
        __builtin_nontemporal_store(pack8_rn(xs), &((u32x4*)A.dump_x)[(tile * KH1 + step) * 64 + lane]);                        \
      _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) { ah[mt] = nh[mt]; al[mt] = nl[mt]; }                                      \
      if (step + 1 < KH) {                                                                                                       \
        _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) {                                                                       \
          nh[mt] = __builtin_bit_cast(h8, (W)[(((step + 1) * 4 + mt) * 2 + 0) * 64 + lw]);                                       \
          nl[mt] = __builtin_bit_cast(h8, (W)[(((step + 1) * 4 + mt) * 2 + 1) * 64 + lw]);                                       \
        }                                                                                                                        \
      }                                                                                                                          \
      _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) ACC[mt] = MFMAH(ah[mt], b.hi, ACC[mt]);                                    \
      _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) ACC[mt] = MFMAH(al[mt], b.hi, ACC[mt]);                                    \
      _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) ACC[mt] = MFMAH(ah[mt], b.lo, ACC[mt]);                                    \
    }                                                                                                                            \
  }

// f16f8: W = the layer's region, hi fragments [step][m-tile][lane] first, the fp8 fragments [pair][m-tile][part][lane] behind them
#define EGO_MLP_LAYER_F8(LAYER, W, ACC, SRC)                                                                                     \
  {                                                                                                                              \
    constexpr int KH = (LAYER) == 1 ? KH1 : KH2;                                                                                 \
    const u32x4* WF = (W) + ((LAYER) == 1 ? F8_HI1 : F8_HI2) / 4;                                                                \
    h8 ah[4], nh[4];                                                                                                             \
    v8i a8[4], b8;                                                                                                               \
    _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) nh[mt] = __builtin_bit_cast(h8, (W)[mt * 64 + lw]);                         \
    _Pragma("unroll") for (int step = 0; step < KH; ++step) {                                                                    \
      float xs[8];                                                                                                               \
      SRC(step, xs);                                                                                                             \
      const h8 bh = split8_f8(xs, b8, step & 1);                                                                                 \
      _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) ah[mt] = nh[mt];                                                          \
      if (step + 1 < KH) {                                                                                                       \
        _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) nh[mt] = __builtin_bit_cast(h8, (W)[((step + 1) * 4 + mt) * 64 + lw]);  \
      }                                                                                                                          \
      if ((step & 1) == 0) { /* the pair's fp8 fragments: needed after the second step's main-term MFMAs */                      \
        _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) a8[mt] = load_a8(WF, step >> 1, mt, lw);                                \
      }                                                                                                                          \
      _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) ACC[mt] = MFMAH(ah[mt], bh, ACC[mt]);                                      \
      if (step & 1) {                                                                                                            \
        _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) ACC[mt] = MFMA8(a8[mt], b8, ACC[mt]);                                    \
      }                                                                                                                          \
    }                                                                                                                            \
  }

// f16f6: groups of four steps; layer 1's last group holds only steps 8, 9 (xl = their 16 values).  The block maximum only has to
// look at layer 1's unbounded values: every one of its groups holds cosines of magnitude ~1 and nothing else above 1, so its
// running maximum starts at 1.  Step-outer / value-inner on purpose: a flat loop over the values exceeds the unroller's size limit
// with the group code in its body, and a rolled loop indexes the register arrays through scratch.
#define EGO_MLP_LAYER_F6(LAYER, ACC, SRC)                                                                                        \
  {                                                                                                                              \
    constexpr int KH = (LAYER) == 1 ? KH1 : KH2;                                                                                 \
    constexpr bool L2 = (LAYER) == 2;                                                                                            \
    constexpr float amax0 = L2 ? 0.f : 1.f;                                                                                      \
    const F6Bases fb = f6_bases(lw);                                                                                             \
    h8 ah[4], nh[4];                                                                                                             \
    uint32_t hp[16];                                                                                                             \
    float res[32], xl[16];                                                                                                       \
    float amax = amax0;                                                                                                          \
    _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) nh[mt] = f6_hi(lds, fb, L2, 0, mt);                                         \
    _Pragma("unroll") for (int step = 0; step < KH; ++step) {                                                                    \
      float xs[8];                                                                                                               \
      SRC(step, xs);                                                                                                             \
      int mmask = L2 ? 0xff : 0;                                                                                                 \
      _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                                            \
        if (!L2 && step >= 8) xl[(step - 8) * 8 + e] = xs[e];                                                                    \
        if (!L2 && layer1_unbounded(step * 8 + e)) mmask |= 1 << e;                                                              \
      }                                                                                                                          \
      const int sg = step & 3;                                                                                                   \
      const h8 bh = split8_f6(xs, hp + 4 * sg, res + 8 * sg, amax, mmask);                                                       \
      _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) ah[mt] = nh[mt];                                                          \
      if (step + 1 < KH) {                                                                                                       \
        _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) nh[mt] = f6_hi(lds, fb, L2, step + 1, mt);                              \
      }                                                                                                                          \
      _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) ACC[mt] = MFMAH(ah[mt], bh, ACC[mt]);                                      \
      if (sg == 3) {                                                                                                             \
        const B6 b6 = group6(hp, res, amax);                                                                                     \
        group_mfma6(lds, fb, L2, step >> 2, b6, ACC);                                                                            \
        amax = amax0;                                                                                                            \
      } else if (!L2 && step == KH - 1) {                                                                                        \
        const B6 b6 = group6_half(xl, res, amax);                                                                                \
        group_mfma6(lds, fb, L2, G6_1 - 1, b6, ACC);                                                                             \
      }                                                                                                                          \
    }                                                                                                                            \
  }

// training forward: a layer's output (after the ReLU) as KH2 k-steps of the next layer, [tile][k-step][lane][8 halves], plus the
// ReLU masks as bits: what the shade backward needs of h1 / h2 (it would otherwise re-read both dumps, 1 KB per sample).
// Layer 1's accumulators arrive rectified, layer 2's do not.
#define EGO_DUMP_HIDDEN(LAYER, ACC, DUMP_H)                                                                                      \
  {                                                                                                                              \
    _Pragma("unroll") for (int st = 0; st < KH2; ++st) { /* k-step st of the next layer = registers 8 (st & 1) .. + 7 of m-tile st >> 1 */ \
      float v8[8];                                                                                                               \
      _Pragma("unroll") for (int e = 0; e < 8; ++e) v8[e] = (LAYER) == 1 ? ACC[st >> 1][8 * (st & 1) + e] : relu_f(ACC[st >> 1][8 * (st & 1) + e]); \
      __builtin_nontemporal_store(pack8_rn(v8), &((u32x4*)(DUMP_H))[(tile * KH2 + st) * 64 + lane]);                            \
    }                                                                                                                            \
    __builtin_nontemporal_store(relu_bits(ACC), &((u32x2*)A.dump_bits)[(tile * 2 + ((LAYER) - 1)) * 64 + lane]);                \
  }

struct BasisFrag {

  h8 hi, lo;
};

template <int STEP>
__device__ __forceinline__ BasisFrag basis_frag(const u32x4* __restrict__ BASH, int lane, int gsel) {
  BasisFrag f;
  f.hi = __builtin_bit_cast(h8, BASH[((gsel * KHB + STEP) * 2 + 0) * 64 + lane]);
  f.lo = __builtin_bit_cast(h8, BASH[((gsel * KHB + STEP) * 2 + 1) * 64 + lane]);
  return f;
}

__device__ __forceinline__ void basis_step(const BasisFrag& a, const float x[8], bool keep, f32x16& fe) {
  const HL b = split8(x, keep);
  fe = MFMAH(a.hi, b.hi, fe);
  fe = MFMAH(a.lo, b.hi, fe);
  fe = MFMAH(a.hi, b.lo, fe);
}

// ---- 4-lane-team gather (fp32 tables, f16x3 kernel) ------------------------------------------------------------------
// The vector L1 looks up one distinct 64-byte line per cycle, and with two lanes per sample a load instruction touches
// ~26 distinct lines (PMC: 3270 tag lookups per tile), which - not bytes - bounds the gather.  Here the wave gathers as 16
// teams of 4 lanes, lane = 32*pa + 2*t + pb: team t = the lane pairs (2t, 2t+1) and (2t+32, 2t+33).  In round rd the team
// serves the tile's sample 2t + rd and its lane reads quad pa + 2*(pb ^ rd) of each line, so a team reads a whole line per
// instruction and an instruction touches <= 16 lines; two rounds cover the 32 samples.  The MFMA layout is lane = 32*h + j
// (sample j, half h = pa holds quads h and h + 2, K order app_channel_g): a lane's own sample is 2t + pb, so it keeps the
// round that served it (quad h) and gets quad h + 2 of its sample from the lane next to it: two selects and one neighbour
// exchange per value.
// The exchange is a v_mov_b32_dpp quad_perm (__shfl_xor and ds_swizzle forms were measured in round 1 and removed: DESIGN.md 5.1).
// REPRODUCIBILITY: kernels of this family (fp32-table gather of the f16x3 kernel) have a build-dependent fault that is not
// understood: in affected builds 0.3 % ... 100 % of the calls return one gather round's products wrong in lanes
// 16-31 and 48-63 of a wave in slots 4-7 of its workgroup (the second wave of a SIMD).  It does not depend on the exchange (it also
// hits EGO_GATHER_TEAMS 0, where no lane talks to another), needs two waves co-running on the SIMD, and none of the stand-alone
// probes in tools/ reproduces it.  Builds of this file WITHOUT the SLP vectoriser (egonerf_amd/build.py) have been clean in every
// soak (> 300 000 calls, all exchange forms tried); with it, only the __shfl_xor form happened to be.  tools/flaky_probe*.py,
// tools/variant_test.sh and tests/test_hip_determinism.py are the guards: re-run them after ANY change to this file.

struct TeamSample {  // normalised coordinates of the sample this lane's team serves in one round
  float a_r, a_th, a_ph;
  int g;
};

template <int I>
__device__ __forceinline__ void team_load(const DevField& F, const VMTaps& t, int g, int q, f32x4 raw[18]) {
  const Lin1 X = t.ax[vm_plane_x(I)], Y = t.ax[vm_plane_y(I)], Ln = t.ax[vm_line_ax(I)];
  const int W = F.res[vm_plane_x(I)];
  // compact addressing (DevField): one scalar base + a 32-bit byte offset per tap; quad 4i + q is 64 i bytes further on
  const uint32_t pb = (g ? F.poff[1][I] : F.poff[0][I]) + 16u * (uint32_t)q;
  const uint32_t lb = (g ? F.loff[1][I] : F.loff[0][I]) + 16u * (uint32_t)q;
  const uint32_t r0 = pb + (uint32_t)(Y.i0 * W) * (APP_C * 4), r1 = pb + (uint32_t)(Y.i1 * W) * (APP_C * 4);
  const uint32_t c0 = (uint32_t)X.i0 * (APP_C * 4), c1 = (uint32_t)X.i1 * (APP_C * 4);
  const char* p00 = F.base + (r0 + c0);
  const char* p01 = F.base + (r0 + c1);
  const char* p10 = F.base + (r1 + c0);
  const char* p11 = F.base + (r1 + c1);
  const char* l0 = F.base + (lb + (uint32_t)Ln.i0 * (APP_C * 4));
  const char* l1 = F.base + (lb + (uint32_t)Ln.i1 * (APP_C * 4));
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    raw[i] = *(const f32x4*)(p00 + 64 * i); raw[3 + i] = *(const f32x4*)(p01 + 64 * i); raw[6 + i] = *(const f32x4*)(p10 + 64 * i);
    raw[9 + i] = *(const f32x4*)(p11 + 64 * i); raw[12 + i] = *(const f32x4*)(l0 + 64 * i); raw[15 + i] = *(const f32x4*)(l1 + 64 * i);
  }
}

template <int I>
__device__ __forceinline__ void team_finish(const VMTaps& t, const f32x4 raw[18], float out[12]) {
#pragma clang fp contract(fast)
  const Lin1 X = t.ax[vm_plane_x(I)], Y = t.ax[vm_plane_y(I)], Ln = t.ax[vm_line_ax(I)];
  float w00 = __fmul_rn(Y.w0, X.w0), w01 = __fmul_rn(Y.w0, X.w1);
  float w10 = __fmul_rn(Y.w1, X.w0), w11 = __fmul_rn(Y.w1, X.w1);
  float l0 = Ln.w0, l1 = Ln.w1;
#ifndef EGO_PAIRED_WEIGHTS
  // Every weight in a register of its own: a packed multiply then broadcasts the LOW half of its pair operand
  // (op_sel_hi:[1,0]).  If the compiler vectorises the four products above into {w00, w01} / {w10, w11} pairs, the packed ops
  // that consume w01 / w11 broadcast the HIGH half (op_sel:[1,0,0]) - and every build of these kernels that contained such
  // instructions was non-reproducible, every build without them clean.  tests/test_abi_and_host.py checks the ISA.
  asm volatile("" : "+v"(w00)); asm volatile("" : "+v"(w01)); asm volatile("" : "+v"(w10)); asm volatile("" : "+v"(w11));
  asm volatile("" : "+v"(l0)); asm volatile("" : "+v"(l1));
#endif
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const f32x4 pv = raw[i] * w00 + raw[3 + i] * w01 + raw[6 + i] * w10 + raw[9 + i] * w11;
    const f32x4 lv = raw[12 + i] * l0 + raw[15 + i] * l1;
    const f32x4 m = pv * lv;
    out[4 * i + 0] = m.x; out[4 * i + 1] = m.y; out[4 * i + 2] = m.z; out[4 * i + 3] = m.w;
  }
}

// ---- rolling form of the same gather (gather_basis_team<ROLL = true>): the 18-register load buffer is recycled line by line -----
// A round's 18 loads are three lines of six taps.  Instead of "issue 18, wait, compute 12 products, issue the next 18", the six
// registers of a line are refilled with the NEXT round's loads as soon as that line's four products are computed, so 12-18 loads
// stay in flight all the time instead of the queue draining once per round (the gather is latency-bound, not issue-bound).
struct TapPtrs {
  uint32_t p00, p01, p10, p11, l0, l1;   // byte offsets from DevField::base (compact addressing: half the registers of pointers)
  float w00, w01, w10, w11, wl0, wl1;
};

template <int I>
__device__ __forceinline__ TapPtrs tap_ptrs(const DevField& F, const VMTaps& t, int g, int q) {
  const Lin1 X = t.ax[vm_plane_x(I)], Y = t.ax[vm_plane_y(I)], Ln = t.ax[vm_line_ax(I)];
  const int W = F.res[vm_plane_x(I)];
  const uint32_t pb = (g ? F.poff[1][I] : F.poff[0][I]) + 16u * (uint32_t)q;
  const uint32_t lb = (g ? F.loff[1][I] : F.loff[0][I]) + 16u * (uint32_t)q;
  const uint32_t r0 = pb + (uint32_t)(Y.i0 * W) * (APP_C * 4), r1 = pb + (uint32_t)(Y.i1 * W) * (APP_C * 4);
  const uint32_t c0 = (uint32_t)X.i0 * (APP_C * 4), c1 = (uint32_t)X.i1 * (APP_C * 4);
  TapPtrs tp;
  tp.p00 = r0 + c0; tp.p01 = r0 + c1; tp.p10 = r1 + c0; tp.p11 = r1 + c1;
  tp.l0 = lb + (uint32_t)Ln.i0 * (APP_C * 4);
  tp.l1 = lb + (uint32_t)Ln.i1 * (APP_C * 4);
  tp.w00 = __fmul_rn(Y.w0, X.w0); tp.w01 = __fmul_rn(Y.w0, X.w1);
  tp.w10 = __fmul_rn(Y.w1, X.w0); tp.w11 = __fmul_rn(Y.w1, X.w1);
  tp.wl0 = Ln.w0; tp.wl1 = Ln.w1;
  // separate registers for the weights: see team_finish
  asm volatile("" : "+v"(tp.w00)); asm volatile("" : "+v"(tp.w01)); asm volatile("" : "+v"(tp.w10)); asm volatile("" : "+v"(tp.w11));
  asm volatile("" : "+v"(tp.wl0)); asm volatile("" : "+v"(tp.wl1));
  return tp;
}

__device__ __forceinline__ void line_load(const DevField& F, const TapPtrs& tp, int i, f32x4 r[6]) {
  const char* b = F.base + 64 * i;
  r[0] = *(const f32x4*)(b + tp.p00); r[1] = *(const f32x4*)(b + tp.p01); r[2] = *(const f32x4*)(b + tp.p10);
  r[3] = *(const f32x4*)(b + tp.p11); r[4] = *(const f32x4*)(b + tp.l0); r[5] = *(const f32x4*)(b + tp.l1);
}

__device__ __forceinline__ void line_finish(const TapPtrs& tp, const f32x4 r[6], float out[4]) {
#pragma clang fp contract(fast)
  const f32x4 pv = r[0] * tp.w00 + r[1] * tp.w01 + r[2] * tp.w10 + r[3] * tp.w11;
  const f32x4 lv = r[4] * tp.wl0 + r[5] * tp.wl1;
  const f32x4 m = pv * lv;
  out[0] = m.x; out[1] = m.y; out[2] = m.z; out[3] = m.w;
}

// ga = this lane's quad of the sample served in round 0 (tile column 2t), gb = of round 1 (column 2t + 1).  Even lanes own
// column 2t: they keep ga (quad h) and take the odd neighbour's ga (quad h + 2); odd lanes keep gb and take the even
// neighbour's gb.  v[0..11] = quad h, v[12..23] = quad h + 2 of the lane's own sample.
__device__ __forceinline__ void team_to_halves(const float ga[12], const float gb[12], float* v) {
  if (!EGO_GATHER_TEAMS) {
#pragma unroll
    for (int idx = 0; idx < 12; ++idx) { v[idx] = ga[idx]; v[12 + idx] = gb[idx]; }
    return;
  }
  const bool even = (threadIdx.x & 1) == 0;
#pragma unroll
  for (int idx = 0; idx < 12; ++idx) {
    const float give = even ? gb[idx] : ga[idx];
    v[idx] = even ? ga[idx] : gb[idx];
    v[12 + idx] = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(give), 0xB1 /* quad_perm [1,0,3,2] */, 0xf, 0xf, false));
  }
}

// (v as halves - 0.6 GB less per step each way, forward -0.12 ms - puts the basis gradient of the 1.5 k-sample golden at 2.3e-4 of its
// largest element against the 2e-4 it is held to: v stays fp32)
// All dump stores of the training FORWARD are NONTEMPORAL (`global_store ... nt`): 2.6 GB per launch that nobody reads before the whole pass
// is over (the backward's dh2 / dh1 are read by the next kernels and stay cached; its dfe / dv are written as quarter lines).  Measured (round 5, timing-only builds, one box): forward without its dump stores 0.49 ms, with them 0.94, with the
// stores aimed at a per-wave 40 KB region (no HBM traffic at all) 0.74 - the write path into the XCD's L2 (~17 B / clk / CU, half the read
// rate), not HBM and not the order of loads and stores in the vmcnt queue (moving the stores behind the next loads: +-0), is what a dumping
// wave waits for; nt stores take the forward to 0.79-0.82 ms.
__device__ __forceinline__ void dump24(float* dst, const float* v) {
  if (dst) {
#pragma unroll
    for (int q = 0; q < 6; ++q) __builtin_nontemporal_store(f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]}, &((f32x4*)dst)[64 * q]);  // quad pairs 256 floats apart
  }
}

// whole gather + basis for one tile; ts[rd] = the sample this lane's team serves in round rd.  All 64 lanes must call
// (cross-lane swaps).
// one basis k-step of 8 products: split once, three MFMAs with the wave's grid (g0) and - only in a wave that straddles the yin /
// yang border - three more with the other grid's fragments into the second accumulator (the split is shared: re-splitting in the
// rare branch made the compiler hoist 72 fp16 -> fp32 conversions per tile onto the common path)
template <int STEP>
__device__ __forceinline__ void basis_step2(const u32x4* __restrict__ BASH, int lane, const BasisFrag& a, bool mixed, const float x[8],
                                            f32x16& fe, f32x16& fe2) {
  const HL b = split8(x, true);
  fe = MFMAH(a.hi, b.hi, fe);
  fe = MFMAH(a.lo, b.hi, fe);
  fe = MFMAH(a.hi, b.lo, fe);
  if (mixed) {  // wave-uniform
    const BasisFrag a1 = basis_frag<STEP>(BASH, lane, 1);
    fe2 = MFMAH(a1.hi, b.hi, fe2);
    fe2 = MFMAH(a1.lo, b.hi, fe2);
    fe2 = MFMAH(a1.hi, b.lo, fe2);
  }
}

// the same with the wave's three fragment pairs already loaded (see EGO_ROLL_PLANE)
template <int STEP0>
__device__ __forceinline__ void basis3_pre(const u32x4* __restrict__ BASH, int lane, const BasisFrag& f0, const BasisFrag& f1, const BasisFrag& f2,
                                           bool mixed, const float* v, f32x16& fe, f32x16& fe2) {
  basis_step2<STEP0>(BASH, lane, f0, mixed, v, fe, fe2);
  basis_step2<STEP0 + 1>(BASH, lane, f1, mixed, v + 8, fe, fe2);
  basis_step2<STEP0 + 2>(BASH, lane, f2, mixed, v + 16, fe, fe2);
}

template <int STEP0>
__device__ __forceinline__ void basis3(const u32x4* __restrict__ BASH, int lane, int g0, bool mixed, const float* v, f32x16& fe, f32x16& fe2) {
  const BasisFrag f0 = basis_frag<STEP0>(BASH, lane, g0), f1 = basis_frag<STEP0 + 1>(BASH, lane, g0), f2 = basis_frag<STEP0 + 2>(BASH, lane, g0);
  basis_step2<STEP0>(BASH, lane, f0, mixed, v, fe, fe2);
  basis_step2<STEP0 + 1>(BASH, lane, f1, mixed, v + 8, fe, fe2);
  basis_step2<STEP0 + 2>(BASH, lane, f2, mixed, v + 16, fe, fe2);
}

// ROLL: the rolling form of the load buffer (tap_ptrs / line_load / line_finish above); it needs all 256 registers, so only the
// fused inference kernel uses it (the dumping and stand-alone instantiations would spill)
template <bool ROLL, int HN = 0>
__device__ __forceinline__ void gather_basis_team(const DevField& F, const TeamSample ts[2], const u32x4* __restrict__ BASH, int lane,
                                                  int g, bool mixed, int gu, f32x16& fe, float* vdump) {
  // EGO_GATHER_TEAMS 1: 4-lane teams (above).  0: no teams - both rounds serve the lane's OWN sample (ts[0] == ts[1]), round 0
  // reads quad h and round 1 quad h + 2, nothing is exchanged between lanes; an instruction then touches 32 lines instead of 16.
  const int qa = EGO_GATHER_TEAMS ? (lane >> 5) + 2 * (lane & 1) : (lane >> 5);
  const int qb = EGO_GATHER_TEAMS ? (lane >> 5) + 2 * ((lane & 1) ^ 1) : (lane >> 5) + 2;
  // A lane's output column depends only on its own inputs, so a wave that straddles the yin/yang border (rare) runs the
  // steps with both weight sets on the unmasked products, into two accumulators, and each lane keeps its grid's one at the
  // end: no per-value masking anywhere, and nothing extra for the waves of one grid.
  const int g0 = mixed ? 0 : gu;
  f32x16 fe2;
#pragma unroll
  for (int r = 0; r < 16; ++r) fe2[r] = 0.f;
  const VMTaps tA = vm_setup(ts[0].a_r, ts[0].a_th, ts[0].a_ph, F.res), tB = vm_setup(ts[1].a_r, ts[1].a_th, ts[1].a_ph, F.res);
  // one 18-load buffer in flight (72 VGPRs); the next plane's first round is issued right before the MFMAs of the
  // previous plane so that they overlap; the co-resident wave and the MLP phase hide the rest
  f32x4 raw[18];
  float ga[12], gb[12], v[24];
  if (ROLL) {
    f32x4 (*ln)[6] = (f32x4 (*)[6])raw;  // three lines of six taps
    TapPtrs pa = tap_ptrs<0>(F, tA, ts[0].g, qa), pb = tap_ptrs<0>(F, tB, ts[1].g, qb);
#pragma unroll
    for (int i = 0; i < 3; ++i) line_load(F, pa, i, ln[i]);
#define EGO_ROLL_PLANE(PL, NEXT_A, STEP0, DUMPPTR)                                                        \
    {                                                                                                     \
      _Pragma("unroll") for (int i = 0; i < 3; ++i) {                                                     \
        line_finish(pa, ln[i], ga + 4 * i);                                                               \
        line_load(F, pb, i, ln[i]);                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                \
      }                                                                                                   \
      NEXT_A;                                                                                             \
      /* the plane's basis fragments BEFORE the next plane's tap loads: vmcnt retires in order, so fragments loaded behind them */ \
      /* would make the first basis MFMA wait for all 18 taps of the next plane */                        \
      BasisFrag bf0, bf1, bf2;                                                                            \
      if (HN >= 1) bf0 = basis_frag<STEP0>(BASH, lane, g0);                                               \
      if (HN >= 2) bf1 = basis_frag<STEP0 + 1>(BASH, lane, g0);                                           \
      if (HN >= 3) bf2 = basis_frag<STEP0 + 2>(BASH, lane, g0);                                           \
      __builtin_amdgcn_sched_barrier(0);                                                                  \
      _Pragma("unroll") for (int i = 0; i < 3; ++i) {                                                     \
        line_finish(pb, ln[i], gb + 4 * i);                                                               \
        if (PL < 2) line_load(F, pa, i, ln[i]);                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                \
      }                                                                                                   \
      team_to_halves(ga, gb, v);                                                                          \
      dump24(DUMPPTR, v);                                                                                 \
      if (HN < 1) bf0 = basis_frag<STEP0>(BASH, lane, g0);                                                \
      if (HN < 2) bf1 = basis_frag<STEP0 + 1>(BASH, lane, g0);                                            \
      if (HN < 3) bf2 = basis_frag<STEP0 + 2>(BASH, lane, g0);                                            \
      basis3_pre<STEP0>(BASH, lane, bf0, bf1, bf2, mixed, v, fe, fe2);                                    \
    }
    EGO_ROLL_PLANE(0, pa = tap_ptrs<1>(F, tA, ts[0].g, qa), 0, vdump)
    pb = tap_ptrs<1>(F, tB, ts[1].g, qb);
    EGO_ROLL_PLANE(1, pa = tap_ptrs<2>(F, tA, ts[0].g, qa), 3, (vdump ? vdump + 6 * 256 : nullptr))
    pb = tap_ptrs<2>(F, tB, ts[1].g, qb);
    EGO_ROLL_PLANE(2, (void)0, 6, (vdump ? vdump + 12 * 256 : nullptr))
#undef EGO_ROLL_PLANE
    if (mixed) {
#pragma unroll
      for (int r = 0; r < 16; ++r) fe[r] = g ? fe2[r] : fe[r];
    }
    return;
  }
  team_load<0>(F, tA, ts[0].g, qa, raw);
  team_finish<0>(tA, raw, ga);
  __builtin_amdgcn_sched_barrier(0);
  team_load<0>(F, tB, ts[1].g, qb, raw);
  team_finish<0>(tB, raw, gb);
  team_to_halves(ga, gb, v);
  dump24(vdump, v);
  __builtin_amdgcn_sched_barrier(0);
  team_load<1>(F, tA, ts[0].g, qa, raw);
  basis3<0>(BASH, lane, g0, mixed, v, fe, fe2);
  team_finish<1>(tA, raw, ga);
  __builtin_amdgcn_sched_barrier(0);
  team_load<1>(F, tB, ts[1].g, qb, raw);
  team_finish<1>(tB, raw, gb);
  team_to_halves(ga, gb, v);
  dump24(vdump ? vdump + 6 * 256 : nullptr, v);
  __builtin_amdgcn_sched_barrier(0);
  team_load<2>(F, tA, ts[0].g, qa, raw);
  basis3<3>(BASH, lane, g0, mixed, v, fe, fe2);
  team_finish<2>(tA, raw, ga);
  __builtin_amdgcn_sched_barrier(0);
  team_load<2>(F, tB, ts[1].g, qb, raw);
  team_finish<2>(tB, raw, gb);
  team_to_halves(ga, gb, v);
  dump24(vdump ? vdump + 12 * 256 : nullptr, v);
  basis3<6>(BASH, lane, g0, mixed, v, fe, fe2);
  if (mixed) {
#pragma unroll
    for (int r = 0; r < 16; ++r) fe[r] = g ? fe2[r] : fe[r];
  }
}

// ---- half-precision appearance tables (ego_scene.app_f16) --------------------------------------------------------
// Same [H][W][48] channel-last layout with IEEE half elements (96 B per texel).  Lane half h owns the 16-byte chunks
// 2i+h (8 channels each), so one plane is 18 loads per lane and yields 24 products: one plane per pipeline stage, three
// stages per tile instead of six — the gather is bound by bytes in flight per VGPR, and a VGPR now carries two values.
// Interpolation and everything downstream stay fp32.
__host__ __device__ constexpr int app_channel_f16(int kk, int h) {
  return (kk / APP_HALF) * APP_C + ((kk % APP_HALF) / 8) * 16 + 8 * h + (kk % 8);
}

template <int I>
__device__ __forceinline__ void gather_plane_f16(const DevField& F, const VMTaps& t, int g, int h, float v[APP_HALF]) {
#pragma clang fp contract(fast)
  const Lin1 X = t.ax[vm_plane_x(I)], Y = t.ax[vm_plane_y(I)], Ln = t.ax[vm_line_ax(I)];
  const int W = F.res[vm_plane_x(I)];
  // element offsets are in halves; the DevField pointers are nominally float*
  const _Float16* P = (const _Float16*)(g ? F.plane[1][I] : F.plane[0][I]) + 8 * h;
  const _Float16* L = (const _Float16*)(g ? F.line[1][I] : F.line[0][I]) + 8 * h;
  const h8* p00 = (const h8*)(P + (Y.i0 * W + X.i0) * APP_C);
  const h8* p01 = (const h8*)(P + (Y.i0 * W + X.i1) * APP_C);
  const h8* p10 = (const h8*)(P + (Y.i1 * W + X.i0) * APP_C);
  const h8* p11 = (const h8*)(P + (Y.i1 * W + X.i1) * APP_C);
  const h8* l0 = (const h8*)(L + Ln.i0 * APP_C);
  const h8* l1 = (const h8*)(L + Ln.i1 * APP_C);
  const float w00 = __fmul_rn(Y.w0, X.w0), w01 = __fmul_rn(Y.w0, X.w1);
  const float w10 = __fmul_rn(Y.w1, X.w0), w11 = __fmul_rn(Y.w1, X.w1);
#pragma unroll
  for (int c = 0; c < 3; ++c) {  // chunk 2c+h: h8 index 2c
    const h8 a00 = p00[2 * c], a01 = p01[2 * c], a10 = p10[2 * c], a11 = p11[2 * c], b0 = l0[2 * c], b1 = l1[2 * c];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float pv = (float)a00[e] * w00 + (float)a01[e] * w01 + (float)a10[e] * w10 + (float)a11[e] * w11;
      const float lv = (float)b0[e] * Ln.w0 + (float)b1[e] * Ln.w1;
      v[c * 8 + e] = pv * lv;
    }
  }
}

template <bool MASKED>
__device__ __forceinline__ void gather_basis_f16(const DevField& F, const VMTaps& taps, const u32x4* __restrict__ BASH, int lane,
                                                 int g, int h, int gsel, bool keep_in, f32x16& fe) {
  const bool keep = !MASKED || keep_in;
  float v0[APP_HALF], v1[APP_HALF], v2[APP_HALF];
  BasisFrag f0, f1, f2;
  gather_plane_f16<0>(F, taps, g, h, v0);
  f0 = basis_frag<0>(BASH, lane, gsel); f1 = basis_frag<1>(BASH, lane, gsel); f2 = basis_frag<2>(BASH, lane, gsel);
  __builtin_amdgcn_sched_barrier(0);
  gather_plane_f16<1>(F, taps, g, h, v1);
  basis_step(f0, v0, keep, fe); basis_step(f1, v0 + 8, keep, fe); basis_step(f2, v0 + 16, keep, fe);
  f0 = basis_frag<3>(BASH, lane, gsel); f1 = basis_frag<4>(BASH, lane, gsel); f2 = basis_frag<5>(BASH, lane, gsel);
  __builtin_amdgcn_sched_barrier(0);
  gather_plane_f16<2>(F, taps, g, h, v2);
  basis_step(f0, v1, keep, fe); basis_step(f1, v1 + 8, keep, fe); basis_step(f2, v1 + 16, keep, fe);
  f0 = basis_frag<6>(BASH, lane, gsel); f1 = basis_frag<7>(BASH, lane, gsel); f2 = basis_frag<8>(BASH, lane, gsel);
  __builtin_amdgcn_sched_barrier(0);
  basis_step(f0, v2, keep, fe); basis_step(f1, v2 + 8, keep, fe); basis_step(f2, v2 + 16, keep, fe);
}

// ---- dense gather (ego_scene.app_f16 = EGO_APP_DENSE): the 27 features as the trilinear interpolation of the baked node grid ------------------------
// A lane serves its OWN sample and lane half: per cell corner the half's 14 slots are three 16-byte quads and one 8-byte piece of the
// node (quad 2 q + h of its 128 bytes, csrc/ego_dense.hip), so the two lanes of a sample read the same 64-byte line in every load
// instruction.  The grid is chosen per lane by the sample's own flag: a wave that straddles the yin / yang border needs nothing special,
// and a lane's result depends on its own sample only.  Interpolation along r, then theta, then phi (the dense march's order), fp32,
// every weight in a register pair of its own (dense_weight).  The r pairs are reduced as they land: two pairs of loads in flight.
typedef float f32x2 __attribute__((ext_vector_type(2)));
struct DenseCorner {
  f32x4 a, b, c;
  f32x2 d;
};
__device__ __forceinline__ DenseCorner dense_corner(const char* __restrict__ G, uint32_t off) {
  DenseCorner n;
  n.a = *(const f32x4*)(G + off); n.b = *(const f32x4*)(G + off + 32); n.c = *(const f32x4*)(G + off + 64); n.d = *(const f32x2*)(G + off + 96);
  return n;
}
// a weight is a register PAIR holding it twice, opaque to the compiler: a packed multiply then reads the pair as it stands and
// broadcasts neither half (pinned scalars alone still came out as {w0, w1} pairs with a high-half broadcast in the
// MODE_APP instance)
__device__ __forceinline__ f32x2 dense_weight(float w) {
  f32x2 ww = {w, w};
  asm volatile("" : "+v"(ww));
  return ww;
}
__device__ __forceinline__ DenseCorner dense_lerp(const DenseCorner& x, const DenseCorner& y, f32x2 w0, f32x2 w1) {
  // fma(y, w1, x * w0), spelled out (the file is built with -ffp-contract=off): every instance rounds alike, which the bit equality
  // of the plain, folded and compact forms rests on
  const f32x4 w0q = __builtin_shufflevector(w0, w0, 0, 1, 0, 1), w1q = __builtin_shufflevector(w1, w1, 0, 1, 0, 1);
  DenseCorner n;
  n.a = __builtin_elementwise_fma(y.a, w1q, x.a * w0q); n.b = __builtin_elementwise_fma(y.b, w1q, x.b * w0q);
  n.c = __builtin_elementwise_fma(y.c, w1q, x.c * w0q); n.d = __builtin_elementwise_fma(y.d, w1, x.d * w0);
  return n;
}

__device__ __forceinline__ void gather_app_dense(const char* __restrict__ G, uint32_t grid_off, const int32_t res[3], const VMTaps& t, int h,
                                                 f32x16& fe) {
  const Lin1 &Rr = t.ax[0], &Tt = t.ax[1], &Pp = t.ax[2];
  const uint32_t nr128 = (uint32_t)res[0] * 128u, gb = grid_off + 16u * (uint32_t)h;
  const uint32_t row00 = gb + ((uint32_t)Pp.i0 * (uint32_t)res[1] + (uint32_t)Tt.i0) * nr128;
  const uint32_t row01 = gb + ((uint32_t)Pp.i0 * (uint32_t)res[1] + (uint32_t)Tt.i1) * nr128;
  const uint32_t row10 = gb + ((uint32_t)Pp.i1 * (uint32_t)res[1] + (uint32_t)Tt.i0) * nr128;
  const uint32_t row11 = gb + ((uint32_t)Pp.i1 * (uint32_t)res[1] + (uint32_t)Tt.i1) * nr128;
  const uint32_t c0 = (uint32_t)Rr.i0 * 128u, c1 = (uint32_t)Rr.i1 * 128u;
  const f32x2 w6[6] = {dense_weight(Rr.w0), dense_weight(Rr.w1), dense_weight(Tt.w0), dense_weight(Tt.w1), dense_weight(Pp.w0), dense_weight(Pp.w1)};
  DenseCorner p0 = dense_corner(G, row00 + c0), p1 = dense_corner(G, row00 + c1);
  DenseCorner q0 = dense_corner(G, row01 + c0), q1 = dense_corner(G, row01 + c1);
  __builtin_amdgcn_sched_barrier(0);
  const DenseCorner v00 = dense_lerp(p0, p1, w6[0], w6[1]);
  p0 = dense_corner(G, row10 + c0); p1 = dense_corner(G, row10 + c1);
  __builtin_amdgcn_sched_barrier(0);
  const DenseCorner v01 = dense_lerp(q0, q1, w6[0], w6[1]);
  q0 = dense_corner(G, row11 + c0); q1 = dense_corner(G, row11 + c1);
  const DenseCorner u0 = dense_lerp(v00, v01, w6[2], w6[3]);
  __builtin_amdgcn_sched_barrier(0);
  const DenseCorner v10 = dense_lerp(p0, p1, w6[0], w6[1]);
  const DenseCorner v11 = dense_lerp(q0, q1, w6[0], w6[1]);
  const DenseCorner u1 = dense_lerp(v10, v11, w6[2], w6[3]);
  const DenseCorner d = dense_lerp(u0, u1, w6[4], w6[5]);
  fe[0] = d.a.x; fe[1] = d.a.y; fe[2] = d.a.z; fe[3] = d.a.w; fe[4] = d.b.x; fe[5] = d.b.y; fe[6] = d.b.z; fe[7] = d.b.w;
  fe[8] = d.c.x; fe[9] = d.c.y; fe[10] = d.c.z; fe[11] = d.c.w; fe[12] = d.d.x; fe[13] = d.d.y; fe[14] = 0.f; fe[15] = 0.f;
}

// PX: arithmetic of the MLP's correction terms: 0 = fp16 (f16x3), 1 = fp8 (f16f8), 2 = fp6 (f16f6)
// FOLD: rows H / J in the epilogue (models/EgoNeRF.py:579-598): a wave owns whole rays (S a multiple of 32, a ray = S / 32 consecutive
// tiles), keeps sum w r, w b, w (lane half 0) and sum w g, w z (lane half 1) per lane across the ray's tiles and finishes the pixel -
// background, clamp, depth - itself; no per-sample colours are written and k_composite (12 us per 4096 x 512 launch: 25 MB of colours
// written here, 42 MB read there) is not launched.
// COMPACT: the tiles are cut from the live-sample list (ego_shade_live) instead of the flat [N][S] order: lane j of tile t shades sample
// live[32 t + j], reads its coordinates at that index and its direction from ray live[..] / S, and writes its colour there.  Every lane's
// result depends on its own sample only, so the colours are the bits the tile walk writes for the same samples.
// DAPP: the features come from the baked node grid (gather_app_dense) instead of the tables and the basis; inference without dumps
// and with fp32 tables only (MODE_SHADE in its three forms, and MODE_APP so that the features can be checked on their own).  Then A.F
// describes the node grid, not the tables: F.base = the grid, F.poff[g][0] = the byte offset of grid g in it, F.res = its resolution.
// MARCH (the three FOLD + DAPP instances; ego_render_forward's one-launch eval render): ahead of its first tile a wave marches the rays
// it is about to shade - march_wave_rays (ego_march.h), k_march_density's dense one-wave form on MARCH passes side by side - into the
// workspace slots that kernel fills, and the tile loop reads them through A.z / A.comp_w / A.coords as it reads that kernel's output.
// The march's argument block is a kernel parameter of its own that only a marching instance has (MB: a grown ShadeArgs moves literals
// in every instance); it is read through an opaque address inside the march, so that nothing of it can become an invariant of the tile
// loop.  That address is `kernel-argument segment + sizeof(ShadeArgs)`: it is the code-object ABI's layout (explicit arguments first, in
// declaration order, each at its natural alignment), so `mb` must stay the SECOND AND LAST explicit parameter, and a MarchBlock whose
// alignment sizeof(ShadeArgs) is no multiple of does not compile (static_assert below).
// A wave's tiles read what other lanes of the SAME wave stored: vmcnt(0) and a wavefront-scope release / acquire pair stand between; the
// stores and the tile loop's loads go through the CU's one write-through vector L1, which is coherent between the CU's waves (a sibling
// wave may have pulled in a line of tile flags before this wave stored its own).  The tile loop must read these buffers with vector loads.
struct MarchBlock {
  MarchArgs a;
  int32_t rays_per_wave;   // the folded deal: wave w of the grid owns rays [w * rays_per_wave, (w + 1) * rays_per_wave) below N
};

template <int MODE, bool DUMP = false, bool TAB16 = false, int PX = 0, bool FOLD = false, bool COMPACT = false, bool DAPP = false, int MARCH = 0,
          class... MB>
__global__ __launch_bounds__(512) void k_shade_h(ShadeArgs A, MB... mb) {
  constexpr bool P8 = PX == 1, P6 = PX == 2;
  static_assert(!MARCH || (FOLD && DAPP), "the in-wave march exists for the folded dense instances only");
  static_assert(sizeof...(MB) == (MARCH ? 1 : 0), "a marching instance takes the march's argument block, the others nothing");
  // RAY_VIEW: a folded wave's tiles are whole rays, so the dense instances encode the view direction once per ray and keep the lane
  // half's eight view slots across its tiles; their tile loop holds no division m / S, no load of the direction and no encoding of it.
  // The table instances have no registers for that (built: 6 / 19 VGPRs spilled in the f16x3 / f16f6 forms; with the direction as
  // scalars and the encoding per tile, 7 of 1780 VALU per tile) and keep the per-tile form.
  constexpr bool RAY_VIEW = FOLD && DAPP;
  static_assert(!DAPP || (MODE != MODE_MLP && !DUMP && !TAB16), "the dense gather replaces the fp32-table gather of inference only");
  static_assert(!FOLD || (MODE == MODE_SHADE && !DUMP), "compositing folds into the fused inference kernel only");
  static_assert(!COMPACT || (MODE == MODE_SHADE && !DUMP && !FOLD), "the live-sample list is an input of the two-launch inference shade only");
  static_assert(!PX || (!DUMP && MODE != MODE_APP), "the fp8 / fp6 correction arithmetic exists for the inference MLP only");
  __shared__ __attribute__((aligned(16))) float lds[(MODE == MODE_APP ? 0 : LDS_W_FLOATS) + 4];
  const float* blob = A.packed + PACKED_FLOATS;  // the f16x3 half of the packed blob
  if (MODE != MODE_APP) {
    const f32x4* src = (const f32x4*)blob;
    const f32x4* src8 = (const f32x4*)(A.packed + 2 * PACKED_FLOATS + BASIS16_FLOATS + (P6 ? F8_FLOATS : 0));  // f16f8 / f16f6 layout of W1 / W2
    // The 150 KB image goes to LDS by the loads themselves (global_load_lds_dwordx4: a wave instruction moves 1 KB, no VGPRs), and
    // nobody waits for it here: the first tile's gather + basis phase reads no LDS, so the workgroup meets at a barrier in front of
    // its first MLP phase instead (`need_sync` below).  A launch has ~32 us of fixed cost at 4096 x 512 (tools/shade_scaling.py), of
    // which the fill - every CU pulling the same 150 KB through its L1 with all waves parked - was the largest piece.
    constexpr int NQ = LDS_W_FLOATS / 4, NCH = NQ / 64;   // float4 quads; whole 1 KB chunks (the image ends 1 quad behind them)
    static_assert(F8_FLOATS % 256 == 0 && NQ - NCH * 64 < 64, "chunking of the LDS image");
    const int wv_u = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int c = wv_u; c < NCH; c += 8) {
      const f32x4* from = ((PX && c < F8_FLOATS / 256) ? src8 : src) + c * 64 + (threadIdx.x & 63);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)from, (__attribute__((address_space(3))) void*)(lds + c * 256), 16, 0, 0);
    }
    for (int i = NCH * 64 + threadIdx.x; i < NQ; i += 512) ((f32x4*)lds)[i] = src[i];
    if constexpr (MARCH) {
      // LUT and hints once per workgroup, in LDS next to the image, behind barriers of their own; then the wave's rays.  (The first
      // global load of either waits for the wave's share of the image, 19 KB: vmcnt retires in order.)
      static_assert(sizeof(ShadeArgs) % alignof(MarchBlock) == 0, "the march block follows ShadeArgs in the kernel-argument segment");
      static_assert(sizeof...(MB) == 1 && (std::is_same<MB, MarchBlock>::value && ...), "the march block is the kernel's second and last explicit parameter");
      uint64_t ka = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(ShadeArgs);
      asm volatile("" : "+s"(ka));
      const MarchBlock* mblock = (const MarchBlock*)(const __attribute__((address_space(4))) MarchBlock*)ka;
      __shared__ float march_lut[LUT_MAX];
      const MarchArgs& MA = mblock->a;
      const LutHints H = lut_hints(MA.c, march_lut);
      const int64_t ray0 = ((int64_t)blockIdx.x * 8 + wv_u) * mblock->rays_per_wave;
      const int64_t ray1 = ray0 + mblock->rays_per_wave < MA.N ? ray0 + mblock->rays_per_wave : MA.N;
      march_wave_rays<MARCH>(MA, march_lut, H, ray0, ray1, threadIdx.x & 63);
      __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): the march's stores have reached L2 ...
      wave_handover();                      // ... and no load of the tile loop is issued ahead of that
    }
  }
  bool need_sync = MODE != MODE_APP;   // wave-uniform: the barrier that publishes the LDS image is still ahead
  {
    // MODE.FP16_OVFL = 1: an out-of-range f32 -> fp8 / f16 conversion saturates to the largest finite value instead of producing
    // NaN / inf (v_cvt_pk_fp8_f32 returns NaN above 448, tools/fp8_layout_probe.hip); a saturated correction operand costs accuracy
    // of one low-order term, a NaN would poison the pixel.  Round 5: for every arithmetic, not only the fp8 / fp6 ones - in the
    // three-term fp16 split hi = 65504 and lo = x - hi then carry a value up to twice the half range exactly (inf - inf was NaN), and
    // the training forward's x / h1 / h2 dumps (halves) stay finite.
    __builtin_amdgcn_s_setreg(1 | (23 << 6) | (0 << 11), 1);
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  // wave priority follows the phase: high while gathering (latency-bound: get the loads out), low in the MLP phase, whose MFMAs
  // fill the matrix pipe anyway - 0.9 % faster than the static priority of k_shade (no priority / static: measured, removed)
  // (DAPP: the count is read as a scalar, so that no vector copy of it can become a loop invariant for the MLP phase to spill)
  const int32_t n_live = COMPACT ? (DAPP ? __builtin_amdgcn_readfirstlane(*A.n_live) : *A.n_live) : 0;
  const int64_t n_tiles = ((COMPACT ? (int64_t)n_live : A.M) + 31) >> 5;
  const u32x4* W1 = (const u32x4*)(lds + OFF_W1);
  const u32x4* W2 = (const u32x4*)(lds + OFF_W2);
  const f32x4* B1 = (const f32x4*)(lds + OFF_B1);
  const f32x4* B2 = (const f32x4*)(lds + OFF_B2);
  const f32x4* W3 = (const f32x4*)(lds + OFF_W3);
  // basis fragments: K order of the fp32-table gather, or of the fp16-table gather (third region of the blob)
  const u32x4* BASH = TAB16 ? (const u32x4*)(A.packed + 2 * PACKED_FLOATS) : (const u32x4*)(blob + OFF_BASIS);

  // Tile order: a wave walks a contiguous run of tiles, i.e. along its rays (the angular taps of the next tile are the lines this
  // wave's L1 just served: -1.5..2.3 % kernel time against tiles dealt round-robin over the grid, A/B on one box).  Skipped tiles
  // (tile mask) are the tails of rays and every wave owns whole rays; sharing the ACTIVE tiles evenly instead (prefix sums over the
  // mask in the prologue, or chunks dealt through an atomic counter) was built and measured: DESIGN.md 4.3.
  const int64_t n_wv = (int64_t)gridDim.x * 8;
  const int64_t tpr = FOLD ? (int64_t)(A.S >> 5) : 0;   // tiles per ray
  const int64_t rays_per_wave = FOLD ? (A.M / A.S + n_wv - 1) / n_wv : 0;
  const int64_t per_wave = FOLD ? rays_per_wave * tpr : (n_tiles + n_wv - 1) / n_wv;
  const int64_t tile0 = ((int64_t)blockIdx.x * 8 + wave) * per_wave;
  const int64_t tile1 = tile0 + per_wave < n_tiles ? tile0 + per_wave : n_tiles;
  const int64_t seg_len = FOLD ? tpr : per_wave;   // FOLD: one ray per segment
  int64_t fold_ray = ((int64_t)blockIdx.x * 8 + wave) * rays_per_wave;   // FOLD: the segment's ray, seg0 / tpr, counted instead of divided
  for (int64_t seg0 = tile0; seg0 < tile1; seg0 += seg_len, ++fold_ray) {
  const int64_t seg1 = seg0 + seg_len < tile1 ? seg0 + seg_len : tile1;
  float c0 = 0.f, c1 = 0.f, c2 = 0.f;   // FOLD, lane half 0: sum w r, w b, w; half 1: sum w g, w z
  // What a ray's tiles share is fetched and made once, at the top of the ray (so also for a ray whose first tiles, or all of them,
  // the tile mask skips), through a wave-uniform address: d_z for the depth quirk of the epilogue and, with RAY_VIEW, the lane half's
  // eight view slots - by the function and on the floats that the other forms use per tile, so the bits are theirs.
  float fold_dz = 0.f, fold_vw[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if constexpr (FOLD) {
    const float* R = A.rays + fold_ray * 6;
    fold_dz = R[5];
    if constexpr (RAY_VIEW) view_slots<EncHw>(R[3], R[4], fold_dz, h, fold_vw);
  }
  // the tile mask is read 64 tiles at a time (one byte per lane + ballot) and walked with find-first-set: a skipped tile costs no
  // memory round trip (a per-tile flag load sat on the critical path of every skipped tile)
  for (int64_t wbase = seg0; wbase < seg1; wbase += 64) {
    unsigned long long wmask;
    {
      const int64_t t = wbase + (int64_t)lane;
      const bool in = t < seg1;
      wmask = (MODE == MODE_SHADE && !COMPACT && A.tile_active) ? __ballot(in && A.tile_active[in ? t : seg0] != 0) : __ballot(in);
    }
  while (wmask != 0ull) {
    const int64_t tile = wbase + (int64_t)__builtin_ctzll(wmask);
    wmask &= wmask - 1ull;
    int lw = lane;
    asm volatile("" : "+v"(lw));  // keeps the LDS weight reads inside the loop (see k_shade)
    if (MODE != MODE_MLP) __builtin_amdgcn_s_setprio(2);
    const int hw = lw >> 5;
    // DAPP: with the load buffer gone the gather phase leaves registers free, and the compiler fills them with lane-derived loop
    // invariants that the MLP phase then spills; taken from the opaque copy they are recomputed per tile (two VALU) instead
    const int jt = DAPP ? (lw & 31) : j, ht = DAPP ? hw : h;
    const int64_t m_raw = tile * 32 + jt;
    const bool valid = m_raw < (COMPACT ? (int64_t)n_live : A.M);
    // COMPACT: the list entry (a lane past the end repeats the last live sample and writes nothing)
    const int64_t m = COMPACT ? (int64_t)A.live[valid ? m_raw : n_live - 1] : valid ? m_raw : A.M - 1;
    // FOLD: the sample's weight and distance travel while the tile is computed (fetched where they are used, their latency is exposed once per tile)
    float fold_w = 0.f, fold_z = 0.f;
    if (FOLD) { fold_w = A.comp_w[m]; fold_z = A.z[m]; }

    f32x16 fe;
    float vd0 = 0.f, vd1 = 0.f, vd2 = 0.f;
    if (MODE == MODE_MLP) {
      const float* fp = A.feat + m * APP_DIM;
#pragma unroll
      for (int r = 0; r < 16; ++r) fe[r] = (r < NSLOT && 2 * r + h < APP_DIM) ? fp[min(2 * r + h, APP_DIM - 1)] : 0.f;
      vd0 = A.dirs[m * 3]; vd1 = A.dirs[m * 3 + 1]; vd2 = A.dirs[m * 3 + 2];
    } else {
      float a_r, a_th, a_ph;
      int g;
      if (MODE == MODE_APP) {
        const float* p = A.c7n + m * 7;
        g = (p[6] == 0.f) ? 0 : 1;
        const int b = g ? 3 : 0;
        a_r = p[b]; a_th = p[b + 1]; a_ph = p[b + 2];
      } else {
        if constexpr (!RAY_VIEW) {   // (RAY_VIEW: the ray is the segment's, its view slots are in fold_vw)
          int32_t s_div = A.S;
          if constexpr (DAPP) asm volatile("" : "+s"(s_div));   // (the reciprocal behind the division is such an invariant too)
          const uint32_t ray = (uint32_t)m / (uint32_t)s_div;
          const float* R = A.rays + (int64_t)ray * 6;
          vd0 = R[3]; vd1 = R[4]; vd2 = R[5];
        }
        // normalised coordinates come from ego_march_density (no acos/atan2/LUT search here)
        const f32x4 cc = ((const f32x4*)A.coords)[m];
        a_r = cc.x; a_th = cc.y; a_ph = cc.z; g = cc.w != 0.f;
      }
      const bool any_yin = __ballot(g == 0) != 0ull, any_yang = __ballot(g != 0) != 0ull;
      const bool mixed = any_yin && any_yang;
      const int gu = any_yin ? 0 : 1;
      VMTaps taps;
      if constexpr (DAPP) {   // ... and the same for the three axis scales (n - 1) / 2: the resolutions go through an opaque copy
        int32_t rs[3] = {A.F.res[0], A.F.res[1], A.F.res[2]};
        asm volatile("" : "+s"(rs[0]), "+s"(rs[1]), "+s"(rs[2]));
        taps = vm_setup(a_r, a_th, a_ph, rs);
      } else {
        taps = vm_setup(a_r, a_th, a_ph, A.F.res);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) fe[r] = 0.f;
      // per plane: two half-stages of 18 loads (12 products each); 3 basis k-steps of 8 products.  Loads of the
      // next half-stage are issued before the MFMAs of the previous one; sched_barriers bound the hoisting.
      // Waves whose 32 samples all lie in one grid (the common case) take the path without per-value masking.
      // lw / hw (opaque copies of lane / lane half) keep the per-table base pointers from being hoisted out of the tile
      // loop, where 24 64-bit loop invariants would spill.  Waves whose 32 samples all lie in one grid (the common case)
      // take the path without per-value masking; border-straddling waves run both weight sets masked.
      if (DAPP) {
        gather_app_dense(A.F.base, g ? A.F.poff[1][0] : A.F.poff[0][0], A.F.res, taps, hw, fe);
      } else if (TAB16) {
        if (!mixed) {
          gather_basis_f16<false>(A.F, taps, BASH, lw, g, hw, gu, true, fe);
        } else {
          gather_basis_f16<true>(A.F, taps, BASH, lw, g, hw, 0, g == 0, fe);
          gather_basis_f16<true>(A.F, taps, BASH, lw, g, hw, 1, g != 0, fe);
        }
      } else {
        // team gather: in round rd this lane's 4-lane team serves sample 2*((lane >> 1) & 15) + rd of the tile
        TeamSample ts[2];
#pragma unroll
        for (int rd = 0; rd < 2; ++rd) {
          const int64_t mt_raw = EGO_GATHER_TEAMS ? tile * 32 + 2 * ((lw >> 1) & 15) + rd : tile * 32 + (lw & 31);
          const int64_t mt = COMPACT ? (int64_t)A.live[mt_raw < n_live ? mt_raw : n_live - 1] : mt_raw < A.M ? mt_raw : A.M - 1;
          if (MODE == MODE_APP) {
            const float* p = A.c7n + mt * 7;
            ts[rd].g = (p[6] == 0.f) ? 0 : 1;
            const int b = ts[rd].g ? 3 : 0;
            ts[rd].a_r = p[b]; ts[rd].a_th = p[b + 1]; ts[rd].a_ph = p[b + 2];
          } else {
            const f32x4 c4 = ((const f32x4*)A.coords)[mt];
            ts[rd].a_r = c4.x; ts[rd].a_th = c4.y; ts[rd].a_ph = c4.z; ts[rd].g = c4.w != 0.f;
          }
        }
        float* vd = (DUMP && valid && A.dump_v) ? A.dump_v + dump_off(tile, 144, 0, hw, j) : nullptr;   // (v is optional since ABI v15: the sorted scatter can take d(basis) along)
        // one gather per tile; a border-straddling wave runs the basis steps of each plane twice (yin weights with the
        // yang lanes zeroed, then the reverse) inside gather_basis_team
        gather_basis_team<(MODE == MODE_SHADE && !DUMP), (FOLD ? EGO_HOIST_FOLD : EGO_HOIST_PLAIN)>(A.F, ts, BASH, lw, g, mixed, gu, fe, vd);
      }
    }

    if (MODE == MODE_APP) {
      if (valid) {
        float* o = A.out + m * APP_DIM;
#pragma unroll
        for (int r = 0; r < NSLOT; ++r)
          if (2 * r + ht < APP_DIM) o[2 * r + ht] = fe[r];
      }
      continue;
    }

    __builtin_amdgcn_s_setprio(0);
    if (need_sync) {
      // the LDS image was written by global_load_lds: its completion is counted by vmcnt, which the barrier's own release fence
      // (lgkmcnt) does not wait for.  Here the gather has already drained the counter, so the wait is free.
      __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0) (gfx9 encoding: vmcnt = bits 3:0 + 15:14, expcnt 7, lgkmcnt 15 = no wait)
      __syncthreads();
      need_sync = false;
    }
    if (DUMP && valid) {
#pragma unroll
      for (int q = 0; q < 4; ++q) __builtin_nontemporal_store(f32x4{fe[4 * q], fe[4 * q + 1], fe[4 * q + 2], fe[4 * q + 3]}, &((f32x4*)A.dump_fe)[(tile * 4 + q) * 64 + lane]);
    }
    float vw[8];
    if constexpr (RAY_VIEW) {
#pragma unroll
      for (int e = 0; e < 8; ++e) vw[e] = fold_vw[e];
    } else {
      view_slots<EncHw>(vd0, vd1, vd2, ht, vw);
    }

    // ---- layer 1 (10 steps of 8 values per lane half) ----------------------------------------------------------
    f32x16 H[4];
    EGO_LOAD_BIAS(B1, H)
    {
      float s1 = 0.f, c1 = 0.f, s2 = 0.f, c2 = 0.f;   // the encodings of the feature slot the generator stands in
      if (P8) EGO_MLP_LAYER_F8(1, W1, H, EGO_X_LAYER1)
      else if (P6) EGO_MLP_LAYER_F6(1, H, EGO_X_LAYER1)
      else EGO_MLP_LAYER_F16X3(1, W1, H, EGO_X_LAYER1)
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) H[mt][r] = relu_f(H[mt][r]);
    if (DUMP && valid) EGO_DUMP_HIDDEN(1, H, A.dump_h1)

    // ---- layer 2 (8 steps: registers of H), layer 3 on the VALU ------------------------------------------------
    f32x16 G[4];
    EGO_LOAD_BIAS(B2, G)
    if (P8) EGO_MLP_LAYER_F8(2, W2, G, EGO_X_LAYER2)
    else if (P6) EGO_MLP_LAYER_F6(2, G, EGO_X_LAYER2)
    else EGO_MLP_LAYER_F16X3(2, W2, G, EGO_X_LAYER2)
    if (DUMP && valid) EGO_DUMP_HIDDEN(2, G, A.dump_h2)
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      f32x4 w3[16];  // all 16 rows of this tile first: one LDS latency instead of 16 exposed round trips
#pragma unroll
      for (int r = 0; r < 16; ++r) w3[r] = W3[(mt * 2 + hw) * 16 + r];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float hv = relu_f(G[mt][r]);
        o0 = fmaf(hv, w3[r].x, o0); o1 = fmaf(hv, w3[r].y, o1); o2 = fmaf(hv, w3[r].z, o2);
      }
    }
    // A channel's logit is own + partner, in either lane of the pair.  Lane half 0 finishes red and blue, half 1 green: one exchange
    // carries what the partner finishes (half 1's o0, half 0's o1), one o2; two sigmoids per lane instead of three.
    float oa = ht ? o1 : o0;
    {
      const float give = ht ? o0 : o1;
      if constexpr (DAPP) {   // __shfl_xor(v, 32, 64) with the partner's index taken from the opaque lane copy (see jt / ht)
        const int partner = (lw ^ 32) << 2;
        oa += __int_as_float(__builtin_amdgcn_ds_bpermute(partner, __float_as_int(give)));
        o2 += __int_as_float(__builtin_amdgcn_ds_bpermute(partner, __float_as_int(o2)));
      } else {
        oa += __shfl_xor(give, 32, 64);
        o2 += __shfl_xor(o2, 32, 64);
      }
    }
    const float* b3 = lds + OFF_B3;
    const float ca = sigmoidf(oa + (ht ? b3[1] : b3[0])), cb = sigmoidf(o2 + b3[2]);   // half 0: red, blue; half 1: green, (blue)
    if (FOLD) {
      // weights are >= 0 and a tile skipped above holds only zeros (the fold is used with shade_above = 0), so nothing is conditional
      const float wgt = valid ? fold_w : 0.f;
      c0 += wgt * ca;
      c1 += wgt * (ht ? fold_z : cb);
      c2 += wgt;
    } else if (valid) {
      float* o = A.out + m * 3;
      if (ht == 0) { o[0] = ca; o[2] = cb; }
      else o[1] = ca;
    }
  }
  }
  if (FOLD) {   // the pixel of ray seg0 / tpr (rows H, J: k_composite's arithmetic on the per-lane sums)
    // sums over the 32 lanes of each half on the DPP path (no LDS round trips: the wave is alone with this chain at the end of a ray):
    // row_shr 1, 2, 4, 8 inside the 16-lane rows, then row_bcast:15 into rows 1 / 3: lane 31 holds half 0's sums, lane 63 half 1's
#define EGO_SUM_STEP(v, ctrl, rmask) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rmask, 0xf, false))
#define EGO_HALF_SUM(v) EGO_SUM_STEP(v, 0x111, 0xf); EGO_SUM_STEP(v, 0x112, 0xf); EGO_SUM_STEP(v, 0x114, 0xf); EGO_SUM_STEP(v, 0x118, 0xf); EGO_SUM_STEP(v, 0x142, 0xa)
    EGO_HALF_SUM(c0); EGO_HALF_SUM(c1); EGO_HALF_SUM(c2);
    // (the tree is the same in both halves, so lane 63's green is the sum lane 31 would have formed of the same per-lane values)
    const float green = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c0), 63));
    const float dp = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c1), 63));
#undef EGO_HALF_SUM
#undef EGO_SUM_STEP
    if (lane == 31) {
      const int64_t ray = fold_ray;
      const float* R = A.rays + ray * 6;
      float cr = c0, cg = green, cb = c1;
      const float c3 = c2;
      if (A.envmap) {
        float e[3];
        envmap_lookup(A.envmap, A.envmap_h, R[3], R[4], R[5], e);
        const float b = A.comp_bg[ray];
        const float bx = b * e[0], by = b * e[1], bz = b * e[2];
        cr += bx; cg += by; cb += bz;
        if (A.bg_map) { A.bg_map[ray * 3] = bx; A.bg_map[ray * 3 + 1] = by; A.bg_map[ray * 3 + 2] = bz; }
        if (A.env_map) { A.env_map[ray * 3] = e[0]; A.env_map[ray * 3 + 1] = e[1]; A.env_map[ray * 3 + 2] = e[2]; }
      }
      A.rgb_map[ray * 3] = fminf(fmaxf(cr, 0.f), 1.f);
      A.rgb_map[ray * 3 + 1] = fminf(fmaxf(cg, 0.f), 1.f);
      A.rgb_map[ray * 3 + 2] = fminf(fmaxf(cb, 0.f), 1.f);
      if (A.depth) A.depth[ray] = dp + (1.f - c3) * fold_dz;  // (1-acc) * d_z: reference quirk, EgoNeRF.py:598
    }
  }
  }
  if (need_sync) {   // a wave without a tile still owes the workgroup its arrival - and its DMA chunks, which must have LANDED first
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): global_load_lds completion is tracked by vmcnt, not by the barrier's lgkmcnt fence
    __syncthreads();
  }
}
#undef EGO_X_LAYER1
#undef EGO_X_LAYER2
#undef EGO_MLP_LAYER_F16X3
#undef EGO_MLP_LAYER_F8
#undef EGO_MLP_LAYER_F6
#undef EGO_DUMP_HIDDEN
#undef EGO_LOAD_BIAS

// ---- host side: one function fills the common launch arguments, one picks the kernel instance --------------------------------
ShadeArgs shade_args(const ego_scene* sc, int64_t M, int32_t S) {   // (the tables go in with the instance: launch_shade)
  ShadeArgs a{};
  a.c = make_coords(*sc); a.packed = sc->packed; a.M = M; a.S = S;
  return a;
}

// PX = 0 f16x3, 1 f16f8, 2 f16f6 where the MLP runs for inference (MLP, SHADE, SHADE + FOLD, SHADE + COMPACT), 0 elsewhere
// the marching form of the folded dense kernel (MARCH passes of a ray side by side); `mb` travels behind `a`
constexpr int MARCH_P = 2;
void launch_shade_march(int32_t precision, const ShadeArgs& a, const MarchBlock& mb, hipStream_t st) {
  const unsigned grid = shade_grid(a.M);
  if (precision == EGO_PREC_F16F8) return k_shade_h<MODE_SHADE, false, false, 1, true, false, true, MARCH_P, MarchBlock><<<grid, 512, 0, st>>>(a, mb);
  if (precision == EGO_PREC_F16F6) return k_shade_h<MODE_SHADE, false, false, 2, true, false, true, MARCH_P, MarchBlock><<<grid, 512, 0, st>>>(a, mb);
  k_shade_h<MODE_SHADE, false, false, 0, true, false, true, MARCH_P, MarchBlock><<<grid, 512, 0, st>>>(a, mb);
}

template <int MODE, bool DUMP, bool FOLD, bool COMPACT, bool TAB16, bool DAPP = false>
void launch_shade_h(int32_t precision, const ShadeArgs& a, hipStream_t st) {
  const unsigned grid = shade_grid(a.M);
  if constexpr (MODE != MODE_APP && !DUMP) {
    if (precision == EGO_PREC_F16F8) return k_shade_h<MODE, DUMP, TAB16, 1, FOLD, COMPACT, DAPP><<<grid, 512, 0, st>>>(a);
    if (precision == EGO_PREC_F16F6) return k_shade_h<MODE, DUMP, TAB16, 2, FOLD, COMPACT, DAPP><<<grid, 512, 0, st>>>(a);
  }
  k_shade_h<MODE, DUMP, TAB16, 0, FOLD, COMPACT, DAPP><<<grid, 512, 0, st>>>(a);
}

// the baked node grid (app_f16 = EGO_APP_DENSE: app16.plane[0][0]) as the field of a DAPP instance (see k_shade_h)
int dense_app_field(const ego_scene* sc, const char* who, DevField& F) {
  const float* grid = sc->app16.plane[0][0];
  if (!grid) return ego_fail(EGO_E_BADARG, "%s: app_f16 is EGO_APP_DENSE but app16.plane[0][0] (the node grid) is null", who);
  if (sc->app16.n_comp != APP_C || sc->app16.res[0] != sc->app.res[0] || sc->app16.res[1] != sc->app.res[1] || sc->app16.res[2] != sc->app.res[2])
    return ego_fail(EGO_E_BADARG, "%s: the dense appearance grid must be baked from 48 components at the resolution of `app`", who);
  const uint64_t grid_bytes = (uint64_t)sc->app.res[0] * (uint64_t)sc->app.res[1] * (uint64_t)sc->app.res[2] * 128u;
  if (((uintptr_t)grid & 15) != 0) return ego_fail(EGO_E_BADARG, "%s: the dense appearance grid must be 16-byte aligned", who);
  if (2 * grid_bytes >= ((uint64_t)1 << 32))
    return ego_fail(EGO_E_BADARG, "%s: the dense appearance grid must stay under 4 GB (32-bit byte offsets)", who);
  F.base = (const char*)grid;   // (see k_shade_h, DAPP)
  F.poff[0][0] = 0u; F.poff[1][0] = (uint32_t)grid_bytes;
  return EGO_OK;
}

// The set of shade instances: the entry point fixes MODE / DUMP / FOLD / COMPACT, the scene's mlp_precision and app_f16 pick the rest.
// k_shade (fp32 MFMA) and TAB16 (gather from the fp16 tables) exist where nothing is dumped or folded (their entry points refuse
// EGO_PREC_F32 / app_f16), TAB16 only where tables are read.  `who` names the entry point in error texts, `label` the launch.
template <int MODE, bool DUMP = false, bool FOLD = false, bool COMPACT = false>
int launch_shade(const ego_scene* sc, ShadeArgs& a, const char* who, const char* label, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  if (MODE != MODE_MLP) a.F = make_field(sc->app);
  if constexpr (!DUMP && !FOLD) {
    if (sc->mlp_precision == EGO_PREC_F32) {
      k_shade<MODE, COMPACT><<<shade_grid(a.M), 512, 0, st>>>(a);
      return ego_launch_status(label);
    }
    if constexpr (MODE != MODE_MLP) {
      if (sc->app_f16 == EGO_APP_HALF) {
        if (int e = check_app16(sc, who)) return e;
        a.F = make_field(sc->app16);
        launch_shade_h<MODE, DUMP, FOLD, COMPACT, true>(sc->mlp_precision, a, st);
        return ego_launch_status(label);
      }
    }
  }
  if constexpr (!DUMP && MODE != MODE_MLP) {
    if (sc->app_f16 == EGO_APP_DENSE) {   // the baked node grid (app16.plane[0][0]) instead of tables and basis
      if (int e = dense_app_field(sc, who, a.F)) return e;
      launch_shade_h<MODE, DUMP, FOLD, COMPACT, false, true>(sc->mlp_precision, a, st);
      return ego_launch_status(label);
    }
  }
  launch_shade_h<MODE, DUMP, FOLD, COMPACT, false>(sc->mlp_precision, a, st);
  return ego_launch_status(label);
}

}  // namespace

// ego_render_forward's question (csrc/ego_render.hip): can shading and compositing run as one launch for this scene and sample count?
bool ego_can_fold_composite(const ego_scene* sc, int32_t S) {
  return sc && ego_shape_is_tuned(sc) && sc->app_f16 != EGO_APP_HALF && sc->mlp_precision != EGO_PREC_F32 && sc->weight_thres <= 0.f && S >= 32 && (S & 31) == 0;
}

// ... and does it pay?  The folded kernel deals whole RAYS to its waves (a wave finishes its rays' pixels itself), the two-launch kernel
// deals 32-sample tiles: with few rays, or a ray count just above a multiple of the wave count, some waves get one ray more than the
// others and the launch runs as long as they do (4097 rays x 512 samples: 48 tiles on the critical path against 33).  Folded only when
// its critical path is within 3 % of the tile-granular one.
bool ego_fold_is_balanced(int64_t N, int32_t S) {
  if (N <= 0 || S < 32) return false;
  const int64_t tpr = S >> 5, n_wv = (int64_t)shade_grid(N * (int64_t)S) * 8;
  const int64_t rays_per_wave = (N + n_wv - 1) / n_wv, tiles_per_wave = (N * tpr + n_wv - 1) / n_wv;
  return rays_per_wave * tpr * 100 <= tiles_per_wave * 103;
}

extern "C" {

int32_t ego_render_forward_folds(const ego_scene* sc, int64_t N, int32_t S) {
  const char* f = getenv("EGO_RENDER_FOLD");
  if (f && f[0] == '0') return 0;
  if (!ego_can_fold_composite(sc, S)) return 0;
  return (f && f[0] == '1') || ego_fold_is_balanced(N, S) ? 1 : 0;
}

int ego_shade_kernel_info(int32_t precision, int32_t* out, int32_t n) {
  EGO_REQUIRE(out && n == 8, "shade_kernel_info: out must hold 8 values");
  EGO_REQUIRE(precision == EGO_PREC_F16X3 || precision == EGO_PREC_F32 || precision == EGO_PREC_F16F8 || precision == EGO_PREC_F16F6,
              "shade_kernel_info: unknown precision");
  out[0] = 32;
  if (precision == EGO_PREC_F32) {          // k_shade: one v_mfma_f32_32x32x2_f32 per k (basis) / per k and m-tile (layers 1, 2)
    out[1] = KS_BASIS + 4 * (KS1 + KS2); out[2] = 0; out[3] = 2 * 32 * 32 * 2; out[4] = 0; out[5] = 0;
  } else if (precision == EGO_PREC_F16X3) {  // three v_mfma_f32_32x32x16_f16 per 8-k step (and m-tile)
    out[1] = 3 * (KHB + 4 * (KH1 + KH2)); out[2] = 0; out[3] = 2 * 32 * 32 * 16; out[4] = 0; out[5] = 0;
  } else if (precision == EGO_PREC_F16F6) {  // basis as f16x3; layers 1, 2: one fp16 MFMA per step + two fp6 MFMAs per group of four steps
    out[1] = 3 * KHB + 4 * (KH1 + KH2); out[2] = 4 * 2 * (G6_1 + G6_2); out[3] = 2 * 32 * 32 * 16; out[4] = 2 * 32 * 32 * 64;
    out[5] = 2 * (G6_1 + G6_2);              // 32-value conversions (v_cvt_scalef32_pk32_fp6_f16 / _2xpk16_fp6_f32)
  } else {                                   // basis as f16x3; layers 1, 2: one fp16 MFMA per step + one fp8 MFMA per pair of steps
    out[1] = 3 * KHB + 4 * (KH1 + KH2); out[2] = 4 * (KH1 / 2 + KH2 / 2); out[3] = 2 * 32 * 32 * 16; out[4] = 2 * 32 * 32 * 64;
    out[5] = (KS1 + KS2) / 2 * 2;            // per pair of values: one v_cvt_pk_fp8_f32 (x) and one v_cvt_scalef32_pk_fp8_f32 (residual)
  }
  out[6] = 2 * (3 * APP_C * APP_DIM + MLP_IN * HID + HID * HID + HID * 3);
  out[7] = 3 * (4 + 2) * APP_C * 4;
  return EGO_OK;
}

int ego_app_feature(const ego_scene* sc, const float* c7n, int64_t M, float* out, void* stream) {
  EGO_TRACE("ego_app_feature");
  EGO_REQUIRE(M >= 0 && M < (1ll << 31), "app_feature: M out of range [0, 2^31)");
  if (M == 0) return EGO_OK;
  EGO_REQUIRE(c7n && out, "app_feature: null argument");
  if (sc && !ego_shape_is_tuned(sc)) return ego_generic_app_feature(sc, c7n, M, out, stream);
  if (int e = check_shade_config(sc, "app_feature", true, false)) return e;
  ShadeArgs a = shade_args(sc, M, 1);
  a.c7n = c7n; a.out = out;
  return launch_shade<MODE_APP>(sc, a, "app_feature", "k_shade<APP>", stream);
}

int ego_mlp_fea(const ego_scene* sc, const float* viewdirs, const float* feat, int64_t M, float* rgb, void* stream) {
  EGO_TRACE("ego_mlp_fea");
  EGO_REQUIRE(M >= 0 && M < (1ll << 31), "mlp_fea: M out of range [0, 2^31)");
  if (M == 0) return EGO_OK;
  EGO_REQUIRE(viewdirs && feat && rgb, "mlp_fea: null argument");
  if (sc && !ego_shape_is_tuned(sc)) return ego_generic_mlp_fea(sc, viewdirs, feat, M, rgb, stream);
  if (int e = check_shade_config(sc, "mlp_fea", false, true)) return e;
  ShadeArgs a = shade_args(sc, M, 1);
  a.feat = feat; a.dirs = viewdirs; a.out = rgb;
  return launch_shade<MODE_MLP>(sc, a, "mlp_fea", "k_shade<MLP>", stream);
}

int ego_shade(const ego_scene* sc, const float* rays, const float* z, const float* coords, int64_t N, int32_t S, float* rgb,
              const ego_shade_dump* dump, const uint8_t* tile_active, void* stream) {
  EGO_TRACE("ego_shade");
  EGO_REQUIRE(rays && z && rgb && N >= 0 && S >= 1 && N * (int64_t)S < (1ll << 31), "shade: null argument or N*S >= 2^31");
  if (sc && !ego_shape_is_tuned(sc)) {   // any other model shape: fp32 compatibility kernel (inference only)
    if (dump) return ego_fail(EGO_E_UNSUPPORTED, "shade: activation dumps (training) exist for the tuned model shape only (app_dim 27, 48 components, "
                                                  "MLP_Fea 150/128/128 with view_pe = fea_pe = 2)");
    if (N == 0) return EGO_OK;
    return ego_generic_shade(sc, rays, coords, N, S, rgb, tile_active, stream);
  }
  if (int e = check_shade_config(sc, "shade", true, true)) return e;
  EGO_REQUIRE(sc->r_lut && sc->n_r_lut >= 2 && sc->n_r_lut <= LUT_MAX, "shade: r_lut missing or > 1024 entries");
  EGO_REQUIRE(coords || sc->mlp_precision == EGO_PREC_F32, "shade: coords (from ego_march_density) is required unless mlp_precision = EGO_PREC_F32");
  if (N == 0) return EGO_OK;
  ShadeArgs a = shade_args(sc, N * (int64_t)S, S);
  a.rays = rays; a.z = z; a.coords = coords; a.out = rgb; a.tile_active = tile_active;
  if (!dump) return launch_shade<MODE_SHADE>(sc, a, "shade", "k_shade<SHADE>", stream);
  EGO_REQUIRE(sc->mlp_precision != EGO_PREC_F32 && dump->h1 && dump->h2 && dump->relu_bits && dump->fe,   // (x and v are optional)
              "shade: activation dumps need the fp16-split arithmetic (not EGO_PREC_F32) and non-null h1 / h2 / v / relu_bits / fe buffers (x is optional)");
  a.dump_x = dump->x; a.dump_h1 = dump->h1; a.dump_h2 = dump->h2; a.dump_v = dump->v; a.dump_bits = dump->relu_bits; a.dump_fe = dump->fe;
  return launch_shade<MODE_SHADE, true>(sc, a, "shade", "k_shade<SHADE>", stream);
}

}  // extern "C"

// ego_render_forward's compact path: ego_shade over the samples of the list live[*n_live] (csrc/ego_compact.hip) only; colours land at the
// samples' [N][S] places, the others are not written.  The grid is sized for N S samples and the kernel deals the ceil(*n_live / 32) tiles.
int ego_shade_live(const ego_scene* sc, const float* rays, const float* z, const float* coords, int64_t N, int32_t S, const int32_t* live,
                   const int32_t* n_live, float* rgb, void* stream) {
  EGO_TRACE("ego_shade_live");
  EGO_REQUIRE(rays && z && coords && live && n_live && rgb && N >= 1 && S >= 1 && N * (int64_t)S < (1ll << 31),
              "shade_live: null argument or N*S outside [1, 2^31)");
  EGO_REQUIRE(sc && ego_shape_is_tuned(sc), "shade_live: tuned model shape only");
  if (int e = check_shade_config(sc, "shade_live", true, true)) return e;
  EGO_REQUIRE(sc->r_lut && sc->n_r_lut >= 2 && sc->n_r_lut <= LUT_MAX, "shade_live: r_lut missing or > 1024 entries");
  ShadeArgs a = shade_args(sc, N * (int64_t)S, S);
  a.rays = rays; a.z = z; a.coords = coords; a.out = rgb; a.live = live; a.n_live = n_live;
  return launch_shade<MODE_SHADE, false, false, true>(sc, a, "shade_live", "k_shade<SHADE, live list>", stream);
}

extern "C" int ego_shade_composite(const ego_scene* sc, const float* rays, const float* z, const float* coords, const float* weight,
                                   const float* bg_weight, int64_t N, int32_t S, const uint8_t* tile_active, float* rgb_map, float* depth,
                                   float* bg_map, float* env_map, void* stream) {
  EGO_TRACE("ego_shade_composite");
  EGO_REQUIRE(rays && z && coords && weight && rgb_map && N >= 0 && S >= 32 && (S & 31) == 0 && N * (int64_t)S < (1ll << 31),
              "shade_composite: null argument, S not a multiple of 32, or N*S >= 2^31");
  if (!ego_can_fold_composite(sc, S)) return ego_fail(EGO_E_UNSUPPORTED, "shade_composite: tuned model shape, fp32 tables, a split-precision arithmetic and weight_thres <= 0 only");
  if (int e = check_shade_config(sc, "shade_composite", true, true)) return e;
  EGO_REQUIRE(!sc->envmap || bg_weight, "shade_composite: envmap needs bg_weight");
  if (N == 0) return EGO_OK;
  ShadeArgs a = shade_args(sc, N * (int64_t)S, S);
  a.rays = rays; a.z = z; a.coords = coords; a.tile_active = tile_active;
  a.comp_w = weight; a.comp_bg = bg_weight; a.envmap = sc->envmap; a.envmap_h = sc->envmap_h;
  a.rgb_map = rgb_map; a.depth = depth; a.bg_map = bg_map; a.env_map = env_map;
  return launch_shade<MODE_SHADE, false, true>(sc, a, "shade_composite", "k_shade<SHADE, composite>", stream);
}

// ego_render_forward's one-launch eval render: ego_march_density + ego_shade_composite as the marching form of the folded dense kernel.
// `m` is the march's argument block (ego_march_fill_args); the tile loop reads the workspace slots it names.
bool ego_can_march_in_shade(const ego_scene* sc, int32_t S) {
  return ego_can_fold_composite(sc, S) && sc->app_f16 == EGO_APP_DENSE && sc->density_dense && sc->density.n_comp == 16 &&
         sc->density.res[0] == sc->app.res[0] && sc->density.res[1] == sc->app.res[1] && sc->density.res[2] == sc->app.res[2] &&
         !sc->occ && !(sc->term_eps > 0.f) && sc->r_lut && sc->n_r_lut >= 2 && sc->n_r_lut <= LUT_MAX;
}

int ego_march_shade_composite(const ego_scene* sc, const MarchArgs& m, float* rgb_map, float* depth, float* bg_map, float* env_map, void* stream) {
  EGO_TRACE("ego_march_shade_composite");
  const int64_t N = m.N;
  const int32_t S = m.S;
  EGO_REQUIRE(rgb_map && m.dense && m.weight && m.coords_out && (m.z_in || m.z_out) && !m.occ.vol && !m.sigma_out && !(m.term_eps > 0.f) &&
              N >= 0 && S >= 32 && (S & 31) == 0 && N * (int64_t)S < (1ll << 31), "march_shade_composite: needs the dense march without mask or early termination, S a multiple of 32, N*S < 2^31");
  if (!ego_can_march_in_shade(sc, S)) return ego_fail(EGO_E_UNSUPPORTED, "march_shade_composite: the folded dense shade with both baked grids at one resolution only");
  if (int e = check_shade_config(sc, "march_shade_composite", true, true)) return e;
  EGO_REQUIRE(!sc->envmap || m.bg, "march_shade_composite: envmap needs bg_weight");
  if (N == 0) return EGO_OK;
  ShadeArgs a = shade_args(sc, N * (int64_t)S, S);
  a.rays = m.rays; a.z = m.z_out ? m.z_out : m.z_in; a.coords = m.coords_out; a.tile_active = m.tile_active;
  a.comp_w = m.weight; a.comp_bg = m.bg; a.envmap = sc->envmap; a.envmap_h = sc->envmap_h;
  a.rgb_map = rgb_map; a.depth = depth; a.bg_map = bg_map; a.env_map = env_map;
  a.F = make_field(sc->app);
  if (int e = dense_app_field(sc, "march_shade_composite", a.F)) return e;
  MarchBlock mb;
  mb.a = m;
  const int64_t n_wv = (int64_t)shade_grid(a.M) * 8;
  mb.rays_per_wave = (int32_t)((N + n_wv - 1) / n_wv);
  launch_shade_march(sc->mlp_precision, a, mb, (hipStream_t)stream);
  return ego_launch_status("k_shade<SHADE, composite, march>");
}

