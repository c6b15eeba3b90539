// The tuned model shape (app_dim 27, 48 appearance components, MLP_Fea 150 -> 128 -> 128 -> 3 with view_pe = fea_pe = 2) as the
// translation units that serve it share it: shape constants, the layout of the packed weight blob, the per-lane K orders that the
// packers (ego_pack.hip) bake into the weights and the kernels (ego_shade.hip, ego_train.hip, ego_wgrad.hip) rely on, the fp16-split
// operand types, and the host-side checks of the entry points.
//
// Work mapping (wave64): a wave owns a tile of 32 consecutive samples; lane l serves sample
// j = l & 31 and "half" h = l >> 5.  In D = A*B (32x32x2): A[i][k] comes from lane (i, k) = (l&31, l>>5),
// B[k][j] from lane (j, k) = (l&31, l>>5), and D[i][j] lands in lane j + 32*((i>>2)&1), register
// r = (i&3) + 4*(i>>3).  So with samples on the N axis a lane only ever supplies / receives values of
// ITS OWN sample: the gathered products feed the basis MFMAs straight from registers, the basis
// output feeds layer 1, layer 1 feeds layer 2 — no cross-lane traffic, no LDS round trip for
// activations.  The price is a fixed K-order per lane half, which ego_pack_mlp bakes into the weights:
//   * lane half h gathers appearance channels [24h, 24h+24) of each of the 3 planes  (72 k-steps)
//   * basis rows are permuted so half h receives features f = 2r + h in register r   (14 slots)
//   * layer-1 k-steps: 80 per half, slot-major; the order is defined once, at x_channel() below
//   * layer-2 k-step m*16 + r consumes hidden unit m*32 + (r&3) + 8*(r>>2) + 4h
// Layer 3 (128 -> 3) runs on the VALU from the layer-2 accumulators + one xor-32 exchange.
#pragma once
#include "ego_device.h"
#include "ego_host.h"

constexpr int APP_C = 48;      // appearance components per plane
constexpr int APP_HALF = 24;   // channels gathered by one lane half
constexpr int APP_DIM = 27;
constexpr int HID = 128;
constexpr int NSLOT = 14;      // feature slots per lane half
constexpr int KS_BASIS = 72;
constexpr int KS1 = 80;
constexpr int KS2 = 64;
constexpr int MLP_IN = 150;

constexpr int OFF_W1 = 0;                           // [KS1/4][4 m][64 lanes][4]
constexpr int OFF_W2 = OFF_W1 + KS1 * 4 * 64;       // [KS2/4][4 m][64][4]
constexpr int OFF_B1 = OFF_W2 + KS2 * 4 * 64;       // [4 m][2 h][16 r]
constexpr int OFF_B2 = OFF_B1 + 128;
constexpr int OFF_W3 = OFF_B2 + 128;                // [4 m][2 h][16 r][4 (c0,c1,c2,0)]
constexpr int OFF_B3 = OFF_W3 + 512;                // [4]
constexpr int LDS_W_FLOATS = OFF_B3 + 4;            // 37636 floats = 150544 B
constexpr int OFF_BASIS = LDS_W_FLOATS;             // [2 g][KS_BASIS/4][64][4]
constexpr int PACKED_FLOATS = OFF_BASIS + 2 * (KS_BASIS / 4) * 64 * 4;
constexpr int LUT_MAX = 1024;

__host__ __device__ constexpr int slot_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// appearance channel (0..143, plane-major) gathered by lane half h as its kk-th product: the halves interleave at
// 16-byte granularity (half h owns float4 quads 2i+h of a texel), so the two lanes of a sample always read the
// same 64-byte line in a given load instruction -> half as many L1 tag lookups as a [0,24) / [24,48) split.
// K order of the f16x3 kernel's gather (gather_team4, ego_shade.hip): samples are gathered by 4-lane teams (part p reads quad
// 4i+p of line i, so a team reads whole 64-byte lines) and transposed into the 2-lanes-per-sample MFMA layout with
// v_permlane16_swap + v_permlane32_swap.  Lane half h ends up with the parts p = h (first 12 products of a plane) and
// p = h + 2 (next 12): product kk = plane*24 + half*12 + i*4 + c is channel plane*48 + 16i + 4(h + 2 half) + c.
// Activation dumps of the training forward / backward (logical [M][2 K] matrices: x 160, h1/h2/dh1/dh2 128, v 144 columns).
// Logical column of element kk of lane half h: dump_col(kk, h) (the float4 quads of the two halves interleave).  Storage is
// tile-blocked and lane-major: [tile = m / 32][quad pair q = kk / 4][lane = 32 h + (m % 32)][4 floats], so every store / load
// instruction of the shade kernels moves 1 KB of contiguous memory (row-major rows gave 32-byte pieces 640 B apart and
// 2.5 TB/s; this layout 1.88 -> 1.37 ms for the dumping forward).  Buffers hold ceil(M / 32) * 32 rows.
__host__ __device__ constexpr int64_t dump_off(int64_t tile, int width, int q, int h, int j) {
  return tile * (32 * (int64_t)width) + q * 256 + (h * 32 + j) * 4;
}
__host__ __device__ constexpr int dump_col(int kk, int h) { return (kk >> 2) * 8 + h * 4 + (kk & 3); }

__host__ __device__ constexpr int app_channel_g(int kk, int h) {
  return (kk / APP_HALF) * APP_C + (((kk % APP_HALF) % 12) / 4) * 16 + 4 * (h + 2 * ((kk % APP_HALF) / 12)) + (kk % 4);
}

// (fp32-MFMA kernel k_shade: lane half h owns float4 quads 2i+h)
__host__ __device__ constexpr int app_channel(int kk, int h) {
  return (kk / APP_HALF) * APP_C + ((kk % APP_HALF) / 4) * 8 + 4 * h + (kk % 4);
}

// ---- the layer-1 operand order: THE definition; the weight packers, the shade kernels, the weight-gradient pass and
// ego_train_layout(0) all take it from here.  X register kk of lane half h: 14 feature slots r (feature f = 2r + h) x
// (f, sin f, sin 2f, cos f, cos 2f), then the half's eight view slots, then two zero pads.
constexpr int KX_FEAT = 5 * NSLOT;   // first view slot

// reference MLP input column held by X register kk of lane half h (-1: zero weight)
__host__ __device__ constexpr int x_channel(int kk, int h) {
  if (kk < KX_FEAT) {
    const int kind = kk % 5, r = kk / 5, f = 2 * r + h;
    if (f >= APP_DIM) return -1;
    const int pe0 = APP_DIM + 3;               // 30: sin block of the feature PE
    const int pe1 = pe0 + 2 * APP_DIM;         // 84: cos block
    switch (kind) {
      case 0: return f;
      case 1: return pe0 + 2 * f;
      case 2: return pe0 + 2 * f + 1;
      case 3: return pe1 + 2 * f;
      default: return pe1 + 2 * f + 1;
    }
  }
  if (kk < KX_FEAT + 8) {
    const int t = (kk - KX_FEAT) + 8 * h;
    // d0 d1 d2 | sin d0, sin 2d0, sin d1, sin 2d1, sin d2, sin 2d2 | cos ... | pad
    return t < 3 ? APP_DIM + t : (t < 15 ? APP_DIM + 3 + 4 * APP_DIM + (t - 3) : -1);
  }
  return -1;
}

// kk is the first value of a feature slot: the generator encodes the slot here
__host__ __device__ constexpr bool layer1_slot_head(int kk) { return kk < KX_FEAT && kk % 5 == 0; }

// values that are not bounded by 1 (features, raw view direction): all the f16f6 block maximum has to look at
__host__ __device__ constexpr bool layer1_unbounded(int kk) {
  return layer1_slot_head(kk) || (kk >= KX_FEAT && kk < KX_FEAT + 3);
}

// The two encoders of (sin x, cos x, sin 2x, cos 2x): hardware transcendentals (the f16 kernels and everything that re-derives
// their operands) and the fp32 kernel's polynomial form
struct EncHw {
  static __device__ __forceinline__ void enc(float x, float& s1, float& c1, float& s2, float& c2) { sincos_x_2x_hw(x, s1, c1, s2, c2); }
};
struct EncF32 {
  static __device__ __forceinline__ void enc(float x, float& s1, float& c1, float& s2, float& c2) {
    sincos_f32(x, s1, c1);
    sincos_f32(__fmul_rn(x, 2.f), s2, c2);
  }
};

// the eight view slots of lane half h (3 raw + 12 encodings + 1 pad over the two halves)
template <class ENC>
__device__ __forceinline__ void view_slots(float d0, float d1, float d2, int h, float (&vw)[8]) {
  float sa0, ca0, sb0, cb0, sa1, ca1, sb1, cb1, sa2, ca2, sb2, cb2;
  ENC::enc(d0, sa0, ca0, sb0, cb0);
  ENC::enc(d1, sa1, ca1, sb1, cb1);
  ENC::enc(d2, sa2, ca2, sb2, cb2);
  // half 0: d0 d1 d2 sin(d0) sin(2d0) sin(d1) sin(2d1) sin(d2) | half 1: sin(2d2) cos(d0) cos(2d0) ... cos(2d2) 0
  vw[0] = h ? sb2 : d0; vw[1] = h ? ca0 : d1; vw[2] = h ? cb0 : d2; vw[3] = h ? ca1 : sa0;
  vw[4] = h ? cb1 : sb0; vw[5] = h ? ca2 : sa1; vw[6] = h ? cb2 : sb1; vw[7] = h ? 0.f : sa2;
}

// X register kk (a constant after unrolling) of a lane half, picked from its slot's feature value f and encodings s1 .. c2, or from
// the half's view slots vw.  An expression: ego_wgrad.hip's x_make encodes its slots ahead of the loads' arrival and picks from
// arrays, and through a function its kernel's code changes.  The operands of the other branches are not evaluated.
#define EGO_LAYER1_PICK(kk, f, s1, c1, s2, c2, vw)                                                                              \
  ((kk) < KX_FEAT ? ((kk) % 5 == 0 ? (f) : ((kk) % 5 == 1 ? (s1) : ((kk) % 5 == 2 ? (s2) : ((kk) % 5 == 3 ? (c1) : (c2))))) \
                  : ((kk) < KX_FEAT + 8 ? (vw)[(kk) - KX_FEAT] : 0.f))

// The generator of the shade kernels: walk kk upwards; fe[r] = the half's feature slots.  Slot r is encoded into s1 .. c2 when its
// first value is asked for, i.e. right before the MFMAs that consume it.
template <class ENC, class FE>
__device__ __forceinline__ float layer1_value(int kk, const FE& fe, const float (&vw)[8], float& s1, float& c1, float& s2, float& c2) {
  if (layer1_slot_head(kk)) ENC::enc(fe[kk / 5], s1, c1, s2, c2);
  return EGO_LAYER1_PICK(kk, fe[kk / 5], s1, c1, s2, c2, vw);
}

// ---- fp16-split ("f16x3") weight layout ------------------------------------------------------------------
// Same regions/offsets as the fp32 blob, but the three matrix regions hold fp16 pairs: w = hi + lo with
// hi = fp16(w), lo = fp16(w - hi) (22 significant bits).  Fragment order [k-step][m-tile][term hi|lo][lane][8 k]:
// one ds_read_b128 / global_load_dwordx4 per (step, tile, term) per lane, conflict-free.  A lane's 8 k of a step
// are its values 8*step .. 8*step+7 in the same per-half K order as the fp32 layout.
constexpr int KH1 = KS1 / 8, KH2 = KS2 / 8, KHB = KS_BASIS / 8;
constexpr int BASIS16_FLOATS = 2 * KHB * 2 * 64 * 4;  // third blob region (basis fragments for the fp16-table gather): [2 g][9 steps][2 terms][64 lanes][8 halves]

__device__ inline void split_weight(float w, _Float16& hi, _Float16& lo) {
  hi = (_Float16)w;
  lo = (_Float16)(w - (float)hi);
}

// ---- fp16 main term + fp8 correction terms ("f16f8") weight layout ----------------------------------------------------
// w*x = w_hi*x_hi (one v_mfma_f32_32x32x16_f16 per k-step, as in f16x3) + [w_lo*x_hi + w_hi*x_lo] on the block-scaled fp8 path:
// ONE v_mfma_scale_f32_32x32x64_f8f6f4 per PAIR of k-steps carries both correction terms (K = 64 = 2 terms x 2 steps x 8 values
// x 2 lane halves), at ~1.9x the matrix-pipe time of one fp16 instruction instead of 4x.  The corrections are ~2^-11 of the main
// term, so e4m3's 4 significant bits leave ~2^-16 relative error per product (measured: DESIGN.md 4.1, profiles/r02/precision_sweep.json).
// Operand bytes of a lane (row i = lane & 31 of m-tile mt, half h = lane >> 5; probed layout: byte b = k offset b of the lane's
// 32-wide K block, tools/fp8_layout_probe.hip):
//   A: [0..7] e4m3(w_lo * 2^11) step 2p | [8..15] same, step 2p+1 | [16..23] e4m3(w_hi) step 2p | [24..31] e4m3(w_hi) step 2p+1
//   B: [0..7] e4m3(x)           step 2p | [8..15] same, step 2p+1 | [16..23] e4m3(x_lo * 2^11) step 2p | [24..31] ..., step 2p+1
// and the instruction's E8M0 block scale of A is 2^-11 (exponent byte 116), of B 2^0 (127).
// Region layout (32-bit slots, same OFF_W1 / OFF_W2 extents as the other layouts, so the LDS image keeps its size):
//   per layer: hi fragments [step][m-tile][lane][8 halves], then fp8 fragments [pair][m-tile][part 0|1][lane][16 bytes]
constexpr int F8_HI1 = KH1 * 4 * 64 * 4;          // 32-bit slots of layer 1's hi part (10240)
constexpr int F8_HI2 = KH2 * 4 * 64 * 4;          // layer 2 (8192)
constexpr int F8_FLOATS = OFF_B1;                 // W1 + W2 regions only; biases / W3 come from the f16x3 blob

// ---- fp16 main term + fp6 correction terms ("f16f6") weight layout ------------------------------------------------------------
// Same split as f16f8, with the two correction terms on the fp6 (e2m3) path of v_mfma_scale_f32_32x32x64_f8f6f4, which runs at
// 1.18x the time of one fp16 32x32x16 instruction where the fp8 path takes 2.0x, and whose operands one conversion instruction
// produces for 32 values at a time (v_cvt_scalef32_pk32_fp6_f16 / v_cvt_scalef32_2xpk16_fp6_f32: 64 clk per 32 values against
// 16 x ~10 clk on the fp8 path; tools/fp6_probe.hip, profiles/r04/fp6_probe.txt).  e2m3 spans 6 binades only, so every block of 32
// K values of a lane carries its own power-of-two scale (the instruction's E8M0 block scale is per lane): static for the weights
// (from the block's largest magnitude), dynamic for the activations (exponent of the largest |x| of the lane's 32 values).
// A GROUP is 4 k-steps = 32 values of a lane half; per group and m-tile two fp6 MFMAs: term 0 = w_lo * x_hi, term 1 = w_hi * x_lo.
// Element e of a lane's 192-bit operand sits at bits [6e, 6e + 6); it carries the lane's K value f6_value(layer, group, term, e):
//   term 0 (B from pk32_fp6_f16 of the four steps' packed halves): value 32 g + e
//   term 1 (B from 2xpk16_fp6_f32 of the residuals, which interleaves its two 16-value sources): even e -> 32 g + e / 2, odd e -> 32 g + 16 + e / 2
//   layer 1's last group holds only steps 8, 9: both terms come from 2xpk16(values, zeros): even e -> 64 + e / 2, odd e -> none
// Scale bytes: with eb = biased exponent of the block's largest |x| (clamped to >= 14) the conversions divide by 2^(eb - 129) (x) and
// 2^(eb - 140) (residual, i.e. 2^-11 further down) and the MFMAs pass eb itself as B's block scale; the 2^-2 / 2^-13 that this
// overstates is folded into A's static scale byte, which is biased(weight block scale) - 2 (term 0) / - 13 (term 1).
// Image layout (32-bit slots; it replaces the first OFF_B1 slots of the LDS image, biases / W3 behind it stay where they are):
//   F6I_HI1 / F6I_HI2: fp16 hi fragments [step][m-tile][lane][8 halves] of layers 1 / 2 (as f16f8)
//   F6I_Q1 / F6I_Q2:   the fp6 operands [group][m-tile][quad 0..2][lane][4]: the two terms' 6 + 6 dwords of a lane as three 16-byte
//                      pieces: term 0 dwords 0-3 | term 1 dwords 0-3 | term 0 dwords 4-5, term 1 dwords 4-5.  (Separate 16 + 8 byte
//                      pieces per term made the compiler pair the 8-byte reads of neighbouring fragments and copy the halves apart,
//                      +42 v_mov per tile; term 0's six dwords followed by term 1's, +81: it does not coalesce a 12-register tuple.)
//   F6I_SC:            scale bytes [group (layer 1's three, then layer 2's two)][lane][2 dwords]: byte mt of dword t = block scale of
//                      (term t, m-tile mt) - the MFMA's op_sel picks the byte
// The kernel addresses LDS as `per-lane base + 16-bit immediate` with one opaque base per 64 KB window (f6_bases): left to itself
// the compiler spends a v_add on every read beyond 64 KB (62 more per tile than f16f8).
constexpr int G6_1 = 3, G6_2 = 2;                 // groups per layer
constexpr int F6I_HI1 = 0, F6I_HI2 = F6I_HI1 + F8_HI1;
constexpr int F6I_Q1 = F6I_HI2 + F8_HI2, F6I_Q2 = F6I_Q1 + G6_1 * 4 * 3 * 256;
constexpr int F6I_SC = F6I_Q2 + G6_2 * 4 * 3 * 256;
constexpr int F6I_END = F6I_SC + (G6_1 + G6_2) * 128;
constexpr int F6_FLOATS = OFF_B1;
static_assert(F6I_END <= F6_FLOATS, "f16f6 image must fit the W1 / W2 part of the LDS image");
static_assert(F6I_SC * 4 < 3 * 65536, "16-byte-stride part of the f16f6 image: three 64 KB windows");

// ---- fp16-split operands: x = hi + lo with hi = fp16(x), lo = fp16(x - hi); a product runs as three v_mfma_f32_32x32x16_f16
// (w_hi*x_hi + w_lo*x_hi + w_hi*x_lo, fp32 accumulate)
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
#define MFMAH(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)

struct HL {
  h8 hi, lo;
};

__device__ __forceinline__ void split_pair(float a, float b, bool keep, uint32_t& hi, uint32_t& lo) {
  a = keep ? a : 0.f;
  b = keep ? b : 0.f;
  const auto hp = __builtin_amdgcn_cvt_pkrtz(a, b);
  hi = __builtin_bit_cast(uint32_t, hp);
  // residuals a - hi, b - hi are exact; each is ONE v_fma_mix_f32 (hi * -1 + a) reading the half straight from the packed
  // register: no v_cvt_f32_f16 back-conversion (VALU and MFMA time add up on this SIMD, tools/coissue_probe.hip).  The -1 is
  // made opaque so that the fma survives to instruction selection (a literal -1 folds into convert + subtract); the
  // instruction should come from the compiler rather than from inline asm, which its hazard recogniser cannot see into.
  float neg1 = -1.0f;
  asm("" : "+v"(neg1));
  const float ra = __builtin_fmaf((float)hp[0], neg1, a), rb = __builtin_fmaf((float)hp[1], neg1, b);
  lo = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(ra, rb));
}

__device__ __forceinline__ HL split8(const float x[8], bool keep) {
  u32x4 hi, lo;
  uint32_t a, b;
  split_pair(x[0], x[1], keep, a, b); hi.x = a; lo.x = b;
  split_pair(x[2], x[3], keep, a, b); hi.y = a; lo.y = b;
  split_pair(x[4], x[5], keep, a, b); hi.z = a; lo.z = b;
  split_pair(x[6], x[7], keep, a, b); hi.w = a; lo.w = b;
  HL o;
  o.hi = __builtin_bit_cast(h8, hi);
  o.lo = __builtin_bit_cast(h8, lo);
  return o;
}

// 8 fp32 values -> 8 halves, round to nearest: one k-step of an activation dump (ego_shade_dump's x / h1 / h2), and of the x
// that ego_weight_grad_x re-derives
__device__ __forceinline__ u32x4 pack8_rn(const float x[8]) {
  u32x4 o;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    typedef float f2v __attribute__((ext_vector_type(2)));
    typedef _Float16 h2v __attribute__((ext_vector_type(2)));
    o[q] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f2v{x[2 * q], x[2 * q + 1]}, h2v));
  }
  return o;
}

// ---- host side: what every entry point of the tuned shape checks, and the persistent grid of the shade-shaped kernels
static inline int check_shade_config(const ego_scene* sc, const char* who, bool need_tables, bool need_mlp) {
  if (!sc) return ego_fail(EGO_E_BADARG, "%s: null scene", who);
  if (sc->app_dim != APP_DIM) return ego_fail(EGO_E_UNSUPPORTED, "%s: app_dim %d (supported: 27)", who, sc->app_dim);
  if (need_tables) {
    if (sc->app.n_comp != APP_C) return ego_fail(EGO_E_UNSUPPORTED, "%s: appearance n_comp %d (supported: 48)", who, sc->app.n_comp);
    for (int g = 0; g < 2; ++g)
      for (int i = 0; i < 3; ++i)
        if (!sc->app.plane[g][i] || !sc->app.line[g][i]) return ego_fail(EGO_E_BADARG, "%s: null appearance table", who);
    if (sc->app.res[0] < 2 || sc->app.res[1] < 2 || sc->app.res[2] < 2) return ego_fail(EGO_E_BADARG, "%s: appearance resolution < 2", who);
    if (!ego_field_is_compact(sc->app, 4))
      return ego_fail(EGO_E_BADARG, "%s: the 12 appearance tables must lie within 4 GB of each other (allocate them from one buffer)", who);
  }
  if (need_mlp && (sc->mlp_in != MLP_IN || sc->mlp_hidden != HID || sc->view_pe != 2 || sc->fea_pe != 2))
    return ego_fail(EGO_E_UNSUPPORTED, "%s: MLP_Fea config in=%d hidden=%d view_pe=%d fea_pe=%d (supported: 150/128/2/2)", who,
                    sc->mlp_in, sc->mlp_hidden, sc->view_pe, sc->fea_pe);
  if (!sc->packed) return ego_fail(EGO_E_BADARG, "%s: scene.packed is null (call ego_pack_mlp first)", who);
  return EGO_OK;
}

static inline int check_app16(const ego_scene* sc, const char* who) {
  if (sc->app16.n_comp != APP_C) return ego_fail(EGO_E_BADARG, "%s: app_f16 is set but app16.n_comp is %d", who, sc->app16.n_comp);
  for (int g = 0; g < 2; ++g)
    for (int i = 0; i < 3; ++i)
      if (!sc->app16.plane[g][i] || !sc->app16.line[g][i]) return ego_fail(EGO_E_BADARG, "%s: app_f16 is set but an app16 table is null", who);
  return EGO_OK;
}

static inline unsigned shade_grid(int64_t M) {
  const int64_t tiles = (M + 31) >> 5;
  const int64_t wgs = (tiles + 7) / 8;
  return (unsigned)(wgs < 256 ? wgs : 256);  // persistent: one 8-wave workgroup per CU
}
