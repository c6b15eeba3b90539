// libegonerf_hip.so: the weight / basis packers of the tuned shape.  ego_pack_mlp turns the MLP_Fea weights and the two basis
// matrices into the blob the shade kernels read (ego_tuned.h has its regions and K orders): the fp32 fragments, their fp16-split
// form, the basis fragments for the fp16-table gather, and the f16f8 / f16f6 images of layers 1 and 2.
#include "ego_tuned.h"
#include "ego_generic.h"

namespace {

__global__ void k_pack_mlp(const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                           const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ b3,
                           const float* __restrict__ basis_yin, const float* __restrict__ basis_yang,
                           float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= PACKED_FLOATS) return;
  float v = 0.f;
  if (idx < OFF_W2) {  // W1 fragments
    const int j = idx & 3, lane = (idx >> 2) & 63, m = (idx >> 8) & 3, kk4 = idx >> 10;
    const int ch = x_channel(kk4 * 4 + j, lane >> 5);
    if (ch >= 0) v = w1[(m * 32 + (lane & 31)) * MLP_IN + ch];
  } else if (idx < OFF_B1) {  // W2 fragments
    const int e = idx - OFF_W2;
    const int j = e & 3, lane = (e >> 2) & 63, m2 = (e >> 8) & 3, kk4 = e >> 10;
    const int kk = kk4 * 4 + j;
    v = w2[(m2 * 32 + (lane & 31)) * HID + (kk >> 4) * 32 + slot_row(kk & 15, lane >> 5)];
  } else if (idx < OFF_W3) {  // biases of layers 1, 2 in accumulator layout
    const int e = (idx - OFF_B1) & 127;
    const float* b = (idx < OFF_B2) ? b1 : b2;
    v = b[(e >> 5) * 32 + slot_row(e & 15, (e >> 4) & 1)];
  } else if (idx < OFF_B3) {  // W3 in accumulator layout
    const int e = idx - OFF_W3;
    const int c = e & 3, r = (e >> 2) & 15, h = (e >> 6) & 1, m = e >> 7;
    if (c < 3) v = w3[c * HID + m * 32 + slot_row(r, h)];
  } else if (idx < OFF_BASIS) {
    const int c = idx - OFF_B3;
    if (c < 3) v = b3[c];
  } else {  // basis fragments
    const int e = idx - OFF_BASIS;
    const int j = e & 3, lane = (e >> 2) & 63, kk4 = (e >> 8) % (KS_BASIS / 4), g = e / (KS_BASIS / 4 * 256);
    const int i = lane & 31, h = lane >> 5, kk = kk4 * 4 + j;
    const int rh = (i >> 2) & 1, r = (i & 3) + 4 * (i >> 3), f = 2 * r + rh;  // feature delivered to tile row i
    if (r < NSLOT && f < APP_DIM) {
      const int col = app_channel(kk, h);
      v = (g ? basis_yang : basis_yin)[f * (3 * APP_C) + col];
    }
  }
  out[idx] = v;
}

__global__ void k_pack_mlp_h(const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                             const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ b3,
                             const float* __restrict__ basis_yin, const float* __restrict__ basis_yang,
                             const float* __restrict__ f32_blob, float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // one 32-bit slot = two fp16
  if (idx >= PACKED_FLOATS) return;
  if (idx >= OFF_B1 && idx < OFF_BASIS) { out[idx] = f32_blob[idx]; return; }  // biases, W3, b3 stay fp32
  _Float16 pr[2];
  for (int p = 0; p < 2; ++p) {
    float w = 0.f;
    int term;
    if (idx < OFF_W2) {
      const int hidx = (idx - OFF_W1) * 2 + p;
      const int e = hidx & 7, lane = (hidx >> 3) & 63, step = hidx >> 12, mt = (hidx >> 10) & 3;
      term = (hidx >> 9) & 1;
      const int ch = x_channel(step * 8 + e, lane >> 5);
      if (ch >= 0) w = w1[(mt * 32 + (lane & 31)) * MLP_IN + ch];
    } else if (idx < OFF_B1) {
      const int hidx = (idx - OFF_W2) * 2 + p;
      const int e = hidx & 7, lane = (hidx >> 3) & 63, step = hidx >> 12, mt = (hidx >> 10) & 3;
      term = (hidx >> 9) & 1;
      const int kk = step * 8 + e;
      w = w2[(mt * 32 + (lane & 31)) * HID + (kk >> 4) * 32 + slot_row(kk & 15, lane >> 5)];
    } else {
      const int hidx = (idx - OFF_BASIS) * 2 + p;
      const int e = hidx & 7, lane = (hidx >> 3) & 63, sg = hidx >> 10;  // sg = g * KHB + step
      term = (hidx >> 9) & 1;
      const int g = sg / KHB, kk = (sg % KHB) * 8 + e;
      const int i = lane & 31, h = lane >> 5;
      const int rh = (i >> 2) & 1, r = (i & 3) + 4 * (i >> 3), f = 2 * r + rh;
      if (r < NSLOT && f < APP_DIM) {
        const int col = app_channel_g(kk, h);
        w = (g ? basis_yang : basis_yin)[f * (3 * APP_C) + col];
      }
    }
    _Float16 hi, lo;
    split_weight(w, hi, lo);
    pr[p] = term ? lo : hi;
  }
  typedef _Float16 h2v __attribute__((ext_vector_type(2)));
  h2v v = {pr[0], pr[1]};
  out[idx] = __builtin_bit_cast(float, v);
}

// basis fragments for the fp16-table gather: same [g][step][term][lane][8] order, columns follow app_channel_f16
__host__ __device__ constexpr int app_channel_f16_fwd(int kk, int h) {
  return (kk / APP_HALF) * APP_C + ((kk % APP_HALF) / 8) * 16 + 8 * h + (kk % 8);
}

__global__ void k_pack_basis16(const float* __restrict__ basis_yin, const float* __restrict__ basis_yang, float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * KHB * 2 * 64 * 4) return;
  _Float16 pr[2];
  for (int p = 0; p < 2; ++p) {
    const int hidx = idx * 2 + p;
    const int e = hidx & 7, lane = (hidx >> 3) & 63, term = (hidx >> 9) & 1, sg = hidx >> 10;
    const int g = sg / KHB, kk = (sg % KHB) * 8 + e;
    const int i = lane & 31, h = lane >> 5;
    const int rh = (i >> 2) & 1, r = (i & 3) + 4 * (i >> 3), f = 2 * r + rh;
    float w = 0.f;
    if (r < NSLOT && f < APP_DIM) w = (g ? basis_yang : basis_yin)[f * (3 * APP_C) + app_channel_f16_fwd(kk, h)];
    _Float16 hi, lo;
    split_weight(w, hi, lo);
    pr[p] = term ? lo : hi;
  }
  typedef _Float16 h2v __attribute__((ext_vector_type(2)));
  h2v v = {pr[0], pr[1]};
  out[idx] = __builtin_bit_cast(float, v);
}

__device__ inline uint32_t e4m3_byte(float v) {
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v, 0.f, 0, false) & 0xffu;
}

__global__ void k_pack_mlp_f8(const float* __restrict__ w1, const float* __restrict__ w2, float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // one 32-bit slot
  if (idx >= F8_FLOATS) return;
  const bool l2 = idx >= OFF_W2;
  const int e0 = l2 ? idx - OFF_W2 : idx;
  const int hi_slots = l2 ? F8_HI2 : F8_HI1;
  auto weight = [&](int step, int e, int lane, int mt) -> float {
    if (!l2) {
      const int ch = x_channel(step * 8 + e, lane >> 5);
      return ch >= 0 ? w1[(mt * 32 + (lane & 31)) * MLP_IN + ch] : 0.f;
    }
    const int kk = step * 8 + e;
    return w2[(mt * 32 + (lane & 31)) * HID + (kk >> 4) * 32 + slot_row(kk & 15, lane >> 5)];
  };
  uint32_t word = 0;
  if (e0 < hi_slots) {  // [step][mt][lane][8 halves]
    _Float16 pr[2];
    for (int p = 0; p < 2; ++p) {
      const int hidx = e0 * 2 + p;
      const int e = hidx & 7, lane = (hidx >> 3) & 63, mt = (hidx >> 9) & 3, step = hidx >> 11;
      _Float16 hi, lo;
      split_weight(weight(step, e, lane, mt), hi, lo);
      pr[p] = hi;
    }
    typedef _Float16 h2v __attribute__((ext_vector_type(2)));
    h2v v = {pr[0], pr[1]};
    word = __builtin_bit_cast(uint32_t, v);
  } else {  // [pair][mt][part][lane][16 bytes]
    for (int b = 0; b < 4; ++b) {
      const int bidx = (e0 - hi_slots) * 4 + b;
      const int byte = bidx & 15, lane = (bidx >> 4) & 63, part = (bidx >> 10) & 1, mt = (bidx >> 11) & 3, pair = bidx >> 13;
      const int pos = part * 16 + byte;                    // byte of the 32-byte operand
      const int step = 2 * pair + ((pos >> 3) & 1), e = pos & 7;
      const float w = weight(step, e, lane, mt);
      _Float16 hi, lo;
      split_weight(w, hi, lo);
      const float v = pos < 16 ? (w - (float)hi) * 2048.0f : (float)hi;
      word |= e4m3_byte(v) << (8 * b);
    }
  }
  out[idx] = __builtin_bit_cast(float, word);
}

__host__ __device__ constexpr int f6_value(int layer2, int grp, int term, int e) {
  if (!layer2 && grp == G6_1 - 1) return (e & 1) ? -1 : 64 + (e >> 1);
  if (term == 0) return 32 * grp + e;
  return 32 * grp + ((e & 1) ? 16 + (e >> 1) : (e >> 1));
}

// e2m3 code of v (already divided by its block scale): round to nearest even, saturating at 7.5
__device__ inline uint32_t e2m3_code(float v) {
  const uint32_t s = v < 0.f ? 32u : 0u;
  const float a = fminf(fabsf(v), 7.5f);
  if (a < 1.0f) return s | (uint32_t)rintf(a * 8.0f);     // subnormal step 1/8; 8 = the code of 1.0
  const int e = a < 2.0f ? 0 : (a < 4.0f ? 1 : 2);
  int m = (int)rintf(ldexpf(a, 3 - e));                    // 8..16
  int ee = e;
  if (m == 16) { m = 8; ee = e + 1; }
  if (ee > 2) return s | 31u;
  return s | (uint32_t)(((ee + 1) << 3) | (m - 8));
}

__device__ inline float mlp_weight_k(const float* __restrict__ w1, const float* __restrict__ w2, bool l2, int k, int lane, int mt) {
  if (!l2) {
    const int ch = k < KS1 ? x_channel(k, lane >> 5) : -1;
    return ch >= 0 ? w1[(mt * 32 + (lane & 31)) * MLP_IN + ch] : 0.f;
  }
  return w2[(mt * 32 + (lane & 31)) * HID + (k >> 4) * 32 + slot_row(k & 15, lane >> 5)];
}

// the fp16 hi fragments of both layers: one thread per 32-bit slot
__global__ void k_pack_mlp_f6(const float* __restrict__ w1, const float* __restrict__ w2, float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t* o = (uint32_t*)out;
  const int n_hi = F8_HI1 + F8_HI2;
  if (idx < n_hi) {  // [step][mt][lane][8 halves]
    const bool l2 = idx >= F8_HI1;
    const int e0 = l2 ? idx - F8_HI1 : idx;
    _Float16 pr[2];
    for (int p = 0; p < 2; ++p) {
      const int hidx = e0 * 2 + p;
      const int e = hidx & 7, lane = (hidx >> 3) & 63, mt = (hidx >> 9) & 3, step = hidx >> 11;
      _Float16 hi, lo;
      split_weight(mlp_weight_k(w1, w2, l2, step * 8 + e, lane, mt), hi, lo);
      pr[p] = hi;
    }
    typedef _Float16 h2v __attribute__((ext_vector_type(2)));
    h2v v = {pr[0], pr[1]};
    o[(l2 ? F6I_HI2 : F6I_HI1) + e0] = __builtin_bit_cast(uint32_t, v);
  }
}

// the fp6 operands: one 32-lane group per (layer / group, m-tile, lane, term), lane e = element e (the one-thread-per-operand form took
// 29 us - two dependent chains of 32 scattered weight reads per thread - on every training iteration, whose weights change every step)
__global__ void k_pack_mlp_f6_frag(const float* __restrict__ w1, const float* __restrict__ w2, float* __restrict__ out) {
  uint32_t* o = (uint32_t*)out;
  const int item = blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5), e = threadIdx.x & 31;
  if (item >= (G6_1 + G6_2) * 4 * 64 * 2) return;
  const int term = item & 1, lane = (item >> 1) & 63, mt = (item >> 7) & 3, gg = item >> 9;
  const bool l2 = gg >= G6_1;
  const int grp = l2 ? gg - G6_1 : gg;
  const int k = f6_value(l2, grp, term, e);
  float w = 0.f;
  if (k >= 0) {
    _Float16 hi, lo;
    const float wf = mlp_weight_k(w1, w2, l2, k, lane, mt);
    split_weight(wf, hi, lo);
    w = term == 0 ? wf - (float)hi : (float)hi;   // term 0 carries the exact fp32 residual of the weight, term 1 a copy of its fp16 part
  }
  float amax = fabsf(w);
#pragma unroll
  for (int sh = 1; sh < 32; sh <<= 1) amax = fmaxf(amax, __shfl_xor(amax, sh, 32));
  int E = amax > 0.f ? ilogbf(amax) : -100;
  if (E < -100) E = -100;
  if (ldexpf(amax, 2 - E) > 7.75f) E += 1;          // the largest element would saturate: one binade up
  const float inv = ldexpf(1.0f, 2 - E);            // 1 / block scale, block scale = 2^(E - 2)
  const uint32_t c = e2m3_code(w * inv);
  const int bit = 6 * e, wi = bit >> 5, sh = bit & 31;
  uint32_t mine = 0;                                // after the reduction lane d < 6 holds dword d of the 192-bit operand
#pragma unroll
  for (int d = 0; d < 6; ++d) {
    uint32_t v = (d == wi ? c << sh : 0u) | ((d == wi + 1 && sh > 26) ? c >> (32 - sh) : 0u);
#pragma unroll
    for (int x = 1; x < 32; x <<= 1) v |= __shfl_xor(v, x, 32);
    if (e == d) mine = v;
  }
  uint32_t* q = o + (l2 ? F6I_Q2 : F6I_Q1) + (grp * 4 + mt) * 768 + lane * 4;
  if (e < 4) q[term * 256 + e] = mine;
  else if (e < 6) q[512 + 2 * term + (e - 4)] = mine;
  if (e == 0) {
    const int byte = (E - 2) + 127 - (term == 0 ? 2 : 13);
    ((uint8_t*)(o + F6I_SC + gg * 128))[lane * 8 + term * 4 + mt] = (uint8_t)(byte < 0 ? 0 : (byte > 254 ? 254 : byte));
  }
}

}  // namespace

extern "C" {

int64_t ego_packed_floats(void) { return 2 * (int64_t)PACKED_FLOATS + BASIS16_FLOATS + F8_FLOATS + F6_FLOATS; }

int64_t ego_packed_floats_scene(const ego_scene* sc) {
  if (!sc) return -1;
  return ego_shape_is_tuned(sc) ? ego_packed_floats() : ego_generic_packed_floats(sc);
}

int ego_pack_mlp(const ego_scene* sc, float* packed_out, void* stream) { return ego_pack_mlp_for(sc, packed_out, 0, stream); }

int64_t ego_packed_floats_compat(const ego_scene* sc) { return sc ? ego_generic_packed_floats(sc) : -1; }

int ego_pack_mlp_compat(const ego_scene* sc, float* packed_out, void* stream) {
  EGO_TRACE("ego_pack_mlp_compat");
  EGO_REQUIRE(sc && packed_out, "pack_mlp_compat: null argument");
  if (sc->head != EGO_HEAD_RGB)
    for (int i = 0; i < 3; ++i) EGO_REQUIRE(sc->mlp_w[i] && sc->mlp_b[i], "pack_mlp_compat: null MLP weight");
  EGO_REQUIRE(sc->basis[0] && sc->basis[1], "pack_mlp_compat: null basis matrix");
  return ego_generic_pack(sc, packed_out, stream);
}

int ego_pack_mlp_for(const ego_scene* sc, float* packed_out, int32_t for_training, void* stream) {
  EGO_TRACE("ego_pack_mlp_for");
  EGO_REQUIRE(sc && packed_out, "pack_mlp: null argument");
  if (sc->head != EGO_HEAD_RGB)   // RGBRender has no MLP (tensorBase.py:37-39): only the basis matrices are packed
    for (int i = 0; i < 3; ++i) EGO_REQUIRE(sc->mlp_w[i] && sc->mlp_b[i], "pack_mlp: null MLP weight");
  EGO_REQUIRE(sc->basis[0] && sc->basis[1], "pack_mlp: null basis matrix");
  if (!ego_shape_is_tuned(sc)) return ego_generic_pack(sc, packed_out, stream);   // any other shape: the fp32 compatibility kernels' layout
  k_pack_mlp<<<(PACKED_FLOATS + 255) / 256, 256, 0, (hipStream_t)stream>>>(sc->mlp_w[0], sc->mlp_b[0], sc->mlp_w[1], sc->mlp_b[1],
                                                                          sc->mlp_w[2], sc->mlp_b[2], sc->basis[0], sc->basis[1],
                                                                          packed_out);
  if (int e = ego_launch_status("k_pack_mlp")) return e;
  k_pack_mlp_h<<<(PACKED_FLOATS + 255) / 256, 256, 0, (hipStream_t)stream>>>(sc->mlp_w[0], sc->mlp_b[0], sc->mlp_w[1], sc->mlp_b[1],
                                                                            sc->mlp_w[2], sc->mlp_b[2], sc->basis[0], sc->basis[1],
                                                                            packed_out, packed_out + PACKED_FLOATS);
  if (int e = ego_launch_status("k_pack_mlp_h")) return e;
  k_pack_basis16<<<(BASIS16_FLOATS + 255) / 256, 256, 0, (hipStream_t)stream>>>(sc->basis[0], sc->basis[1], packed_out + 2 * PACKED_FLOATS);
  if (int e = ego_launch_status("k_pack_basis16")) return e;
  if (for_training) return EGO_OK;   // the f16f8 / f16f6 images below are read by the inference arithmetics only
  k_pack_mlp_f8<<<(F8_FLOATS + 255) / 256, 256, 0, (hipStream_t)stream>>>(sc->mlp_w[0], sc->mlp_w[1],
                                                                          packed_out + 2 * PACKED_FLOATS + BASIS16_FLOATS);
  if (int e = ego_launch_status("k_pack_mlp_f8")) return e;
  float* f6 = packed_out + 2 * PACKED_FLOATS + BASIS16_FLOATS + F8_FLOATS;
  if (const hipError_t err = hipMemsetAsync(f6, 0, sizeof(float) * F6_FLOATS, (hipStream_t)stream)) return (int)err;  // the gaps behind the blocks
  k_pack_mlp_f6<<<(F8_HI1 + F8_HI2 + 255) / 256, 256, 0, (hipStream_t)stream>>>(sc->mlp_w[0], sc->mlp_w[1], f6);
  if (int e = ego_launch_status("k_pack_mlp_f6")) return e;
  k_pack_mlp_f6_frag<<<((G6_1 + G6_2) * 4 * 64 * 2 + 7) / 8, 256, 0, (hipStream_t)stream>>>(sc->mlp_w[0], sc->mlp_w[1], f6);
  return ego_launch_status("k_pack_mlp_f6_frag");
}

}  // extern "C"
