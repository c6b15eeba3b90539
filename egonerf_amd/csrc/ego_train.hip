// libegonerf_hip.so: backward kernels of the training step and their entry points.
//
// Weight gradients are NOT reduced here: the kernels emit per-sample activation gradients in the same
// lane-contiguous order as the forward dumps and the host layer turns them into dW with plain library GEMMs
// (K = all samples of the step), then un-permutes the small result matrices (ego_train_layout tables).
#include "ego_tuned.h"

namespace {

// ---- transposed fragments for the data-gradient chain (fp16-split, same [step][tile][term][lane][8] order) ------
constexpr int T_W2T = 0;                                   // dH1 = W2^T dH2 : [8 steps][4 m-tiles]
constexpr int T_W1T = T_W2T + KH2 * 4 * 2 * 64 * 4;        // dX  = W1^T dH1 : [8 steps][5 m-tiles]   (16384)
constexpr int T_W3 = T_W1T + KH2 * 5 * 2 * 64 * 4;         // W3 in accumulator layout (fp32)         (+20480)
constexpr int T_BAST = T_W3 + 512;                          // dv  = B_g^T dfe: [2 g][2 steps][5 m-tiles]
constexpr int TRAIN_FLOATS = T_BAST + 2 * 2 * 5 * 2 * 64 * 4;
constexpr int TRAIN_LDS_FLOATS = T_BAST;                    // 37376 floats = 149504 B

__global__ void k_pack_train(const float* __restrict__ w1, const float* __restrict__ w2, const float* __restrict__ w3,
                             const float* __restrict__ basis_yin, const float* __restrict__ basis_yang, float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= TRAIN_FLOATS) return;
  if (idx >= T_W3 && idx < T_BAST) {
    const int e = idx - T_W3;
    const int c = e & 3, r = (e >> 2) & 15, h = (e >> 6) & 1, m = e >> 7;
    out[idx] = c < 3 ? w3[c * HID + m * 32 + slot_row(r, h)] : 0.f;
    return;
  }
  _Float16 pr[2];
  for (int p = 0; p < 2; ++p) {
    float w = 0.f;
    int term;
    if (idx < T_W1T) {  // [step][mt][term][lane][8]: A[i = out unit][k = in unit] = W2[in][out]
      const int hidx = (idx - T_W2T) * 2 + p;
      const int e = hidx & 7, lane = (hidx >> 3) & 63, mt = (hidx >> 10) & 3, step = hidx >> 12;
      term = (hidx >> 9) & 1;
      const int kk = step * 8 + e;
      const int in_unit = (kk >> 4) * 32 + slot_row(kk & 15, lane >> 5);
      w = w2[in_unit * HID + mt * 32 + (lane & 31)];
    } else if (idx < T_W3) {  // [step][t 0..4][term][lane][8]: row i of tile t <-> X register 16t + r(i) of half h(i)
      const int hidx = (idx - T_W1T) * 2 + p;
      const int e = hidx & 7, lane = (hidx >> 3) & 63, rest = hidx >> 10;  // rest = step * 5 + t
      term = (hidx >> 9) & 1;
      const int t = rest % 5, step = rest / 5;
      const int i = lane & 31, hi = (i >> 2) & 1, ri = (i & 3) + 4 * (i >> 3);
      const int ch = x_channel(16 * t + ri, hi);
      const int kk = step * 8 + e;
      const int unit = (kk >> 4) * 32 + slot_row(kk & 15, lane >> 5);
      if (ch >= 0) w = w1[unit * MLP_IN + ch];
    } else {  // [g][step 0..1][t 0..4][term][lane][8]: row <-> v register 16t + r(i) of half h(i); k = feature slot
      const int hidx = (idx - T_BAST) * 2 + p;
      const int e = hidx & 7, lane = (hidx >> 3) & 63, rest = hidx >> 10;  // rest = (g * 2 + step) * 5 + t
      term = (hidx >> 9) & 1;
      const int t = rest % 5, step = (rest / 5) & 1, g = rest / 10;
      const int i = lane & 31, hi = (i >> 2) & 1, ri = (i & 3) + 4 * (i >> 3);
      const int kv = 16 * t + ri;
      const int slot = step * 8 + e, f = 2 * slot + (lane >> 5);
      if (kv < KS_BASIS && slot < NSLOT && f < APP_DIM) w = (g ? basis_yang : basis_yin)[f * (3 * APP_C) + app_channel_g(kv, hi)];
    }
    _Float16 hi16, lo16;
    split_weight(w, hi16, lo16);
    pr[p] = term ? lo16 : hi16;
  }
  typedef _Float16 h2v __attribute__((ext_vector_type(2)));
  h2v v = {pr[0], pr[1]};
  out[idx] = __builtin_bit_cast(float, v);
}

struct GradField {
  float* plane[2][3];
  float* line[2][3];
};

struct ShadeBwdArgs {
  const float* tpacked;   // k_pack_train blob
  const float* coords;    // [M][4]
  float* dc;              // in: dL/d rgb_sample [M][3]; out: dL/d (pre-sigmoid output) [M][3]
  const float* rgb;       // [M][3] sigmoid outputs of the forward
  const float* fe;        // forward dump [tile][quad][lane][4]: the lane's feature slots (the encodings' derivative is re-derived from them)
  const uint32_t* bits;   // forward's ReLU masks [tile][layer][lane][2] (relu_bits)
  uint16_t* dh2;          // out, scaled fp16 [tile][k-step 0..7][lane][8]: the B operand (main term) of the next product as it is,
  uint16_t* dh1;          //   i.e. element e of step s of lane half h = logical column dump_col(8 s + e, h) of the [M][128] matrix
  float* dh_scale;        // out [2][ceil(M / 32) * 32]: dh2 (row 0) / dh1 (row 1) = fp16 payload * this per-sample power of two
  float* dfe;             // out [M][32]: dL/d(feature slots) of the sample's own grid, half h at +16h
  float* dv;              // out, ceil(M/32)*32 rows: dL/d(plane x line products), [tile][plane*3+line][sample][16] (feeds k_vm_scatter)
  uint32_t* dv_absmax;    // out (optional): max |dv| over the valid samples as float bits, by atomicMax (zeroed by the launcher): the
                          // bound the fused sorted scatter derives its fixed-point unit from, so that it need not read dv once more
  int64_t M;
};

// Gradients are small (1e-8 .. 1e-3) and would fall into / below fp16's subnormal range in the fp16 split, so each
// sample's operand vector is scaled by an exact power of two that brings its largest magnitude to [2^12, 2^13).
// A lane supplies only its own sample's column of B and receives the same column of D, so the scale commutes with
// the product; both lanes of a sample (l, l^32) must agree on it.
// inv_dump (optional): what goes into dh_scale - inv, but 0 for a sample whose vector is all zero (scale 1 there): the weight-gradient
// pass takes the LARGEST scale of a 32-sample step as its reference (k_wgrad_h), and a 1.0 standing for "nothing" next to real scales
// of 2^-20 would flush the whole step
__device__ __forceinline__ float sample_scale(float amax, float& inv, float* inv_dump = nullptr) {
  amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
  const int e = (__float_as_int(amax) >> 23) & 0xff;  // biased exponent; 0 for zero / fp32 subnormals
  const int k = (e == 0 || e > 254) ? 0 : 139 - e;    // 2^k * amax in [2^12, 2^13)
  const int kc = k > 100 ? 100 : (k < -100 ? -100 : k);
  inv = __int_as_float((127 - kc) << 23);
  if (inv_dump) *inv_dump = (e == 0 || e > 254) ? 0.f : inv;
  return __int_as_float((127 + kc) << 23);
}

// split8 with the main term rounded to nearest (v_cvt_pk_f16_f32) instead of truncated: the main term is also what the kernel
// stores for the weight-gradient pass, where a truncation bias (always towards zero, 2^-12 on average) would not average out over
// the samples while a rounding error does
__device__ __forceinline__ HL split8_rn(const float x[8]) {
  typedef float f2v __attribute__((ext_vector_type(2)));
  typedef _Float16 h2v __attribute__((ext_vector_type(2)));
  u32x4 hi, lo;
  float neg1 = -1.0f;
  asm("" : "+v"(neg1));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float a = x[2 * q], b = x[2 * q + 1];
    const h2v hp = __builtin_convertvector(f2v{a, b}, h2v);
    hi[q] = __builtin_bit_cast(uint32_t, hp);
    const float ra = __builtin_fmaf((float)hp[0], neg1, a), rb = __builtin_fmaf((float)hp[1], neg1, b);
    lo[q] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(ra, rb));
  }
  HL o;
  o.hi = __builtin_bit_cast(h8, hi);
  o.lo = __builtin_bit_cast(h8, lo);
  return o;
}

template <int NT>
__device__ __forceinline__ float tiles_amax(const f32x16* v) {
  float m = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, fabsf(v[t][r]));
  return m;
}

// one f16x3 matrix step: acc[t] += A(step, t) * b for NT m-tiles; A fragments [step][t][term][lane] as u32x4
template <int NT>
__device__ __forceinline__ void mfma_step(const u32x4* __restrict__ A, int step, int lw, const HL& b, f32x16* acc) {
  h8 ah[NT], al[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    ah[t] = __builtin_bit_cast(h8, A[((step * NT + t) * 2 + 0) * 64 + lw]);
    al[t] = __builtin_bit_cast(h8, A[((step * NT + t) * 2 + 1) * 64 + lw]);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = MFMAH(ah[t], b.hi, acc[t]);
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = MFMAH(al[t], b.hi, acc[t]);
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = MFMAH(ah[t], b.lo, acc[t]);
}

__global__ __launch_bounds__(512) void k_shade_bwd(ShadeBwdArgs A) {
  __shared__ __attribute__((aligned(16))) float lds[TRAIN_LDS_FLOATS];
  {
    const f32x4* src = (const f32x4*)A.tpacked;
    f32x4* dst = (f32x4*)lds;
    for (int i = threadIdx.x; i < TRAIN_LDS_FLOATS / 4; i += 512) dst[i] = src[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int64_t n_tiles = (A.M + 31) >> 5;
  const u32x4* W2T = (const u32x4*)(lds + T_W2T);
  const u32x4* W1T = (const u32x4*)(lds + T_W1T);
  const f32x4* W3 = (const f32x4*)(lds + T_W3);
  const u32x4* BAST = (const u32x4*)(A.tpacked + T_BAST);

  float dvmax = 0.f;   // running max |dv| of this wave's valid samples
  uint32_t dvbad = 0;  // NaN bits once a valid sample's feature gradient is not finite (its dv is NaN then; fmaxf would drop it)
  for (int64_t tile = (int64_t)blockIdx.x * 8 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 8) {
    int lw = lane;
    asm volatile("" : "+v"(lw));
    const int hw = lw >> 5;
    const int64_t m_raw = tile * 32 + j;
    const bool valid = m_raw < A.M;
    const int64_t m = valid ? m_raw : A.M - 1;

    // d(pre-sigmoid output)
    float d0, d1, d2;
    {
      const float* dc = A.dc + m * 3;
      const float* c = A.rgb + m * 3;
      d0 = valid ? dc[0] * c[0] * (1.f - c[0]) : 0.f;
      d1 = valid ? dc[1] * c[1] * (1.f - c[1]) : 0.f;
      d2 = valid ? dc[2] * c[2] * (1.f - c[2]) : 0.f;
    }
    // dH2 = (H2 > 0) * W3^T do, in accumulator layout == the B-operand K order of the next product
    f32x16 dH2[4];
    {
      const u32x2 on = ((const u32x2*)A.bits)[(tile * 2 + 1) * 64 + lane];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const f32x4 w = W3[(mt * 2 + hw) * 16 + r];
          dH2[mt][r] = ((on[mt >> 1] >> (16 * (mt & 1) + r)) & 1u) ? fmaf(w.x, d0, fmaf(w.y, d1, w.z * d2)) : 0.f;
        }
    }
    // both lanes of a sample read dc[m] in the same load above (d0..d2 depend on it), so the overwrite is ordered
    if (valid && h == 0) { float* o = A.dc + m * 3; o[0] = d0; o[1] = d1; o[2] = d2; }

    // dH1 = (H1 > 0) * W2^T dH2
    f32x16 dH1[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) dH1[mt][r] = 0.f;
    {
      float inv, inv_d;
      const float sc = sample_scale(tiles_amax<4>(dH2), inv, &inv_d);
      if (valid && h == 0) A.dh_scale[m] = inv_d;
#pragma unroll
      for (int step = 0; step < KH2; ++step) {
        float xs[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) xs[e] = dH2[(step * 8 + e) >> 4][(step * 8 + e) & 15] * sc;
        const HL b = split8_rn(xs);
        // the main term IS the dump: dh2 = fp16 payload * inv to 2^-12 (half the bytes of an fp32 dump, no conversion of its own)
        if (valid) ((u32x4*)A.dh2)[(tile * 8 + step) * 64 + lane] = __builtin_bit_cast(u32x4, b.hi);   // (cached: the weight-gradient passes read it next; nontemporal cost them 1-2 %)
        mfma_step<4>(W2T, step, lw, b, dH1);
      }
      const u32x2 on = ((const u32x2*)A.bits)[(tile * 2 + 0) * 64 + lane];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dH1[mt][r] = ((on[mt >> 1] >> (16 * (mt & 1) + r)) & 1u) ? dH1[mt][r] * inv : 0.f;
    }

    // dX = W1^T dH1: 5 output tiles = this lane half's 80 layer-1 input registers
    f32x16 dX[5];
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) dX[t][r] = 0.f;
    float inv_x;
    {
      float inv_xd;
      const float sc = sample_scale(tiles_amax<4>(dH1), inv_x, &inv_xd);
      if (valid && h == 0) A.dh_scale[((A.M + 31) & ~(int64_t)31) + m] = inv_xd;
#pragma unroll
      for (int step = 0; step < KH2; ++step) {
        float xs[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) xs[e] = dH1[(step * 8 + e) >> 4][(step * 8 + e) & 15] * sc;
        const HL b = split8_rn(xs);
        if (valid) ((u32x4*)A.dh1)[(tile * 8 + step) * 64 + lane] = __builtin_bit_cast(u32x4, b.hi);
        mfma_step<5>(W1T, step, lw, b, dX);
      }
    }

    // through the positional encoding: slot r holds (f, sin f, sin 2f, cos f, cos 2f) at X registers 5r .. 5r+4
    float dfe[16];
    {
      float fwd_fe[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 t = ((const f32x4*)A.fe)[(tile * 4 + q) * 64 + lane];
        fwd_fe[4 * q] = t.x; fwd_fe[4 * q + 1] = t.y; fwd_fe[4 * q + 2] = t.z; fwd_fe[4 * q + 3] = t.w;
      }
#pragma unroll
      for (int r = 0; r < NSLOT; ++r) {
        // the forward's own sine / cosine instructions on the forward's own feature value: bit-identical encodings, nothing read back
        float s1, c1, s2, c2;
        sincos_x_2x_hw(fwd_fe[r], s1, c1, s2, c2);
#define DXK(kk) dX[(kk) >> 4][(kk) & 15]
        dfe[r] = (DXK(5 * r) + DXK(5 * r + 1) * c1 + 2.f * DXK(5 * r + 2) * c2 - DXK(5 * r + 3) * s1 - 2.f * DXK(5 * r + 4) * s2) * inv_x;
#undef DXK
      }
      dfe[14] = 0.f; dfe[15] = 0.f;
    }
    const f32x4 cc = ((const f32x4*)A.coords)[m];
    const int g = cc.w != 0.f;
    if (valid) {   // 32 columns per sample (its own grid's); the weight-gradient pass routes them to the yin / yang block by coords.w
      f32x4* o = (f32x4*)(A.dfe + m * 32 + hw * 16);
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = f32x4{dfe[4 * q], dfe[4 * q + 1], dfe[4 * q + 2], dfe[4 * q + 3]};   // (an instruction writes quarter lines here and in dv below: not nontemporal)
    }

    if (!A.dv) {   // v16: nobody reads dv - ego_scatter_app_sorted re-derives it from dfe in its walk; it only needs max |dfe| for its scale
      uint32_t amu = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) amu = max(amu, __float_as_uint(dfe[r]) & 0x7fffffffu);
      if (valid) dvbad = max(dvbad, amu);   // (raw bits: a NaN / Inf stays above every finite value)
      continue;
    }
    // dv = B_g^T dfe (K = 16 slots per lane half = 2 steps); border-straddling waves run both weight sets masked
    f32x16 dV[5];
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) dV[t][r] = 0.f;
    const bool any_yin = __ballot(g == 0) != 0ull, any_yang = __ballot(g != 0) != 0ull;
    float inv_v;
    {
      float am = 0.f;
      uint32_t amu = 0;   // the same maximum over the raw bits: fmaxf drops a NaN, this keeps it (a NaN / Inf compares above every finite value)
#pragma unroll
      for (int r = 0; r < 16; ++r) { am = fmaxf(am, fabsf(dfe[r])); amu = max(amu, __float_as_uint(dfe[r]) & 0x7fffffffu); }
      if (valid && amu >= 0x7f800000u) dvbad = 0x7fc00000u;
      const float sc = sample_scale(am, inv_v);
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) ds[r] = dfe[r] * sc;
      if (any_yin) {
        mfma_step<5>(BAST, 0, lw, split8(ds, g == 0), dV);
        mfma_step<5>(BAST, 1, lw, split8(ds + 8, g == 0), dV);
      }
      if (any_yang) {
        mfma_step<5>(BAST + 2 * 5 * 2 * 64, 0, lw, split8(ds, g != 0), dV);
        mfma_step<5>(BAST + 2 * 5 * 2 * 64, 1, lw, split8(ds + 8, g != 0), dV);
      }
    }

    // dv, tile-blocked for the scatter kernel: [tile][plane * 3 + line i][sample j][16 channels of the line] (channel
    // 16 i + 4 (h + 2 half) + c of the plane, K order app_channel_g), so the two lanes of a sample fill whole 64-byte lines
    // of a 2 KB block and the scatter's 16 channel-lanes read one line per sample.  fp32: a scaled-fp16 dv (like dh2 / dh1) was
    // built and measured - no faster (the scatter is not bound by these bytes) and its 2^-12 rounding shows in table texels that
    // only a few samples touch (2-3e-4 of the largest gradient against the reference's autograd; tolerance 2e-4), DESIGN.md 4.2
    if (valid) {
      float am = 0.f;   // the 72 values this lane stores (kv = pl * APP_HALF + half * 12 + i * 4 + c) are exactly dV's first 72 K slots
#pragma unroll
      for (int kv = 0; kv < 3 * APP_HALF; ++kv) am = fmaxf(am, fabsf(dV[kv >> 4][kv & 15]));
      dvmax = fmaxf(dvmax, am * inv_v);   // inv_v is a power of two: |x| * inv_v == |x * inv_v|
      float* o = A.dv + tile * (32 * 3 * APP_C) + j * 16;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const int kv = pl * APP_HALF + half * 12 + i * 4;
            *(f32x4*)(o + (pl * 3 + i) * 512 + 4 * (hw + 2 * half)) =
                f32x4{dV[kv >> 4][kv & 15], dV[(kv + 1) >> 4][(kv + 1) & 15], dV[(kv + 2) >> 4][(kv + 2) & 15],
                      dV[(kv + 3) >> 4][(kv + 3) & 15]} * inv_v;
          }
    }
  }
  if (A.dv_absmax) {   // one atomic per wave (2 048 per launch); a NaN's bits compare above every finite value, as the consumer expects
    uint32_t mb = max(__float_as_uint(dvmax) & 0x7fffffffu, dvbad);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mb = max(mb, (uint32_t)__shfl_xor((int)mb, d, 64));
    // (atomics on one address serialise at ~150 ns each: a wave sends its maximum only while it would still raise the value)
    if (lane == 0 && mb > __hip_atomic_load(A.dv_absmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(A.dv_absmax, mb);
  }
}

// ---- compositing + density backward: one wave per ray, lane = sample -------------------------------------------
struct MarchBwdArgs {
  const float* z;        // [N][S]
  const float* alpha;    // [N][S] (row stride astride)
  const float* g_alpha;  // dL/d alpha, same stride, or null
  const float* weight;   // [N][S]
  const float* sigma;    // [N][S]
  const float* bg;       // [N] final transmittance
  const float* rgb;      // [N][S][3] per-sample colours of the forward
  const float* g_rgb;    // [N][3] dL/d rgb_map (after the clamp)
  const float* rgb_raw;  // [N][3] rgb_map before the clamp
  const float* env;      // [N][3] background radiance or null
  float* dc;             // out [N][S][3] = weight * g
  float* dfeat;          // out [N][S] = dL/d(density feature), before the per-plane relu mask (feeds k_vm_scatter)
  int64_t N;
  int32_t S;
  int32_t astride;
  float dscale;
};

__global__ __launch_bounds__(256) void k_march_bwd(MarchBwdArgs A) {
#pragma clang fp contract(fast)
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (ray >= A.N) return;
  const int S = A.S;
  float g[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float raw = A.rgb_raw[ray * 3 + c];
    g[c] = (raw >= 0.f && raw <= 1.f) ? A.g_rgb[ray * 3 + c] : 0.f;  // clamp(0,1) backward (inclusive, like torch)
  }
  const float T_end = A.bg[ray];
  const float dT_end = A.env ? (g[0] * A.env[ray * 3] + g[1] * A.env[ray * 3 + 1] + g[2] * A.env[ray * 3 + 2]) : 0.f;
  // pass 1 (forward over the ray): exclusive transmittance T_s, parked in dc[.][0]
  {
    float carryT = 1.f;
    for (int s0 = 0; s0 < S; s0 += 64) {
      const int s = s0 + lane;
      const bool ok = s < S;
      const float a = ok ? A.alpha[ray * A.astride + s] : 0.f;
      const float t = ok ? __fadd_rn(__fsub_rn(1.f, a), 1e-10f) : 1.f;
      const float incT = wave_scan_mul(t, lane);
      float excT = __shfl_up(incT, 1, 64);
      if (lane == 0) excT = 1.f;
      if (ok) A.dc[(ray * S + s) * 3] = carryT * excT;
      carryT *= __shfl(incT, 63, 64);
    }
  }
  // pass 2 (backward over the ray): R_s = sum_{k>s} (g . c_k) w_k + dT_end T_end as a true suffix sum.  (total - prefix
  // would cancel catastrophically exactly where it is then divided by t_s ~ 1e-10, i.e. behind opaque samples.)
  float carryR = dT_end * T_end;
  const int n_chunks = (S + 63) >> 6;
  for (int ch = n_chunks - 1; ch >= 0; --ch) {
    const int s0 = ch << 6;
    const int s = min(s0 + lane, S - 1);
    const bool ok = (s0 + lane) < S;
    const int64_t o = ray * S + s;
    const float a = ok ? A.alpha[ray * A.astride + s] : 0.f;
    const float t = __fadd_rn(__fsub_rn(1.f, a), 1e-10f);
    const float* c = A.rgb + o * 3;
    const float gc = g[0] * c[0] + g[1] * c[1] + g[2] * c[2];
    const float w = ok ? A.weight[o] : 0.f;
    const float q = gc * w;
    float incQ = q;  // inclusive suffix within the chunk
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float v = __shfl_down(incQ, d, 64);
      if (lane + d < 64) incQ += v;
    }
    const float R = carryR + (incQ - q);
    const float T = ok ? A.dc[o * 3] : 0.f;
    const float dalpha = gc * T - R / t + ((A.g_alpha && ok) ? A.g_alpha[ray * A.astride + s] : 0.f);
    const int sn = (s < S - 1) ? s + 1 : s - 1;
    const float zz = A.z[o], zn = A.z[ray * S + sn];
    const float dist = (s < S - 1) ? __fsub_rn(zn, zz) : __fsub_rn(zz, zn);
    const float sg = A.sigma[o];
    const float dsigma = dalpha * (1.f - a) * __fmul_rn(dist, A.dscale);
    const float df = ok ? dsigma * (1.f - expf(-sg)) : 0.f;  // softplus'(x) = sigmoid(x) = 1 - exp(-softplus(x))
    if (ok) {
      float* dc = A.dc + o * 3;
      dc[0] = w * g[0]; dc[1] = w * g[1]; dc[2] = w * g[2];
    }
    carryR += __shfl(incQ, 0, 64);
    if (ok) A.dfeat[o] = df;
  }
}

// ---- table-gradient scatter: lane = channel, so every atomic instruction covers whole 64-B lines -----------------------
// Float atomics on MI355X are bound by LINE requests at L2 (~21 G lines/s measured, tools/atomic_probe.hip), however many of
// a line's 16 dwords one instruction carries: 21 G atomics/s with one lane per line, 330 G/s with 16.  So the scatter
// runs with 16 lanes = the 16 channels of one 64-B line and 4 samples per wave instruction.  Each 16-lane group walks SEG
// consecutive samples of one ray and keeps per-tap sums in registers while the texel cell stays the same (consecutive
// samples of a ray move by a fraction of a texel), flushing one coalesced atomic per (cell, tap, line) when it changes —
// a run-length merge with no cross-lane traffic.
struct ScatterArgs {
  DevField F;
  GradField G;
  const float* coords;  // [N][S][4] normalised (r, theta, phi, grid) of the forward
  const float* d;       // DENS: dfeat [N][S]; else k_shade_bwd's dv ([tile of 32 samples][plane * 3 + line][sample][16])
  int64_t N;
  int32_t S, seg, gpr;  // samples per group, groups per ray
};

// one (segment, plane I) per 16-lane group: 18 (C = 48) accumulators, so the kernel runs at full occupancy
template <int C, bool DENS, int I>
__device__ __forceinline__ void scatter_plane(const ScatterArgs& A) {
#pragma clang fp contract(fast)
  constexpr int NL = C / 16;
  const int lane = threadIdx.x & 63, c16 = lane & 15;
  const int64_t grp = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
  const int64_t ray = grp / A.gpr;
  const int s_begin = (int)(grp % A.gpr) * A.seg;
  const int s_end = ray < A.N ? min(A.S, s_begin + A.seg) : s_begin;
  const int W = A.F.res[vm_plane_x(I)];
  // current cell: grid and the clamped tap indices (both i0 and i1: at the table border i0 alone does not identify the taps)
  int curG = -1, curX = 0, curX1 = 0, curY = 0, curY1 = 0, curLg = -1, curLi = 0, curLi1 = 0;
  int oP[4] = {0, 0, 0, 0}, oL[2] = {0, 0};
  float accP[NL][4], accL[NL][2];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
#pragma unroll
    for (int t = 0; t < 4; ++t) accP[i][t] = 0.f;
    accL[i][0] = accL[i][1] = 0.f;
  }
  // taps t: 0 = (y0, x0), 1 = (y0, x1), 2 = (y1, x0), 3 = (y1, x1).  flush_col(k) sends the x_k column
  auto flush_col = [&](int gsel, int k) {
    float* GP = (gsel ? A.G.plane[1][I] : A.G.plane[0][I]) + c16;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      if (k == 0) {
        if (accP[i][0] != 0.f) unsafeAtomicAdd(GP + oP[0] + 16 * i, accP[i][0]);
        if (accP[i][2] != 0.f) unsafeAtomicAdd(GP + oP[2] + 16 * i, accP[i][2]);
      } else {
        if (accP[i][1] != 0.f) unsafeAtomicAdd(GP + oP[1] + 16 * i, accP[i][1]);
        if (accP[i][3] != 0.f) unsafeAtomicAdd(GP + oP[3] + 16 * i, accP[i][3]);
      }
    }
  };
  auto flush_tap = [&](int gsel, int t) {
    float* GL = (gsel ? A.G.line[1][I] : A.G.line[0][I]) + c16;
#pragma unroll
    for (int i = 0; i < NL; ++i)
      if (accL[i][t] != 0.f) unsafeAtomicAdd(GL + oL[t] + 16 * i, accL[i][t]);
  };
  for (int s = s_begin; s < s_end; ++s) {
    const int64_t m = ray * A.S + s;
    float dsample = 0.f;
    if (DENS) {
      dsample = A.d[m];
      if (dsample == 0.f) continue;  // uniform over the 16-lane group
    }
    const f32x4 cc = ((const f32x4*)A.coords)[m];
    const int g = cc.w != 0.f;
    const float ax[3] = {cc.x, cc.y, cc.z};
    const Lin1 X = lin_setup(ax[vm_plane_x(I)], A.F.res[vm_plane_x(I)]), Y = lin_setup(ax[vm_plane_y(I)], A.F.res[vm_plane_y(I)]),
               Ln = lin_setup(ax[vm_line_ax(I)], A.F.res[vm_line_ax(I)]);
    // the x axis of planes 0/1 (and line 2) is r, which crosses a texel every ~2 samples: when the cell moves by one in x the
    // shared tap column keeps accumulating and only the column left behind is sent
    if (!(g == curG && Y.i0 == curY && Y.i1 == curY1 && X.i0 == curX && X.i1 == curX1)) {
      const bool same_row = g == curG && Y.i0 == curY && Y.i1 == curY1;
      if (same_row && X.i0 == curX + 1 && X.i0 == curX1) {
        flush_col(curG, 0);
#pragma unroll
        for (int i = 0; i < NL; ++i) { accP[i][0] = accP[i][1]; accP[i][2] = accP[i][3]; accP[i][1] = 0.f; accP[i][3] = 0.f; }
        oP[0] = oP[1]; oP[2] = oP[3];
        oP[1] = (Y.i0 * W + X.i1) * C; oP[3] = (Y.i1 * W + X.i1) * C;
      } else if (same_row && X.i1 == curX && X.i0 == curX - 1) {
        flush_col(curG, 1);
#pragma unroll
        for (int i = 0; i < NL; ++i) { accP[i][1] = accP[i][0]; accP[i][3] = accP[i][2]; accP[i][0] = 0.f; accP[i][2] = 0.f; }
        oP[1] = oP[0]; oP[3] = oP[2];
        oP[0] = (Y.i0 * W + X.i0) * C; oP[2] = (Y.i1 * W + X.i0) * C;
      } else {
        if (curG >= 0) { flush_col(curG, 0); flush_col(curG, 1); }
#pragma unroll
        for (int i = 0; i < NL; ++i) { accP[i][0] = 0.f; accP[i][1] = 0.f; accP[i][2] = 0.f; accP[i][3] = 0.f; }
        oP[0] = (Y.i0 * W + X.i0) * C; oP[1] = (Y.i0 * W + X.i1) * C;
        oP[2] = (Y.i1 * W + X.i0) * C; oP[3] = (Y.i1 * W + X.i1) * C;
      }
      curG = g; curX = X.i0; curX1 = X.i1; curY = Y.i0; curY1 = Y.i1;
    }
    if (!(g == curLg && Ln.i0 == curLi && Ln.i1 == curLi1)) {
      if (g == curLg && Ln.i0 == curLi + 1 && Ln.i0 == curLi1) {
        flush_tap(curLg, 0);
#pragma unroll
        for (int i = 0; i < NL; ++i) { accL[i][0] = accL[i][1]; accL[i][1] = 0.f; }
        oL[0] = oL[1]; oL[1] = Ln.i1 * C;
      } else if (g == curLg && Ln.i1 == curLi && Ln.i0 == curLi - 1) {
        flush_tap(curLg, 1);
#pragma unroll
        for (int i = 0; i < NL; ++i) { accL[i][1] = accL[i][0]; accL[i][0] = 0.f; }
        oL[1] = oL[0]; oL[0] = Ln.i0 * C;
      } else {
        if (curLg >= 0) { flush_tap(curLg, 0); flush_tap(curLg, 1); }
#pragma unroll
        for (int i = 0; i < NL; ++i) { accL[i][0] = 0.f; accL[i][1] = 0.f; }
        oL[0] = Ln.i0 * C; oL[1] = Ln.i1 * C;
      }
      curLg = g; curLi = Ln.i0; curLi1 = Ln.i1;
    }
    const float* P = (g ? A.F.plane[1][I] : A.F.plane[0][I]) + c16;
    const float* L = (g ? A.F.line[1][I] : A.F.line[0][I]) + c16;
    const float w00 = __fmul_rn(Y.w0, X.w0), w01 = __fmul_rn(Y.w0, X.w1), w10 = __fmul_rn(Y.w1, X.w0), w11 = __fmul_rn(Y.w1, X.w1);
    float pv[NL], lv[NL], di[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      pv[i] = P[oP[0] + 16 * i] * w00 + P[oP[1] + 16 * i] * w01 + P[oP[2] + 16 * i] * w10 + P[oP[3] + 16 * i] * w11;
      lv[i] = L[oL[0] + 16 * i] * Ln.w0 + L[oL[1] + 16 * i] * Ln.w1;
    }
    if (DENS) {
      float dot = pv[0] * lv[0];  // C == 16: one line; relu per plane (EgoNeRF.py:340,346)
#pragma unroll
      for (int sh = 8; sh >= 1; sh >>= 1) dot += __shfl_xor(dot, sh, 16);
      di[0] = dot > 0.f ? dsample : 0.f;
    } else {
#pragma unroll
      for (int i = 0; i < NL; ++i) di[i] = A.d[(m >> 5) * (32 * 3 * C) + (I * NL + i) * 512 + (m & 31) * 16 + c16];  // k_shade_bwd's blocked dv
    }
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const float gp = di[i] * lv[i], gl = di[i] * pv[i];
      accP[i][0] += gp * w00; accP[i][1] += gp * w01; accP[i][2] += gp * w10; accP[i][3] += gp * w11;
      accL[i][0] += gl * Ln.w0; accL[i][1] += gl * Ln.w1;
    }
  }
  if (curG >= 0) { flush_col(curG, 0); flush_col(curG, 1); }
  if (curLg >= 0) { flush_tap(curLg, 0); flush_tap(curLg, 1); }
}

template <int C, bool DENS>
__global__ __launch_bounds__(256) void k_vm_scatter(ScatterArgs A) {
  if (blockIdx.y == 0) scatter_plane<C, DENS, 0>(A);
  else if (blockIdx.y == 1) scatter_plane<C, DENS, 1>(A);
  else scatter_plane<C, DENS, 2>(A);
}

}  // namespace

extern "C" {

int64_t ego_train_packed_floats(void) { return TRAIN_FLOATS; }

int ego_pack_train(const ego_scene* sc, float* out, void* stream) {
  EGO_TRACE("ego_pack_train");
  EGO_REQUIRE(sc && out, "pack_train: null argument");
  if (int e = check_shade_config(sc, "pack_train", true, true)) return e;
  EGO_REQUIRE(sc->mlp_w[0] && sc->mlp_w[1] && sc->mlp_w[2] && sc->basis[0] && sc->basis[1], "pack_train: null weight");
  k_pack_train<<<(TRAIN_FLOATS + 255) / 256, 256, 0, (hipStream_t)stream>>>(sc->mlp_w[0], sc->mlp_w[1], sc->mlp_w[2], sc->basis[0],
                                                                            sc->basis[1], out);
  return ego_launch_status("k_pack_train");
}

int ego_train_layout(int32_t which, int32_t* out, int32_t n) {
  EGO_REQUIRE(out, "train_layout: null output");
  if (which == 0) {  // x dump column -> reference MLP input column (-1: padding)
    EGO_REQUIRE(n == 2 * KS1, "train_layout(0): n must be 160");
    for (int h = 0; h < 2; ++h)
      for (int kk = 0; kk < KS1; ++kk) out[dump_col(kk, h)] = x_channel(kk, h);
  } else if (which == 1) {  // h1 / h2 / dh1 / dh2 dump column -> hidden unit
    EGO_REQUIRE(n == HID, "train_layout(1): n must be 128");
    for (int h = 0; h < 2; ++h)
      for (int mt = 0; mt < 4; ++mt)
        for (int r = 0; r < 16; ++r) out[dump_col(mt * 16 + r, h)] = mt * 32 + slot_row(r, h);
  } else if (which == 2) {  // dfe column (within one grid's 32) -> feature (-1: padding)
    EGO_REQUIRE(n == 32, "train_layout(2): n must be 32");
    for (int h = 0; h < 2; ++h)
      for (int r = 0; r < 16; ++r) out[h * 16 + r] = (r < NSLOT && 2 * r + h < APP_DIM) ? 2 * r + h : -1;
  } else if (which == 3) {  // v dump column -> basis input column (0..143)
    EGO_REQUIRE(n == 2 * KS_BASIS, "train_layout(3): n must be 144");
    for (int h = 0; h < 2; ++h)
      for (int kk = 0; kk < KS_BASIS; ++kk) out[dump_col(kk, h)] = app_channel_g(kk, h);
  } else {
    return ego_fail(EGO_E_BADARG, "train_layout: which must be 0..3");
  }
  return EGO_OK;
}

static GradField make_grad(const ego_vm_grad& g) {
  GradField o;
  for (int a = 0; a < 2; ++a)
    for (int i = 0; i < 3; ++i) { o.plane[a][i] = g.plane[a][i]; o.line[a][i] = g.line[a][i]; }
  return o;
}

static int check_grad(const ego_vm_grad* g, const char* who) {
  if (!g) return ego_fail(EGO_E_BADARG, "%s: null gradient tables", who);
  for (int a = 0; a < 2; ++a)
    for (int i = 0; i < 3; ++i)
      if (!g->plane[a][i] || !g->line[a][i]) return ego_fail(EGO_E_BADARG, "%s: null gradient table pointer", who);
  return EGO_OK;
}

int ego_march_backward(const ego_scene* sc, const float* z, const float* alpha, int32_t alpha_stride, const float* weight,
                       const float* sigma, const float* bg_weight, const float* rgb, const float* g_rgb, const float* g_alpha,
                       const float* rgb_raw, const float* env_map, int64_t N, int32_t S, float* dc, float* dfeat, void* stream) {
  EGO_TRACE("ego_march_backward");
  EGO_REQUIRE(N >= 0 && S >= 2 && alpha_stride >= S, "march_backward: bad size");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(sc && z && alpha && weight && sigma && bg_weight && rgb && g_rgb && rgb_raw && dc && dfeat, "march_backward: null argument");
  if (!sc->act_softplus) return ego_fail(EGO_E_UNSUPPORTED, "march_backward: only the softplus density activation is supported");
  MarchBwdArgs a{};
  a.z = z; a.alpha = alpha; a.g_alpha = g_alpha; a.astride = alpha_stride; a.weight = weight; a.sigma = sigma;
  a.bg = bg_weight; a.rgb = rgb; a.g_rgb = g_rgb;
  a.rgb_raw = rgb_raw; a.env = env_map; a.dc = dc; a.dfeat = dfeat; a.N = N; a.S = S; a.dscale = sc->distance_scale;
  k_march_bwd<<<(unsigned)((N + 3) / 4), 256, 0, (hipStream_t)stream>>>(a);
  return ego_launch_status("k_march_bwd");
}

int ego_shade_backward(const ego_scene* sc, const float* train_packed, const float* coords, float* dc, const float* rgb,
                       const ego_shade_dump* fwd, uint16_t* dh2, uint16_t* dh1, float* dh_scale, float* dfe, float* dv, float* dv_absmax, int64_t N,
                       int32_t S, void* stream) {
  EGO_TRACE("ego_shade_backward");
  EGO_REQUIRE(N >= 0 && S >= 1 && N * (int64_t)S < (1ll << 31), "shade_backward: bad size");
  if (N == 0) {
    if (dv_absmax)
      if (const hipError_t me = hipMemsetAsync(dv_absmax, 0, 4, (hipStream_t)stream)) return ego_fail((int)me, "shade_backward: hipMemsetAsync failed: %s", hipGetErrorString(me));
    return EGO_OK;
  }
  EGO_REQUIRE(sc && train_packed && coords && dc && rgb && fwd && fwd->fe && fwd->relu_bits && dh2 && dh1 && dh_scale && dfe && (dv || dv_absmax),
              "shade_backward: null argument");
  EGO_REQUIRE((((uintptr_t)dh2 | (uintptr_t)dh1 | (uintptr_t)fwd->relu_bits | (uintptr_t)dv) & 15) == 0,
              "shade_backward: dh2 / dh1 / dv / relu_bits must be 16-byte aligned");
  if (int e = check_shade_config(sc, "shade_backward", true, true)) return e;
  ShadeBwdArgs a{};
  a.tpacked = train_packed; a.coords = coords; a.dc = dc; a.rgb = rgb;
  a.fe = fwd->fe; a.bits = fwd->relu_bits; a.dh2 = dh2; a.dh1 = dh1; a.dh_scale = dh_scale; a.dfe = dfe; a.dv = dv; a.M = N * (int64_t)S;
  a.dv_absmax = (uint32_t*)dv_absmax;
  if (dv_absmax)
    if (const hipError_t me = hipMemsetAsync(dv_absmax, 0, 4, (hipStream_t)stream)) return ego_fail((int)me, "shade_backward: hipMemsetAsync failed: %s", hipGetErrorString(me));
  k_shade_bwd<<<shade_grid(a.M), 512, 0, (hipStream_t)stream>>>(a);
  return ego_launch_status("k_shade_bwd");
}

static int scatter_common(const ego_vm_field& f, const ego_vm_grad* g, const float* coords, const float* d, int64_t N, int32_t S,
                          ScatterArgs* a, const char* who) {
  if (!(N >= 0 && S >= 1)) return ego_fail(EGO_E_BADARG, "%s: bad size", who);
  if (N == 0) return EGO_OK;
  if (!coords || !d) return ego_fail(EGO_E_BADARG, "%s: null argument", who);
  if (int e = check_grad(g, who)) return e;
  a->F = make_field(f); a->G = make_grad(*g); a->coords = coords; a->d = d; a->N = N; a->S = S;
  a->seg = 64;
  a->gpr = (S + a->seg - 1) / a->seg;
  return EGO_OK;
}

static dim3 scatter_blocks(const ScatterArgs& a) {
  const int64_t groups = a.N * a.gpr;
  return dim3((unsigned)((groups + 15) / 16), 3);  // 4 groups per wave, 4 waves per workgroup; y = plane
}

int ego_scatter_density(const ego_scene* sc, const ego_vm_grad* gdensity, const float* coords, const float* dfeat, int64_t N, int32_t S,
                        void* stream) {
  EGO_TRACE("ego_scatter_density");
  EGO_REQUIRE(sc, "scatter_density: null scene");
  if (sc->density.n_comp != 16) return ego_fail(EGO_E_UNSUPPORTED, "scatter_density: n_comp %d (supported: 16)", sc->density.n_comp);
  ScatterArgs a{};
  if (int e = scatter_common(sc->density, gdensity, coords, dfeat, N, S, &a, "scatter_density")) return e;
  if (N == 0) return EGO_OK;
  k_vm_scatter<16, true><<<scatter_blocks(a), 256, 0, (hipStream_t)stream>>>(a);
  return ego_launch_status("k_vm_scatter<16>");
}

int ego_scatter_app(const ego_scene* sc, const ego_vm_grad* gapp, const float* coords, const float* dv, int64_t N, int32_t S,
                    void* stream) {
  EGO_TRACE("ego_scatter_app");
  EGO_REQUIRE(sc, "scatter_app: null scene");
  if (sc->app.n_comp != APP_C) return ego_fail(EGO_E_UNSUPPORTED, "scatter_app: n_comp %d (supported: 48)", sc->app.n_comp);
  ScatterArgs a{};
  if (int e = scatter_common(sc->app, gapp, coords, dv, N, S, &a, "scatter_app")) return e;
  if (N == 0) return EGO_OK;
  k_vm_scatter<APP_C, false><<<scatter_blocks(a), 256, 0, (hipStream_t)stream>>>(a);
  return ego_launch_status("k_vm_scatter<48>");
}

}  // extern "C"
