// Device-side internals shared by the any-shape kernels (ego_generic.hip, ego_generic_train.hip, ego_generic_march.hip): the weight
// blob's layout, the pipelined-load loop, the wave-level slab synchronisation, the D layout and grid masks of the MFMA products
// and the encodings' sincos.
#pragma once
#include "ego_device.h"

namespace {

// packed layout (floats): W1T [in_c][HID] | b1 [HID] | W2T [HID][HID] | b2 [HID] | W3 [3][HID] | b3 [4] | basisT [2][3 C][32] | W1 | W2 | basis [2][32][3 C]
struct GenLayout {
  int64_t w1t, b1, w2t, b2, w3, b3, basis, w1n, w2n, basisn, total;
};
__host__ __device__ inline GenLayout gen_layout(int in_c, int hid, int n_comp) {
  GenLayout L;
  int64_t o = 0;
  L.w1t = o; o += (int64_t)in_c * hid;
  L.b1 = o; o += hid;
  L.w2t = o; o += (int64_t)hid * hid;
  L.b2 = o; o += hid;
  L.w3 = o; o += 3 * hid;
  L.b3 = o; o += 4;
  L.basis = o; o += 2 * 3 * (int64_t)n_comp * 32;
  // the same matrices the other way round, for the backward's products on the matrix pipe (B operands with the OUTPUT index contiguous):
  // W1 [HID][in_c], W2 [HID][HID] (the reference's own layouts), basis [2][32][3 C] (rows >= app_dim zero)
  L.w1n = o; o += (int64_t)hid * in_c;
  L.w2n = o; o += (int64_t)hid * hid;
  L.basisn = o; o += 2 * 32 * 3 * (int64_t)n_comp;
  L.total = o;
  return L;
}

enum { G_SHADE = 0, G_APP = 1, G_MLP = 2 };

// n iterations of body(it, b) with the NB values b = loadb(it) of iteration it + PF already in flight: one wave per SIMD has nobody else
// to hide a global load behind (a loop that loads, waits and multiplies spent 3 000 clocks per 512 clocks of MFMA)
template <int PF, int NB, class LB, class BD>
__device__ __forceinline__ void gen_pipelined(int n, LB loadb, BD body) {
  if (n <= 0) return;
  float bq[PF][NB];
#pragma unroll
  for (int p = 0; p < PF; ++p) loadb(p < n ? p : n - 1, bq[p]);
  for (int i0 = 0; i0 < n; i0 += PF) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int it = i0 + p;
      if (it < n) {
        float b[NB];
#pragma unroll
        for (int e = 0; e < NB; ++e) b[e] = bq[p][e];
        const int nx = it + PF;
        loadb(nx < n ? nx : n - 1, bq[p]);
        __builtin_amdgcn_sched_barrier(0);   // (the machine scheduler sinks the loads back to their uses otherwise: `s_waitcnt vmcnt(0)` at the loop's top)
        body(it, b);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
}

// dv element (sample ms, column c = plane * C + channel): row-major [M][ldv], or (ldv == 0; C == 48) the tuned scatters' blocked layout
// [tile of 32 samples][plane * 3 + 16-channel line][sample][16] (include/egonerf_hip.h, ego_shade_backward)
__device__ __forceinline__ int64_t gen_dv_index(int64_t ms, int c, int ldv) {
  return ldv ? ms * ldv + c : (ms >> 5) * (32 * 144) + (int64_t)(c >> 4) * 512 + (ms & 31) * 16 + (c & 15);
}

__device__ __forceinline__ void wave_sync_g() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
typedef __attribute__((address_space(4))) float gen_cfloat;

// The D layout of v_mfma_f32_32x32x2_f32 as the head kernels use it (A = [sample][k], B = [k][column]): register r of lane l of tile mt
// holds column l % 32 of sample 32 mt + 8 (r / 4) + 4 (l / 32) + r % 4 of the wave's 64-sample unit (kk = l / 32); counted from `base`
template <class T>
__device__ __forceinline__ T gen_d_sample(T base, int mt, int r, int kk) { return base + 32 * mt + 8 * (r >> 2) + 4 * kk + (r & 3); }

// which grid the wave's samples belong to (g != 0: yang), as the per-grid products need it: a sample's row of A is zeroed for the grid it
// does not belong to (yang0 / yang1: the grid of samples l31 and 32 + l31, the two A rows this lane feeds), a grid nobody is in is skipped
struct GenGridMask {
  bool any_yin, any_yang, yang0, yang1;
};
__device__ __forceinline__ GenGridMask gen_grid_mask(int g, int l31) {
  const unsigned long long gmask = __ballot(g != 0);
  return {~gmask != 0ull, gmask != 0ull, (bool)((gmask >> l31) & 1ull), (bool)((gmask >> (32 + l31)) & 1ull)};
}

// torch.sin / torch.cos of the positional encodings (tensorBase.py:10-19), both from ONE argument reduction, branch-free: the reduction
// by pi/2 runs in float64 (x - k pi/2 with a two-term pi/2: exact to the last bit of the float32 remainder while |x| < ~1e15 - libm's
// float32 route needs a Payne-Hanek slow path for that, and sinf + cosf inlined 2 x 32 times per frequency were two thirds of this
// kernel's instructions), the Cephes minimax polynomials of sincos_f32 (ego_device.h) on [-pi/4, pi/4] follow in float32: ~1 ulp.
__device__ __forceinline__ void gen_sincos(float x, float& s_out, float& c_out) {
  const double xd = (double)x;
  const double kd = rint(xd * 0.63661977236758134308);
  double rd = fma(kd, -1.57079632679489655800e+00, xd);      // double(pi/2)
  rd = fma(kd, -6.12323399573676603587e-17, rd);             // pi/2 - double(pi/2)
  const float r = (float)rd, r2 = r * r;
  const float ps = fmaf(fmaf(fmaf(-1.9515295891e-4f, r2, 8.3321608736e-3f), r2, -1.6666654611e-1f), r2 * r, r);
  const float pc = fmaf(fmaf(fmaf(2.443315711809948e-5f, r2, -1.388731625493765e-3f), r2, 4.166664568298827e-2f), r2 * r2, fmaf(-0.5f, r2, 1.0f));
  const int q = (int)(kd - 4.0 * floor(kd * 0.25));          // k mod 4 in 0 .. 3, whatever the size of k
  const float s = (q & 1) ? pc : ps, c = (q & 1) ? ps : pc;
  s_out = (q & 2) ? -s : s;
  c_out = ((q + 1) & 2) ? -c : c;
}

}  // namespace
