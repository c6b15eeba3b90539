// The density feature of one sample, lane = sample: sum_i relu(sum_c P_ic * L_ic)      models/EgoNeRF.py:291-347, 232-289
// One body for ego_density_feature (csrc/ego_stages.hip) and the lattice field of the mesh extraction (csrc/ego_mesh.hip).
#pragma once
#include "ego_device.h"

// one bilinear tap = C contiguous floats (C/4 x 16-byte loads).  (k_march_generic, csrc/ego_generic_march.hip, holds the same sum with C
// at run time: called from there, this body changes that kernel's load schedule.)
template <int C>
__device__ __forceinline__ float density_lookup(const DevField& F, int g, float a_r, float a_th, float a_ph) {
#pragma clang fp contract(fast)  // the library is built with -ffp-contract=off; interpolation may use FMAs
  const VMTaps t = vm_setup(a_r, a_th, a_ph, F.res);
  float feat = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const PlaneTaps T = EGO_PLANE_TAPS_OF(F, C, g, i, t.ax);
    float dot = 0.f;
#pragma unroll
    for (int c4 = 0; c4 < C; c4 += 4) {
      const f32x4 pv = tap4(T.p00, c4) * T.w00 + tap4(T.p01, c4) * T.w01 + tap4(T.p10, c4) * T.w10 + tap4(T.p11, c4) * T.w11;
      const f32x4 lv = tap4(T.l0, c4) * T.wl0 + tap4(T.l1, c4) * T.wl1;
      const f32x4 m = pv * lv;
      dot += (m.x + m.y) + (m.z + m.w);
    }
    feat += fmaxf(dot, 0.f);
  }
  return feat;
}
