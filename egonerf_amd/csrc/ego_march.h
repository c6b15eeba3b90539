// Internal: what the two density marches share - k_march_density (csrc/ego_march.hip, 16 density components) and k_march_generic
// (csrc/ego_generic_march.hip, any other count): the one kernel-argument block, and the pieces of a 64-sample pass that are the same
// text in both (lane = sample): phase A (distances, normalised coordinates) and the stores behind a ray's last pass.  The
// transmittance step between them is transmittance_step (ego_device.h), which k_raw2alpha uses too.  What k_march_generic does NOT
// share stays spelled out there, each piece with what sharing it measured: the schedule distance, the density sum, the weight / tile
// flag / output stores.
#pragma once
#include "ego_device.h"

// Everything a march launch reads, by value in the kernel-argument segment (wave-uniform: SGPRs).  Filled by ego_march_density
// (csrc/ego_march.hip) alone.  A member cannot promise __restrict__ (the qualifier tells the compiler nothing there); the pieces that
// gain from it take the pointer as a __restrict__ parameter of their own (sched_z, density_dense).
// The ORDER of the members is measured, not taste: it decides which members one scalar load fetches together and with that the
// kernels' SGPR allocation.  In this order (the kernels' parameter order before there was a block) every instance is as fast as it
// was; with the pointers, the sizes and the scalars grouped, the dense one-wave instance took 62.5 us for 61.5 at 16384 x 128.
struct MarchArgs {
  DevCoords c;
  DevField F;
  const char* dense;           // the field's baked node grid (csrc/ego_dense.hip) or null; k_march_density's dense form only
  uint32_t dense_grid_bytes;   // bytes of one grid of it: the yang grid follows the yin grid
  const float* rays;
  int64_t N;
  int32_t S, C;                // samples per ray; density components (k_march_generic: k_march_density is compiled for 16)
  const float* z_in; const float* r_sched; const float* jitter;   // explicit distances, or the schedule and its optional jitter
  float near_;
  int32_t softplus;
  float shift, dscale;
  float* z_out; float* alpha;
  int32_t alpha_stride;
  float* weight; float* bg; float* coords_out; float* sigma_out;
  DevOcc occ;                  // k_march_generic always takes the exact trilinear test (occ_sample) and never reads `cell`
  float term_eps, shade_above;
  uint8_t* tile_active;
};

struct MarchRay {
  float ox, oy, oz, dx, dy, dz;
};
__device__ __forceinline__ MarchRay march_ray(const float* rays, int64_t ray) {
  const float* R = rays + ray * 6;
  return {R[0], R[1], R[2], R[3], R[4], R[5]};
}

// ---- phase A: lane = sample ------------------------------------------------------------------------------------------------------
struct MarchSample {
  int s;       // the lane's sample, clamped to the ray's last one
  bool ok;     // ... which is its own (false: an idle lane of the tail pass, which computes the last sample again and stores nothing)
  float z, dist;
  float a_r, a_th, a_ph;   // march_coords
  int yang;
};

// z[s] and the distance to its right neighbour (left neighbour for the last sample: dists repeat the last interval), from explicit
// distances or, without them, from the caller's schedule `zz(k)`
template <class SchedZ>
__device__ __forceinline__ MarchSample march_distances(const float* z_in, int64_t ray, int s0, int lane, int S, SchedZ zz) {
  MarchSample m;
  m.s = min(s0 + lane, S - 1);
  m.ok = (s0 + lane) < S;
  const int sn = (m.s < S - 1) ? m.s + 1 : m.s - 1;
  float zn;
  if (z_in) {
    m.z = z_in[ray * S + m.s];
    zn = z_in[ray * S + sn];
  } else {
    m.z = zz(m.s);
    zn = zz(sn);
  }
  m.dist = (m.s < S - 1) ? __fsub_rn(zn, m.z) : __fsub_rn(m.z, zn);
  return m;
}

// the sample point, its yin-yang coordinates and their normalisation; the radius through the caller's `norm_r(r)`
template <class NormR>
__device__ __forceinline__ void march_coords(MarchSample& m, const DevCoords& c, const MarchRay& R, NormR norm_r) {
  const float px = __fadd_rn(R.ox, __fmul_rn(R.dx, m.z)), py = __fadd_rn(R.oy, __fmul_rn(R.dy, m.z)), pz = __fadd_rn(R.oz, __fmul_rn(R.dz, m.z));
  const YinYang y = yinyang_from_xyz(px, py, pz, c);
  m.a_r = norm_r(y.r);
  m.a_th = normalize_ang(y.th, c.th_near, c.th_inv);
  m.a_ph = normalize_ang(y.ph, c.ph_near, c.ph_inv);
  m.yang = y.yang;
}

// ---- behind a ray's last pass: with an environment map the reference appends a column of ones to alpha (EgoNeRF.py:587); the
// background weight is the transmittance behind the last sample
__device__ __forceinline__ void march_store_tail(const MarchArgs& A, int64_t ray, int lane, float carry, bool ones, bool bg) {
  if (ones && A.alpha && lane < A.alpha_stride - A.S) A.alpha[ray * A.alpha_stride + A.S + lane] = 1.f;
  if (bg && A.bg && lane == 0) A.bg[ray] = carry;
}
