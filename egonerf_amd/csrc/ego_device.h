// Device helpers shared by every kernel of libegonerf_hip.so (gfx950 only, wave64).
// Arithmetic follows the reference's ATen op sequence rounding-by-rounding where that is cheap
// (explicit __f*_rn so the compiler does not contract into FMAs the CPU path does not use).
// The geometry of a vector-matrix lookup is defined here once: the axis maps and table sizes (vm_plane_x ... vm_line_elems, host and
// device), the tap set-up with and without derivatives (lin_taps), the per-plane tap description of the fp32 tables (PlaneTaps), the
// envmap's direction -> taps (envmap_taps) and row_sum16.  Host-side builders and checks of these structs: ego_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/egonerf_hip.h"

#define EGO_WAVE 64

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------
// POD copies of the scene that travel in kernel arguments (SGPR-resident, no pointer chasing).
// ---------------------------------------------------------------------------------------------
struct DevField {
  const float* plane[2][3];
  const float* line[2][3];
  int32_t res[3];  // N_r, N_theta, N_phi
  // compact addressing for the forward gathers: the 12 tables of a field lie within 4 GB of `base` (the lowest of them), so a tap
  // is `base + 32-bit byte offset`: one scalar base register pair + one VGPR per address (global_load saddr form) instead of a
  // per-lane 64-bit pointer select and 64-bit adds.  ego_field_is_compact() (ego_host.h) checks it on the host; the backward kernels keep
  // using the pointer arrays.
  const char* base;
  uint32_t poff[2][3];
  uint32_t loff[2][3];
};

struct DevCoords {
  float cx, cy, cz;
  float th_near, ph_near, th_inv, ph_inv;
  const float* r_lut;
  int32_t n_lut;  // N_r + 1
  int32_t n_r;
};

// ---------------------------------------------------------------------------------------------
// Row A  — sample schedule -> points      models/EgoNeRF.py:56-87
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float sched_z(const float* __restrict__ r_sched, const float* __restrict__ jitter,
                                         int64_t ray, int s, int S, float near_) {
  float r = r_sched[s];
  if (jitter) {
    const float step = (s < S - 1) ? __fsub_rn(r_sched[s + 1], r) : __fsub_rn(r, r_sched[S - 2]);
    r = __fadd_rn(r, __fmul_rn(step, jitter[ray * S + s]));
  }
  return __fadd_rn(near_, r);
}

// ---------------------------------------------------------------------------------------------
// Row B: Cartesian -> (r, theta, phi, is_yang)   models/coordinates.py:468-498
// ---------------------------------------------------------------------------------------------
struct YinYang {
  float r, th, ph;
  int yang;
};

#define EGO_PI_4 0.78539816339744830962f       // float32(pi/4): thresholds compare in float32
#define EGO_3PI_4 2.35619449019234492885f

__device__ __forceinline__ float nan_to_zero(float v) { return (v != v) ? 0.0f : v; }

__device__ __forceinline__ YinYang yinyang_from_xyz(float x, float y, float z, const DevCoords& c) {
  const float dx = __fsub_rn(x, c.cx), dy = __fsub_rn(y, c.cy), dz = __fsub_rn(z, c.cz);
  const float r = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
  const float th_n = nan_to_zero(acosf(__fdiv_rn(dz, r)));
  const float ph_n = atan2f(dy, dx);
  const bool yin = (EGO_PI_4 <= th_n) && (th_n <= EGO_3PI_4) && (-EGO_3PI_4 <= ph_n) && (ph_n <= EGO_3PI_4);
  YinYang o;
  o.r = r;
  if (yin) {
    o.th = th_n; o.ph = ph_n; o.yang = 0;
  } else {
    o.th = nan_to_zero(acosf(__fdiv_rn(dy, r)));
    o.ph = atan2f(dz, -dx);
    o.yang = 1;
  }
  return o;
}

// ---------------------------------------------------------------------------------------------
// Row C: normalisation   models/coordinates.py:442-466, :110-131, :156
// `lut` may point to LDS or global memory.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float normalize_r(float r, const float* lut, int n_lut, int n_r) {
  // searchsorted(side='right'): first index with lut[i] > r; NaN sorts last like torch.
  int lo = 0, hi = n_lut;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (!(lut[mid] > r)) lo = mid + 1; else hi = mid;
  }
  int k_out = lo < 1 ? 1 : (lo > n_lut - 1 ? n_lut - 1 : lo);
  const int k_in = k_out - 1;
  const float g0 = lut[k_in], g1 = lut[k_out];
  const float frac = __fdiv_rn(__fsub_rn(r, g0), __fsub_rn(g1, g0));
  const float v = __fdiv_rn(__fadd_rn((float)k_in, frac), (float)n_r);
  return __fsub_rn(__fmul_rn(v, 2.0f), 1.0f);
}

__device__ __forceinline__ float normalize_ang(float a, float near_, float inv) {
  return __fsub_rn(__fmul_rn(__fmul_rn(__fsub_rn(a, near_), inv), 2.0f), 1.0f);
}

// ---------------------------------------------------------------------------------------------
// Bilinear / linear tap set-up with align_corners=True, zero padding (F.grid_sample semantics,
// ATen GridSamplerKernel: ix = (x+1)*((W-1)/2); west weight = 1-fx).
// ---------------------------------------------------------------------------------------------
struct Lin1 {
  int i0, i1;    // clamped indices (always addressable)
  float w0, w1;  // weights with the out-of-range taps zeroed
};

// ... plus the derivative of the two weights with respect to the normalised coordinate: -/+ (n - 1) / 2 where the tap is in range (the
// ray gradients, csrc/ego_ray_grad.hip)
struct LinD : Lin1 {
  float d0, d1;
};

// The one body of the tap set-up; DERIV = false leaves d0 / d1 unset (and their instructions unwritten): lin_setup's callers
template <bool DERIV>
__device__ __forceinline__ LinD lin_taps(float xhat, int n) {
  LinD t;
  const float x1 = __fadd_rn(xhat, 1.0f), sc = 0.5f * (float)(n - 1);
  const float ix = __fmul_rn(x1, sc);
  const float fl = floorf(ix);
  const float f = __fsub_rn(ix, fl);
  // ix may be NaN/huge for degenerate points: keep the int conversion defined and the taps masked (fmaxf(NaN, -2) = -2, so
  // a NaN lands on i0 = -2, i1 = -1: both out of range).  One unsigned compare per tap: 0 <= i < n.
  const float flc = fminf(fmaxf(fl, -2.0f), (float)n);
  const int i0 = (int)flc, i1 = i0 + 1;
  const bool in0 = (unsigned)i0 < (unsigned)n;
  t.w0 = in0 ? __fsub_rn(1.0f, f) : 0.0f;
  const bool in1 = (unsigned)i1 < (unsigned)n;
  t.w1 = in1 ? f : 0.0f;
  if (DERIV) {
    t.d0 = in0 ? -sc : 0.0f;
    t.d1 = in1 ? sc : 0.0f;
  }
  t.i0 = min(max(i0, 0), n - 1);
  t.i1 = min(max(i1, 0), n - 1);
  return t;
}

__device__ __forceinline__ Lin1 lin_setup(float xhat, int n) { return lin_taps<false>(xhat, n); }
__device__ __forceinline__ LinD lind_setup(float xhat, int n) { return lin_taps<true>(xhat, n); }

// The three (plane, line) lookups of one grid address these axes (matMode / vecMode, EgoNeRF.py:30-33):
//   i=0: plane x=r (W=N_r), y=theta (H=N_theta); line = phi
//   i=1: plane x=r,         y=phi   (H=N_phi);   line = theta
//   i=2: plane x=theta (W=N_theta), y=phi;       line = r
struct VMTaps {
  Lin1 ax[3];  // per axis: 0 r, 1 theta, 2 phi
};

__device__ __forceinline__ VMTaps vm_setup(float a_r, float a_th, float a_ph, const int32_t res[3]) {
  VMTaps t;
  t.ax[0] = lin_setup(a_r, res[0]);
  t.ax[1] = lin_setup(a_th, res[1]);
  t.ax[2] = lin_setup(a_ph, res[2]);
  return t;
}

// The axis maps and table sizes, for host and device code alike: the ONE place that says which axes a table spans.  The maps are
// expressions first (macros) and functions over them: k_scatter_generic (csrc/ego_generic_train.hip), where the plane index is a
// run-time value, needs the expression in its own text - a call, even a force-inlined one, is folded later and its code comes out different.
#define VM_PLANE_X(i) ((i) == 2 ? 1 : 0)
#define VM_PLANE_Y(i) ((i) == 0 ? 1 : 2)
#define VM_LINE_AX(i) (2 - (i))
__host__ __device__ __forceinline__ constexpr int vm_plane_x(int i) { return VM_PLANE_X(i); }
__host__ __device__ __forceinline__ constexpr int vm_plane_y(int i) { return VM_PLANE_Y(i); }
__host__ __device__ __forceinline__ constexpr int vm_line_ax(int i) { return VM_LINE_AX(i); }
// elements of plane i, [res[y axis]][res[x axis]][n_comp], and of line i, [res[line axis]][n_comp]
__host__ __device__ __forceinline__ constexpr int64_t vm_plane_elems(const int32_t res[3], int n_comp, int i) {
  return (int64_t)res[vm_plane_y(i)] * res[vm_plane_x(i)] * n_comp;
}
__host__ __device__ __forceinline__ constexpr int64_t vm_line_elems(const int32_t res[3], int n_comp, int i) {
  return (int64_t)res[vm_line_ax(i)] * n_comp;
}

// Plane i of one sample's lookup in channel-last fp32 tables of C channels, described once for the fp32 compatibility, stage and
// ray-gradient kernels, whatever their work split: the plane and line table of the sample's grid, the ELEMENT offsets of the four bilinear
// taps (o<y><x>) and the two line taps (what a scatter applies to the gradient tables too), the same six taps as pointers (thread =
// sample consumers step through them 16 bytes at a time), the four bilinear weights and the two line weights.  Channel c of a tap is
// P[o + c] = p[c].  Nothing a consumer does not read costs an instruction.  The tuned shade / march / scatter / sorted-walk kernels
// keep their own forms on purpose: base + 32-bit offset, run merging.
struct PlaneTaps {
  const float* P;
  const float* L;
  int64_t o00, o01, o10, o11, ol0, ol1;
  const float *p00, *p01, *p10, *p11, *l0, *l1;
  float w00, w01, w10, w11, wl0, wl1;
};

// channels c4 .. c4 + 3 of a tap as one 16-byte load (thread = sample consumers; C % 4 == 0, tables 16-byte aligned)
__device__ __forceinline__ f32x4 tap4(const float* tap, int c4) { return *(const f32x4*)(tap + c4); }

// X, Y, Ln = the taps of the plane's x axis, y axis and of the line's axis (Lin1, or LinD sliced); W = the plane's row length
__device__ __forceinline__ PlaneTaps plane_taps(const Lin1 X, const Lin1 Y, const Lin1 Ln, int W, const float* P, const float* L, int C) {
  PlaneTaps T;
  T.P = P;
  T.L = L;
  T.o00 = ((int64_t)Y.i0 * W + X.i0) * C; T.p00 = T.P + T.o00;
  T.o01 = ((int64_t)Y.i0 * W + X.i1) * C; T.p01 = T.P + T.o01;
  T.o10 = ((int64_t)Y.i1 * W + X.i0) * C; T.p10 = T.P + T.o10;
  T.o11 = ((int64_t)Y.i1 * W + X.i1) * C; T.p11 = T.P + T.o11;
  T.ol0 = (int64_t)Ln.i0 * C; T.l0 = T.L + T.ol0;
  T.ol1 = (int64_t)Ln.i1 * C; T.l1 = T.L + T.ol1;
  T.w00 = __fmul_rn(Y.w0, X.w0); T.w01 = __fmul_rn(Y.w0, X.w1);
  T.w10 = __fmul_rn(Y.w1, X.w0); T.w11 = __fmul_rn(Y.w1, X.w1);
  T.wl0 = Ln.w0; T.wl1 = Ln.w1;
  return T;
}
// ... of plane i of field F for a sample of grid g with the three axes' taps ax[3].  A macro: the field's loads have to stand in the
// kernel's own text, after the copies of the axes - through a function that takes the field by reference, k_shade_generic and
// k_app_bwd_prep select and hoist the table pointers differently and their code changes.
#define EGO_PLANE_TAPS_OF(F, C, g, i, ax) \
  plane_taps((ax)[vm_plane_x(i)], (ax)[vm_plane_y(i)], (ax)[vm_line_ax(i)], (F).res[vm_plane_x(i)], \
             (g) ? (F).plane[1][i] : (F).plane[0][i], (g) ? (F).line[1][i] : (F).line[0][i], C)

// ---------------------------------------------------------------------------------------------
// Row M — occupancy lookup: trilinear F.grid_sample (align_corners, zeros) on a {0,1} volume [N_phi][N_theta][N_r]
// models/EgoNeRF.py:11-24
// ---------------------------------------------------------------------------------------------
struct DevOcc {
  const uint8_t* vol;  // [2][res2][res1][res0] or null
  int32_t res[3];
  const uint8_t* cell; // optional [2][res2-1][res1-1][res0-1]: OR of the 8 corner voxels of every cell (ego_scene.occ_cell)
};

// (occ_occupied_taps below restates this evaluation and occ_occupied's decision for a caller that already holds the taps: a change here
// is a change there; tests/test_hip_dense_density.py holds the two against each other on masked scenes)
__device__ __forceinline__ float occ_sample(const DevOcc& O, int g, float a_r, float a_th, float a_ph) {
  const Lin1 X = lin_setup(a_r, O.res[0]), Y = lin_setup(a_th, O.res[1]), Z = lin_setup(a_ph, O.res[2]);
  const uint8_t* V = O.vol + (int64_t)g * O.res[0] * O.res[1] * O.res[2];
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int ix = (k & 1) ? X.i1 : X.i0, iy = (k & 2) ? Y.i1 : Y.i0, iz = (k & 4) ? Z.i1 : Z.i0;
    const float w = ((k & 1) ? X.w1 : X.w0) * ((k & 2) ? Y.w1 : Y.w0) * ((k & 4) ? Z.w1 : Z.w0);
    v += w * (float)V[((int64_t)iz * O.res[1] + iy) * O.res[0] + ix];
  }
  return v;
}

// "mask value > 0" (tensorBase.py:464-478) for the march: a sample strictly inside a cell (all six axis weights > 0, all taps in
// range) has a positive trilinear value iff any of the cell's eight corner voxels is set - one byte of the per-cell OR volume instead
// of eight dependent byte loads and the interpolation; samples on a lattice plane / outside the volume take the exact evaluation
// (restated in occ_occupied_taps below: keep the two alike)
__device__ __forceinline__ bool occ_occupied(const DevOcc& O, int g, float a_r, float a_th, float a_ph) {
  if (O.cell) {
    const Lin1 X = lin_setup(a_r, O.res[0]), Y = lin_setup(a_th, O.res[1]), Z = lin_setup(a_ph, O.res[2]);
    const bool interior = fminf(fminf(fminf(X.w0, X.w1), fminf(Y.w0, Y.w1)), fminf(Z.w0, Z.w1)) > 0.f;
    if (interior) {
      const int64_t c0 = O.res[0] - 1, c1 = O.res[1] - 1, c2 = O.res[2] - 1;
      return O.cell[(((int64_t)g * c2 + Z.i0) * c1 + Y.i0) * c0 + X.i0] != 0;
    }
  }
  return occ_sample(O, g, a_r, a_th, a_ph) > 0.f;
}

// occ_occupied from the three axes' taps at O.res, for a caller that has them already: the dense march needs the field's own taps in
// its phase B, and a mask of the field's resolution (the usual one) then costs no second set-up.  Same decisions, same evaluation
// order as occ_occupied / occ_sample above, which keep their own text: routed through here, the kernels built on them come out with
// different code.  The volume here has the resolution of a field whose dense grid the march addresses with 32-bit byte offsets (16 B per
// voxel, both grids under 4 GB: ego_march_density checks it), so a voxel or cell index of either grid is below 2^28 and is computed in 32
// bits: base + one VGPR per address instead of a 64-bit multiply chain per lane.
__device__ __forceinline__ bool occ_occupied_taps(const DevOcc& O, int g, const Lin1 X, const Lin1 Y, const Lin1 Z) {
  if (O.cell) {
    const bool interior = fminf(fminf(fminf(X.w0, X.w1), fminf(Y.w0, Y.w1)), fminf(Z.w0, Z.w1)) > 0.f;
    if (interior) {
      const uint32_t c0 = O.res[0] - 1, c1 = O.res[1] - 1, c2 = O.res[2] - 1;
      return O.cell[(((uint32_t)g * c2 + (uint32_t)Z.i0) * c1 + (uint32_t)Y.i0) * c0 + (uint32_t)X.i0] != 0;
    }
  }
  const uint32_t r0 = O.res[0], r1 = O.res[1], gv = (uint32_t)g * r0 * r1 * (uint32_t)O.res[2];
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int ix = (k & 1) ? X.i1 : X.i0, iy = (k & 2) ? Y.i1 : Y.i0, iz = (k & 4) ? Z.i1 : Z.i0;
    const float w = ((k & 1) ? X.w1 : X.w0) * ((k & 2) ? Y.w1 : Y.w0) * ((k & 4) ? Z.w1 : Z.w0);
    v += w * (float)O.vol[gv + ((uint32_t)iz * r1 + (uint32_t)iy) * r0 + (uint32_t)ix];
  }
  return v > 0.f;
}

// ---------------------------------------------------------------------------------------------
// Row E scalars
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float softplus_shift(float f, float shift) {
  const float x = __fadd_rn(f, shift);
  return x > 20.0f ? x : log1pf(expf(x));  // torch softplus, threshold 20
}

// relu as an integer max: one v_max_i32 (fmaxf costs a canonicalising v_max_f32 first); -0.0 and negatives -> +0.0
__device__ __forceinline__ float relu_f(float x) {
  return __builtin_bit_cast(float, max(__builtin_bit_cast(int, x), 0));
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// raw2alpha (tensorBase.py:22-27: alpha = 1 - exp(-sigma * dist)) evaluated as -expm1(-x): the correctly rounded value of the
// reference's expression.  The literal float32 form loses ~6e-8 ABSOLUTE in the subtraction (6e-6 relative at alpha = 0.01), in the
// reference as much as here but with a different exp and therefore a different error; the inverse CDF of the resampling pass
// amplifies exactly those weight errors (steep tiny grids: 1e-4 in RGB from 6e-8 in the coarse weights).  With the accurate form
// this side contributes nothing, so the distance to the reference is the reference's own rounding error instead of the sum of two.
__device__ __forceinline__ float alpha_from(float x) { return -expm1f(-x); }

// sin and cos of one argument: Cody-Waite reduction by pi/2 (two FMAs) + Cephes minimax polynomials on
// [-pi/4, pi/4].  ~1 ulp for |x| < 1e4, branch-free (the libm versions drag a Payne-Hanek slow path
// into every call site, which matters when 68 of them are inlined between MFMAs).
__device__ __forceinline__ void sincos_f32(float x, float& s_out, float& c_out) {
  const float k = rintf(x * 0.63661977236758134308f);
  float r = fmaf(k, -1.57079637050628662109375f, x);      // float32(pi/2)
  r = fmaf(k, 4.37113900018624283e-8f, r);                // pi/2 - float32(pi/2) = -4.371139e-8
  const float r2 = r * r;
  const float ps = fmaf(fmaf(fmaf(-1.9515295891e-4f, r2, 8.3321608736e-3f), r2, -1.6666654611e-1f), r2 * r, r);
  const float pc = fmaf(fmaf(fmaf(2.443315711809948e-5f, r2, -1.388731625493765e-3f), r2, 4.166664568298827e-2f),
                        r2 * r2, fmaf(-0.5f, r2, 1.0f));
  const int q = (int)k;
  const float s = (q & 1) ? pc : ps;
  const float c = (q & 1) ? ps : pc;
  s_out = (q & 2) ? -s : s;
  c_out = ((q + 1) & 2) ? -c : c;
}

// sin/cos of x and 2x (the two positional-encoding frequencies): one reduction + double-angle identities.
// sin 2x = 2 s c, cos 2x = 1 - 2 s^2: adds <= 2 ulp to the ~1 ulp of sincos_f32.
__device__ __forceinline__ void sincos_x_2x(float x, float& s1, float& c1, float& s2, float& c2) {
  sincos_f32(x, s1, c1);
  const float t = s1 + s1;
  s2 = t * c1;
  c2 = fmaf(-t, s1, 1.0f);
}

// Same outputs through the hardware transcendentals (v_sin_f32 / v_cos_f32 take revolutions): 6 VALU issues instead
// of 27.  Measured on gfx950 (tools/sincos_probe.hip): max |err| 1.4e-7 for |x| < 2 (the feature range), 8e-7 at |x| = 12
// (the x / 2pi product rounds at |x| * 6e-8); the double angle doubles it.  Used by the f16x3 shade kernel only.
__device__ __forceinline__ void sincos_x_2x_hw(float x, float& s1, float& c1, float& s2, float& c2) {
  const float t = x * 0.15915494309189533577f;
  s1 = __builtin_amdgcn_sinf(t);
  c1 = __builtin_amdgcn_cosf(t);
  const float d = s1 + s1;
  s2 = d * c1;
  c2 = fmaf(-d, s1, 1.0f);
}

// wave64 inclusive multiplicative scan on the DPP path (no LDS round trips; __shfl_up compiles to ds_bpermute_b32 + s_waitcnt):
// row_shr 1, 2, 4, 8 inside the 16-lane rows, then row_bcast:15 into rows 1 / 3 and row_bcast:31 into rows 2 / 3.  Lanes without a
// source keep `old` = 1.0, the identity, so no per-step select is needed.
__device__ __forceinline__ float wave_scan_mul(float v, int /*lane*/) {
  const int one = __float_as_int(1.0f);
#define EGO_SCAN_STEP(ctrl, rmask) v *= __int_as_float(__builtin_amdgcn_update_dpp(one, __float_as_int(v), ctrl, rmask, 0xf, false))
  EGO_SCAN_STEP(0x111, 0xf);  // row_shr:1
  EGO_SCAN_STEP(0x112, 0xf);  // row_shr:2
  EGO_SCAN_STEP(0x114, 0xf);  // row_shr:4
  EGO_SCAN_STEP(0x118, 0xf);  // row_shr:8
  EGO_SCAN_STEP(0x142, 0xa);  // row_bcast:15 -> rows 1, 3
  EGO_SCAN_STEP(0x143, 0xc);  // row_bcast:31 -> rows 2, 3
#undef EGO_SCAN_STEP
  return v;
}

// The transmittance step of one 64-sample pass (lane = sample; tensorBase.py:22-27), the one body of k_raw2alpha (csrc/ego_stages.hip)
// and both density marches: alpha from x = sigma * dist, the pass's exclusive product of (1 - alpha + 1e-10) and its total.  A lane
// without a sample (`ok` false) has alpha 0 and the factor 1.  The transmittance in front of sample s is (carry in front of the pass) * exc.
struct PassT {
  float a, exc, tot;
};
__device__ __forceinline__ PassT transmittance_step(bool ok, float x, int lane) {
  const float a = ok ? alpha_from(x) : 0.f;
  const float t = ok ? __fadd_rn(__fsub_rn(1.f, a), 1e-10f) : 1.f;
  const float inc = wave_scan_mul(t, lane);
  float exc = __shfl_up(inc, 1, 64);
  if (lane == 0) exc = 1.f;
  return {a, exc, __shfl(inc, 63, 64)};
}

// Row J - environment map (models/envmap.py:6-14, 26-34).  Direction -> taps in the emission [3][2h][h]: F.normalize, u = (n_z + 1) / 2
// on the h-wide axis, v = (atan2(n_y, n_x) + pi) / 2 pi on the 2h axis.  One body for the lookup, its backward into the emission
// (k_envmap_bwd, csrc/ego_stages.hip) and its direction gradient (csrc/ego_ray_grad.hip), which also reads n, |d| and the derivatives.
struct EnvTaps {
  float nx, ny, nz, nrm;
  LinD X, Y;
};

__device__ __forceinline__ EnvTaps envmap_taps(float dx, float dy, float dz, int h) {
  const float nrm = fmaxf(__fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz))), 1e-12f);
  const float nx = __fdiv_rn(dx, nrm), ny = __fdiv_rn(dy, nrm), nz = __fdiv_rn(dz, nrm);
  const float u = __fmul_rn(__fadd_rn(nz, 1.f), 0.5f);
  const float v = __fdiv_rn(__fadd_rn(atan2f(ny, nx), 3.14159265358979323846f), 6.28318530717958647692f);
  return EnvTaps{nx, ny, nz, nrm,
                 lind_setup(__fsub_rn(__fmul_rn(u, 2.f), 1.f), h),        // u indexes the h-wide axis
                 lind_setup(__fsub_rn(__fmul_rn(v, 2.f), 1.f), 2 * h)};   // v indexes the 2h axis
}

// bilinear lookup of the sigmoid-ed emission in direction (dx, dy, dz)
__device__ __forceinline__ void envmap_lookup(const float* __restrict__ em, int h, float dx, float dy, float dz,
                                              float out[3]) {
  const EnvTaps t = envmap_taps(dx, dy, dz, h);
  const Lin1 &X = t.X, &Y = t.Y;
  const float w00 = __fmul_rn(Y.w0, X.w0), w01 = __fmul_rn(Y.w0, X.w1), w10 = __fmul_rn(Y.w1, X.w0),
              w11 = __fmul_rn(Y.w1, X.w1);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float* E = em + (int64_t)ch * 2 * h * h;
    const float s = E[(int64_t)Y.i0 * h + X.i0] * w00 + E[(int64_t)Y.i0 * h + X.i1] * w01 +
                    E[(int64_t)Y.i1 * h + X.i0] * w10 + E[(int64_t)Y.i1 * h + X.i1] * w11;
    out[ch] = sigmoidf(s);
  }
}

// Equirectangular camera ray of pixel (row, col) of an H x W panorama: get_ray_directions_360 (dataLoader/ray_utils.py:24-40),
// the datasets' normalisation and get_rays (:85-113).  m = camera-to-world pose, 3x4 row-major (kernel argument or device memory);
// o[6] = origin, direction.  ONE body for ego_erp_rays (csrc/ego_stages.hip) and the ray-bank gather (csrc/ego_batch.hip): a gathered ray
// has the bits of the corresponding row of ego_erp_rays.
__device__ __forceinline__ void erp_ray(int H, int W, int row, int col, const float* m, int normalize, float* o) {
  const float i = (float)col + 0.5f, j = (float)row + 0.5f;
  const float phi = __fmul_rn(__fsub_rn(1.f, __fdiv_rn(__fmul_rn(2.f, i), (float)W)), 3.14159265358979323846f);
  const float theta = __fdiv_rn(__fmul_rn(__fsub_rn(1.f, __fdiv_rn(__fmul_rn(2.f, j), (float)H)), 3.14159265358979323846f), 2.f);
  const float ct = cosf(theta);
  float d0 = -ct * sinf(phi), d1 = sinf(theta), d2 = -ct * cosf(phi);
  if (normalize) {  // directions / torch.norm(directions, dim=-1): sqrt of the sum of squares, then three divisions
    const float n = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)));
    d0 = __fdiv_rn(d0, n); d1 = __fdiv_rn(d1, n); d2 = __fdiv_rn(d2, n);
  }
  o[0] = m[3]; o[1] = m[7]; o[2] = m[11];
#pragma unroll
  for (int r = 0; r < 3; ++r) o[3 + r] = (d0 * m[4 * r] + d1 * m[4 * r + 1]) + d2 * m[4 * r + 2];
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// sum over the 16 lanes of a row on the DPP path (every lane gets the total; a fixed order)
__device__ __forceinline__ float row_sum16(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xb1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4e, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false));   // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, false));   // row_mirror
  return v;
}
