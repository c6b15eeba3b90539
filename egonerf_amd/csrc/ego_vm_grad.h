// The positional derivative of a vector-matrix lookup, shared by the ray gradients (csrc/ego_ray_grad.hip), the ray
// geometry (csrc/ego_geometry.hip) and the point gradients of the mesh extraction (csrc/ego_mesh.hip):
// d (sum_c P_c L_c) / d (r^, theta^, phi^) per plane, the chart's Jacobian back to xyz, and the unit vector of the result.
// Work split of every caller: a 16-lane row owns a sample, lane = channel 16 at a time.
#pragma once
#include "ego_device.h"

namespace {

// q += g_v[c] d (plane x line)/d (r^, theta^, phi^) over the channels of this lane, plane i of one field; returns this lane's part of
// sum_c P L.  Density: g_v = 1 (the caller applies dfeat and the relu mask).  Appearance: g_v[c] = sum_k basis_g[k][i C + c] dfe[k] is
// re-derived (the tuned path writes no dv) from the channel's basis column in LDS (basis_g [3 C][BT_LD], dfe's own column order) and the
// sample's 32 feature-slot gradients in registers
constexpr int BT_LD = 36;   // 32 slots + 4: a row's 16 lanes read 16-byte pieces 144 B apart, two lanes per bank group instead of sixteen

template <bool DENS>
__device__ __forceinline__ float plane_terms(const DevField& F, int C, int g, int i, const LinD (&ax)[3], int c16, const float* basis_g,
                                             const f32x4 (&dk)[8], float (&q)[3]) {
  const LinD X = ax[vm_plane_x(i)], Y = ax[vm_plane_y(i)], Ln = ax[vm_line_ax(i)];
  const PlaneTaps T = EGO_PLANE_TAPS_OF(F, C, g, i, ax);
  float dot = 0.f;
  for (int c0 = 0; c0 < C; c0 += 16) {
    const int ch = c0 + c16;
    if (ch >= C) continue;
    const float p00 = T.P[T.o00 + ch], p01 = T.P[T.o01 + ch], p10 = T.P[T.o10 + ch], p11 = T.P[T.o11 + ch], l0 = T.L[T.ol0 + ch], l1 = T.L[T.ol1 + ch];
    float gv = 1.f;
    if (!DENS) {
      gv = 0.f;
      const f32x4* b = (const f32x4*)(basis_g + (i * C + ch) * BT_LD);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x4 bj = b[j];
        gv = fmaf(bj.x, dk[j].x, gv); gv = fmaf(bj.y, dk[j].y, gv); gv = fmaf(bj.z, dk[j].z, gv); gv = fmaf(bj.w, dk[j].w, gv);
      }
    }
    const float r0 = fmaf(p01, X.w1, p00 * X.w0), r1 = fmaf(p11, X.w1, p10 * X.w0);   // the two rows at x, and their derivative in x
    const float s0 = fmaf(p01, X.d1, p00 * X.d0), s1 = fmaf(p11, X.d1, p10 * X.d0);
    const float pv = fmaf(r1, Y.w1, r0 * Y.w0), dpx = fmaf(s1, Y.w1, s0 * Y.w0), dpy = fmaf(r1, Y.d1, r0 * Y.d0);
    const float lv = fmaf(l1, Ln.w1, l0 * Ln.w0), dl = fmaf(l1, Ln.d1, l0 * Ln.d0);
    dot = fmaf(pv, lv, dot);
    const float gl = gv * lv;
    q[vm_plane_x(i)] = fmaf(gl, dpx, q[vm_plane_x(i)]);
    q[vm_plane_y(i)] = fmaf(gl, dpy, q[vm_plane_y(i)]);
    q[vm_line_ax(i)] = fmaf(gv * pv, dl, q[vm_line_ax(i)]);
  }
  return dot;
}

// d (r^, theta^, phi^)/d xyz transposed onto q, for the chart the forward chose; 0 at r = 0, for q = 0 and for anything not finite
__device__ __forceinline__ void chart_jt(const DevCoords& c, const float* lut, int yang, float rhat, float x, float y, float z, const float q[3], float out[3]) {
  out[0] = out[1] = out[2] = 0.f;
  if (q[0] == 0.f && q[1] == 0.f && q[2] == 0.f) return;
  const float px = x - c.cx, py = y - c.cy, pz = z - c.cz;
  const float r = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(px, px), __fmul_rn(py, py)), __fmul_rn(pz, pz)));
  if (!(r > 0.f) || !(r < INFINITY)) return;
  // k as normalize_r finds it - searchsorted(side = 'right') clamped to [1, n_lut - 1], i.e. k_in = the last entry <= r, at most n_lut - 2 -
  // but started from the cell the forward's r^ names (r^ = 2 (k_in + frac) / n_r - 1) and walked from there: two reads, not a search
  int k_in = (int)fminf(fmaxf(floorf((rhat + 1.f) * 0.5f * (float)c.n_r), 0.f), (float)(c.n_lut - 2));
  while (k_in > 0 && lut[k_in] > r) --k_in;
  while (k_in < c.n_lut - 2 && !(lut[k_in + 1] > r)) ++k_in;
  // (reciprocals and the second root to 1 ulp: v_rcp_f32 / v_sqrt_f32 - the IEEE divisions were a tenth of the kernel's instructions)
  const float ar = 2.f * __frcp_rn((float)c.n_r * (lut[k_in + 1] - lut[k_in]));
  // yang: the same formulas on (a, b, cc) = (-px, pz, py), mapped back below
  const float a = yang ? -px : px, b = yang ? pz : py, cc = yang ? py : pz;
  const float rho2 = a * a + b * b, inv_r = __frcp_rn(r);
  const float qr = q[0] * ar * inv_r;
  float ga = qr * a, gb = qr * b, gc = qr * cc;
  if (rho2 > 0.f) {   // inside its own domain a chart has rho >= r / sqrt 2
    const float inv_rho2 = __frcp_rn(rho2);
    const float qt = q[1] * 2.f * c.th_inv * (inv_r * inv_r) * (__builtin_amdgcn_sqrtf(rho2) * inv_rho2), qp = q[2] * 2.f * c.ph_inv * inv_rho2;
    ga += qt * a * cc - qp * b;
    gb += qt * b * cc + qp * a;
    gc -= qt * rho2;
  }
  const float ox = yang ? -ga : ga, oy = yang ? gc : gb, oz = yang ? gb : gc;
  const bool ok = fabsf(ox) < INFINITY && fabsf(oy) < INFINITY && fabsf(oz) < INFINITY;   // false for NaN too
  if (ok) { out[0] = ox; out[1] = oy; out[2] = oz; }
}

// v / |v| without overflow or underflow in the squares: scaled by the largest component first.  0 for v = 0 and for anything not finite
__device__ __forceinline__ void unit3(const float v[3], float out[3]) {
  out[0] = out[1] = out[2] = 0.f;
  const float big = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fabsf(v[2]));
  const bool finite = fabsf(v[0]) < INFINITY && fabsf(v[1]) < INFINITY && fabsf(v[2]) < INFINITY;   // false for NaN too
  if (!(big > 0.f) || !finite) return;
  // (reciprocal and reciprocal square root to 1 ulp, v_rcp_f32 / v_rsq_f32, as chart_jt: the IEEE divisions and the root were a
  // seventh of the kernel's vector instructions)
  const float rb = __frcp_rn(big);
  const float a = __fmul_rn(v[0], rb), b = __fmul_rn(v[1], rb), c = __fmul_rn(v[2], rb);
  const float rl = __builtin_amdgcn_rsqf(__fadd_rn(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)), __fmul_rn(c, c)));   // the sum is in [1, 3]
  out[0] = __fmul_rn(a, rl); out[1] = __fmul_rn(b, rl); out[2] = __fmul_rn(c, rl);
}

constexpr int RG_LUT_LDS = 1024;  // radius LUTs up to this many entries are walked in LDS

}  // namespace
