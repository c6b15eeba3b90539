// Multi-sphere images (include/egonerf_hip.h: ego_msi_layers, ego_msi_render, ego_msi_render_backward, ego_msi_project, ego_msi_adam_step): a scene integrated once into L concentric
// shells of premultiplied RGBA around a centre, and views from nearby positions composited from the shells alone - L sphere
// intersections, L bilinear taps and an "over" per pixel, no tables and no MLP.
//
// k_msi_layers runs once per baked chunk: one thread per (texel, layer), layer-major so that a wave's stores are one contiguous run of
// whole texels; the thread finds its run of the ray's ascending z by bisection and folds it in sample order.  k_msi_render is the playback
// hot path: one thread per ray, wave64, no LDS; a tap is four loads of one whole texel (16 B float, 8 B half), neighbouring pixels hit
// neighbouring texels, the radii are wave-uniform.  All arithmetic is fp32 and - like the whole library (-ffp-contract=off) and once more
// by the pragma below - never contracted: tests/msi_ref.py restates both kernels operation by operation.  k_msi_render_bwd is playback's
// backward for float32 texels (float atomic adds to the taps), k_msi_project the clamp that follows an optimiser step, k_msi_adam an Adam step
// of the texels a batch touched, clamp and zeroing of the gradient included.
#include <algorithm>

#include "ego_device.h"
#include "ego_host.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// one texel <-> four floats; a half texel is rounded to nearest even on the way out and exact on the way in
__device__ __forceinline__ f32x4 load_texel(const float* base, int64_t i) { return ((const f32x4*)base)[i]; }
__device__ __forceinline__ f32x4 load_texel(const _Float16* base, int64_t i) {
  const f16x4 h = ((const f16x4*)base)[i];
  return f32x4{(float)h.x, (float)h.y, (float)h.z, (float)h.w};
}
__device__ __forceinline__ void store_texel(float* base, int64_t i, f32x4 v) { ((f32x4*)base)[i] = v; }
__device__ __forceinline__ void store_texel(_Float16* base, int64_t i, f32x4 v) {
  ((f16x4*)base)[i] = f16x4{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
}

// Thread i = k N + n: layer k of ray n.  Its samples are those with bounds[k] <= z < bounds[k + 1]: z ascends along a ray, so they form
// one run, whose first index is found by bisection; every read of the ray's rows is guarded by s < S.
template <typename T>
__global__ __launch_bounds__(256) void k_msi_layers(const float* __restrict__ z, const float* __restrict__ alpha, int alpha_stride,
                                                    const float* __restrict__ rgb, int64_t N, int S, const float* __restrict__ bounds, int L,
                                                    int64_t first, int64_t texels, T* __restrict__ layers) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * L) return;
  const int k = (int)(i / N);
  const int64_t n = i - (int64_t)k * N;
  const float lo = bounds[k], hi = bounds[k + 1];
  const float* zr = z + n * S;
  int a = 0, b = S;   // the first s in [0, S] with z[s] >= lo
  while (a < b) {
    const int m = (a + b) >> 1;
    if (zr[m] < lo) a = m + 1; else b = m;
  }
  const float* ar = alpha + n * alpha_stride;
  const float* cr = rgb + n * S * 3;
  float t = 1.f, r = 0.f, g = 0.f, bl = 0.f;
  for (int s = a; s < S && zr[s] < hi; ++s) {
    const float al = ar[s];
    const float w = t * al;
    r = r + w * cr[3 * s];
    g = g + w * cr[3 * s + 1];
    bl = bl + w * cr[3 * s + 2];
    t = t * (1.f - al);
  }
  store_texel(layers, (int64_t)k * texels + first + n, f32x4{r, g, bl, 1.f - t});
}

struct MsiTap {
  int64_t i00, i01, i10, i11;   // texel indices inside one [Hm][Wm] image
  float fr, fc;
};

// The bilinear footprint of unit direction (ux, uy, uz) in an Hm x Wm equirectangular image: the inverse of erp_ray's mapping under an
// identity pose.  Columns wrap, rows clamp.  The float coordinates are clamped to [-1, Hm] / [-1, Wm] before the integer conversion -
// a no-op for a unit direction, and what keeps the indices inside the image for a NaN or a non-unit one.
__device__ __forceinline__ MsiTap msi_tap(float ux, float uy, float uz, int Hm, int Wm) {
  const float PI = 3.14159265358979323846f;
  const float theta = asinf(fminf(fmaxf(uy, -1.f), 1.f));
  const float phi = atan2f(-ux, -uz);
  float row = (1.f - (2.f * theta) / PI) * ((float)Hm * 0.5f) - 0.5f;
  float col = (1.f - phi / PI) * ((float)Wm * 0.5f) - 0.5f;
  row = fminf(fmaxf(row, -1.f), (float)Hm);
  col = fminf(fmaxf(col, -1.f), (float)Wm);
  const float r0f = floorf(row), c0f = floorf(col);
  const int r0 = (int)r0f, c0 = (int)c0f;
  const int ra = min(max(r0, 0), Hm - 1), rb = min(max(r0 + 1, 0), Hm - 1);
  // c0 lies in [-1, Wm] after the clamp: one step brings it into [0, Wm - 1], and its right neighbour follows from that
  const int ca = c0 < 0 ? c0 + Wm : (c0 >= Wm ? c0 - Wm : c0);
  const int cb = ca + 1 == Wm ? 0 : ca + 1;
  MsiTap t;
  t.i00 = (int64_t)ra * Wm + ca; t.i01 = (int64_t)ra * Wm + cb;
  t.i10 = (int64_t)rb * Wm + ca; t.i11 = (int64_t)rb * Wm + cb;
  t.fr = row - r0f; t.fc = col - c0f;
  return t;
}

template <typename T>
__device__ __forceinline__ f32x4 msi_sample(const T* __restrict__ img, const MsiTap& t) {
  const f32x4 v00 = load_texel(img, t.i00), v01 = load_texel(img, t.i01), v10 = load_texel(img, t.i10), v11 = load_texel(img, t.i11);
  const float gc = 1.f - t.fc, gr = 1.f - t.fr;
  // channel by channel in scalar arithmetic (the file is built without the SLP vectoriser as well): no packed fp32 instruction gets to
  // broadcast one half of a weight pair.  The one packed instruction the compiler still forms in k_msi_render squares
  // the (dy, dz) pair as it was loaded, half by half, without op_sel
  f32x4 o;
  o.x = (v00.x * gc + v01.x * t.fc) * gr + (v10.x * gc + v11.x * t.fc) * t.fr;
  o.y = (v00.y * gc + v01.y * t.fc) * gr + (v10.y * gc + v11.y * t.fc) * t.fr;
  o.z = (v00.z * gc + v01.z * t.fc) * gr + (v10.z * gc + v11.z * t.fc) * t.fr;
  o.w = (v00.w * gc + v01.w * t.fc) * gr + (v10.w * gc + v11.w * t.fc) * t.fr;
  return o;
}

// A ray as every MSI kernel sees it: p = o - c, d = the unit direction, dn = the given direction's length, b = p.d, bb_pp = b b - p.p,
// pn = |p|.  The direction is normalised first - exact for a direction of length exactly 1, a rounding otherwise - so that the pinhole
// cameras' rays, which are not normalised, cross the shells where they should.
struct MsiRay {
  float px, py, pz, dx, dy, dz, dn, b, bb_pp, pn;
};

__device__ __forceinline__ MsiRay msi_ray(const float* __restrict__ rays, int64_t i, float cx, float cy, float cz) {
  const f32x2* in = (const f32x2*)(rays + i * 6);   // 24 bytes per row, 8-byte aligned (checked by the entry point)
  const f32x2 q0 = in[0], q1 = in[1], q2 = in[2];
  MsiRay r;
  r.px = q0.x - cx; r.py = q0.y - cy; r.pz = q1.x - cz;
  r.dn = __fsqrt_rn((q1.y * q1.y + q2.x * q2.x) + q2.y * q2.y);
  r.dx = q1.y / r.dn; r.dy = q2.x / r.dn; r.dz = q2.y / r.dn;
  const float pp = (r.px * r.px + r.py * r.py) + r.pz * r.pz;
  r.b = (r.px * r.dx + r.py * r.dy) + r.pz * r.dz;
  r.bb_pp = r.b * r.b - pp;
  r.pn = __fsqrt_rn(pp);
  return r;
}

// Layer of radius R is crossed (from inside) at t = -b + sqrt(b b - p.p + R R); the tap is the crossing point's direction from the centre
__device__ __forceinline__ float msi_cross(const MsiRay& r, float R) { return __fsqrt_rn(fmaxf(r.bb_pp + R * R, 0.f)) - r.b; }
__device__ __forceinline__ MsiTap msi_layer_tap(const MsiRay& r, float R, float tk, int Hm, int Wm) {
  return msi_tap((r.px + tk * r.dx) / R, (r.py + tk * r.dy) / R, (r.pz + tk * r.dz) / R, Hm, Wm);
}

// One thread per ray.  A layer is skipped when the eye is not inside it (R_k <= |p|); the "over" runs front to back through every
// layer - no early exit; depth is reported in the GIVEN ray's parameter, as a model does.
template <typename T>
__global__ __launch_bounds__(256) void k_msi_render(const float* __restrict__ rays, int64_t N, float cx, float cy, float cz,
                                                    const float* __restrict__ radii, int L, int Hm, int Wm, const T* __restrict__ layers,
                                                    const T* __restrict__ background, float* __restrict__ rgb, float* __restrict__ depth) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const MsiRay ray = msi_ray(rays, i, cx, cy, cz);
  const int64_t texels = (int64_t)Hm * Wm;
  float T_ = 1.f, r = 0.f, g = 0.f, bl = 0.f, dp = 0.f;
  for (int k = 0; k < L; ++k) {
    const float R = radii[k];
    if (R <= ray.pn) continue;
    const float tk = msi_cross(ray, R);
    const f32x4 v = msi_sample(layers + (int64_t)k * texels * 4, msi_layer_tap(ray, R, tk, Hm, Wm));
    r = r + T_ * v.x;
    g = g + T_ * v.y;
    bl = bl + T_ * v.z;
    dp = dp + (T_ * v.w) * (tk / ray.dn);
    T_ = T_ * (1.f - v.w);
  }
  if (background) {   // the shell at infinity, seen in the ray's direction; its alpha is taken as 1
    const f32x4 v = msi_sample(background, msi_tap(ray.dx, ray.dy, ray.dz, Hm, Wm));
    r = r + T_ * v.x;
    g = g + T_ * v.y;
    bl = bl + T_ * v.z;
  }
  rgb[i * 3] = r; rgb[i * 3 + 1] = g; rgb[i * 3 + 2] = bl;
  depth[i] = dp;
}

// ---- the backward of playback (DESIGN.md 3.3 "Refinement") --------------------------------------------------------------------------
// rgb = sum_k T_k C_k + T_end C_bg over the live layers, T_k = prod_{j<k} (1 - A_j).  With g = d loss / d rgb:
//   dC_k = T_k g,  dA_k = -T_k B_{k+1},  B_k = C_k.g + (1 - A_k) B_{k+1},  B_end = C_bg.g (0 without a background),  dC_bg = T_end g.
// Nothing divides by (1 - A_k): a forward walk stores T_k of every live layer in the workspace ([L][N], so a wave's accesses are
// contiguous), a walk back carries B.  Behind a layer with A = 1 every T_k is exactly 0 and so is everything added there.  A sample's
// gradient goes to its four taps with the forward's weights, by float atomic adds: the sums depend on the order of arrival.

__device__ __forceinline__ float dot_g(const f32x4 v, float gx, float gy, float gz) { return (v.x * gx + v.y * gy) + v.z * gz; }

// The forward walk: T_k of every live layer -> ws[k N + i]; returns T_end
__device__ __forceinline__ float msi_store_transmittance(const MsiRay& ray, bool in, int64_t i, int64_t N, const float* __restrict__ radii,
                                                         int L, int Hm, int Wm, const float* __restrict__ layers, float* __restrict__ ws) {
  const int64_t texels = (int64_t)Hm * Wm;
  float T_ = 1.f;
  for (int k = 0; k < L; ++k) {
    const float R = radii[k];
    if (!in || R <= ray.pn) continue;
    ws[(int64_t)k * N + i] = T_;
    const f32x4 v = msi_sample(layers + (int64_t)k * texels * 4, msi_layer_tap(ray, R, msi_cross(ray, R), Hm, Wm));
    T_ = T_ * (1.f - v.w);
  }
  return T_;
}

// The adds: the four lanes of a quad take their four rays in turn, and for each lane c adds channel c - a wave's add instruction is
// sixteen whole texels (16 B each), not sixty-four single dwords in sixty-four places (a lane per ray with sixteen adds of its own per
// layer was measured first: 3.5 x slower).  The values cross the lanes by DPP quad broadcasts, which every lane of the wave
// has to execute: no lane returns early, a lane without a ray or a ray outside the layer carries zeros.
template <int J>
__device__ __forceinline__ float quad_f(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), J * 0x55, 0xf, 0xf, true));
}
template <int J>
__device__ __forceinline__ int quad_i(int x) { return __builtin_amdgcn_update_dpp(0, x, J * 0x55, 0xf, 0xf, true); }

struct QuadTap {
  int i00, i01, i10, i11;   // texels < 2^31 (checked by the entry point)
  float fr, fc;
};

// One add instruction: lane (q, c) adds `a` to channel c of `texel`.  Every lane of the wave arrives here.  The first branch matters only
// for images of a few texels: when the sixteen quads aim at ONE texel the wave sums their shares first, pairwise, and adds once.  On an
// image of useful size the rays of a wave never all share a texel and it costs one wave-uniform test per add (nothing measurable).  It is
// there for accuracy, not speed: thousands of shares added one by one to a single float32 wander further from the exact sum than the
// tolerance of tests/test_hip_msi_refine.py allows; summed sixteen at a time they do not.
__device__ __forceinline__ void add_quad(float* __restrict__ img, int texel, int c, float a) {
  if (__all(texel == __builtin_amdgcn_readfirstlane(texel))) {
    a = a + __shfl_xor(a, 4);
    a = a + __shfl_xor(a, 8);
    a = a + __shfl_xor(a, 16);
    a = a + __shfl_xor(a, 32);
    if ((threadIdx.x & 63) >= 4) return;
  }
  if (a != 0.f) unsafeAtomicAdd(img + (int64_t)texel * 4 + c, a);
}

template <int J>
__device__ __forceinline__ void scatter_quad_from(float* __restrict__ img, const QuadTap& t, const f32x4 dv, int c) {
  const float x = quad_f<J>(dv.x), y = quad_f<J>(dv.y), z = quad_f<J>(dv.z), w = quad_f<J>(dv.w);
  const float mine = c == 0 ? x : (c == 1 ? y : (c == 2 ? z : w));
  const float fr = quad_f<J>(t.fr), fc = quad_f<J>(t.fc);
  const int i00 = quad_i<J>(t.i00), i01 = quad_i<J>(t.i01), i10 = quad_i<J>(t.i10), i11 = quad_i<J>(t.i11);
  const float gc = 1.f - fc, gr = 1.f - fr;
  add_quad(img, i00, c, mine * (gc * gr));
  add_quad(img, i01, c, mine * (fc * gr));
  add_quad(img, i10, c, mine * (gc * fr));
  add_quad(img, i11, c, mine * (fc * fr));
}

// live == false: the lane contributes nothing (zero gradient, zero weights on texel 0), whatever its tap holds
__device__ __forceinline__ void scatter_quad(float* __restrict__ img, const MsiTap& tap, bool live, f32x4 dv, int c) {
  QuadTap t;
  t.i00 = live ? (int)tap.i00 : 0; t.i01 = live ? (int)tap.i01 : 0; t.i10 = live ? (int)tap.i10 : 0; t.i11 = live ? (int)tap.i11 : 0;
  t.fr = live ? tap.fr : 0.f; t.fc = live ? tap.fc : 0.f;
  if (!live) dv = f32x4{0.f, 0.f, 0.f, 0.f};
  scatter_quad_from<0>(img, t, dv, c);
  scatter_quad_from<1>(img, t, dv, c);
  scatter_quad_from<2>(img, t, dv, c);
  scatter_quad_from<3>(img, t, dv, c);
}

__global__ __launch_bounds__(256) void k_msi_render_bwd(const float* __restrict__ rays, int64_t N, float cx, float cy, float cz,
                                                        const float* __restrict__ radii, int L, int Hm, int Wm,
                                                        const float* __restrict__ layers, const float* __restrict__ background,
                                                        const float* __restrict__ g_rgb, float* __restrict__ g_layers,
                                                        float* __restrict__ g_background, float* __restrict__ ws) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = i < N;
  const int64_t ii = in ? i : N - 1;   // a lane past the end reads the last ray and adds nothing
  const int c = threadIdx.x & 3;
  const MsiRay ray = msi_ray(rays, ii, cx, cy, cz);
  const int64_t texels = (int64_t)Hm * Wm;
  const float gx = g_rgb[ii * 3], gy = g_rgb[ii * 3 + 1], gz = g_rgb[ii * 3 + 2];
  const float T_end = msi_store_transmittance(ray, in, ii, N, radii, L, Hm, Wm, layers, ws);
  float B = 0.f;
  if (background) {
    const MsiTap tap = msi_tap(ray.dx, ray.dy, ray.dz, Hm, Wm);
    B = dot_g(msi_sample(background, tap), gx, gy, gz);
    if (g_background) scatter_quad(g_background, tap, in, f32x4{T_end * gx, T_end * gy, T_end * gz, 0.f}, c);
  }
  if (!g_layers) return;   // only the background's gradient was asked for (the same for every lane)
  for (int k = L - 1; k >= 0; --k) {
    const float R = radii[k];
    const bool live = in && !(R <= ray.pn);
    const float Tk = live ? ws[(int64_t)k * N + ii] : 0.f;
    const MsiTap tap = msi_layer_tap(ray, R, msi_cross(ray, R), Hm, Wm);
    const f32x4 v = msi_sample(layers + (int64_t)k * texels * 4, tap);
    scatter_quad(g_layers + (int64_t)k * texels * 4, tap, live, f32x4{Tk * gx, Tk * gy, Tk * gz, -(Tk * B)}, c);
    if (live) B = dot_g(v, gx, gy, gz) + (1.f - v.w) * B;
  }
}

// C <- max(C, 0), A <- clamp(A, 0, 1); a NaN becomes 0.  The one clamp of k_msi_project and k_msi_adam: their bits agree
__device__ __forceinline__ f32x4 msi_project_texel(const f32x4 v) {
  return f32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fminf(fmaxf(v.w, 0.f), 1.f)};
}

// in place
__global__ __launch_bounds__(256) void k_msi_project(float* __restrict__ texels, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  store_texel(texels, i, msi_project_texel(load_texel(texels, i)));
}

// ---- Adam on every texel's own clock (DESIGN.md 3.3 "Texel Adam") -------------------------------------------------------------------
// One lane per texel, a streaming pass over the gradient: 16 B per lane, and a lane whose four gradient values all compare equal to 0
// is done - it reads and writes nothing else.  A touched lane (a NaN compares unequal: touched) advances the texel's own step count,
// its moments - m and v of one texel in one 32-byte record, so that a scattered hit opens one line for them, not two - and the texel,
// torch.optim.Adam's rule in its order with the bias corrections read from a table at the texel's count.  No atomics, no LDS: a texel
// belongs to one lane, the result does not depend on the schedule.
struct TexelAdam {
  float lr, b1, b2, c1, c2, eps;   // c1 = 1 - b1, c2 = 1 - b2, rounded once
  const f32x2* bias;               // [n_bias]: {1 - b1^t, sqrt(1 - b2^t)} at t - 1
  int n_bias, flags;
};

// one channel: the moments, then the step; float32, every operation rounded on its own
__device__ __forceinline__ float adam_m(const TexelAdam& a, float m, float g) { return a.b1 * m + a.c1 * g; }
__device__ __forceinline__ float adam_v(const TexelAdam& a, float v, float g) { return a.b2 * v + (a.c2 * g) * g; }
__device__ __forceinline__ float adam_p(const TexelAdam& a, float p, float m, float v, float step, float root) {
  return p - (step * m) / (__fsqrt_rn(v) / root + a.eps);
}

__device__ __forceinline__ void adam_texel(const TexelAdam& a, float* __restrict__ texels, float* __restrict__ grad,
                                           float* __restrict__ moments, int* __restrict__ hits, int64_t i, const f32x4 g) {
  const int h = hits[i];
  const int t = h == 0x7fffffff ? h : h + 1;   // saturating
  hits[i] = t;
  const f32x2 c = a.bias[max(min(t, a.n_bias), 1) - 1];   // t >= 1 unless the caller's counts were negative: the read stays in the table
  const float step = a.lr / c.x;
  const f32x4 m0 = load_texel(moments, 2 * i), v0 = load_texel(moments, 2 * i + 1), p0 = load_texel(texels, i);
  const f32x4 m{adam_m(a, m0.x, g.x), adam_m(a, m0.y, g.y), adam_m(a, m0.z, g.z), adam_m(a, m0.w, g.w)};
  const f32x4 v{adam_v(a, v0.x, g.x), adam_v(a, v0.y, g.y), adam_v(a, v0.z, g.z), adam_v(a, v0.w, g.w)};
  const f32x4 p{adam_p(a, p0.x, m.x, v.x, step, c.y), adam_p(a, p0.y, m.y, v.y, step, c.y), adam_p(a, p0.z, m.z, v.z, step, c.y),
                adam_p(a, p0.w, m.w, v.w, step, c.y)};
  store_texel(moments, 2 * i, m);
  store_texel(moments, 2 * i + 1, v);
  store_texel(texels, i, (a.flags & EGO_TEXEL_ADAM_PROJECT) ? msi_project_texel(p) : p);
  if (a.flags & EGO_TEXEL_ADAM_ZERO_GRAD) store_texel(grad, i, f32x4{0.f, 0.f, 0.f, 0.f});
}

// A lane takes texels i, i + stride, ...; the gradients of ADAM_AHEAD of them are loaded before the first is looked at, so that a
// wave has 4 KiB of gradient in flight, not 1.  A lane past the end holds a zero gradient: untouched.  The depth matters little
// (DESIGN.md 3.3 holds the figures of experiment builds with 1, 4 and 8; such a build edits the constant below: the project keeps
// no switch for an experiment in its kernel sources).  With at most 2048 workgroups the stride is 524288 texels: images of up to that many
// texels only ever use the first of the ADAM_AHEAD bodies, a 1024 x 2048 layer stack uses all of them over many rounds.
constexpr int ADAM_AHEAD = 4;
constexpr int ADAM_MAX_BLOCKS = 2048;   // a memory-bound pass: 8 workgroups per CU, the rest by the stride
__global__ __launch_bounds__(256) void k_msi_adam(float* __restrict__ texels, float* __restrict__ grad, float* __restrict__ moments,
                                                  int* __restrict__ hits, int64_t n, const TexelAdam a) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x; first < n; first += ADAM_AHEAD * stride) {
    f32x4 g[ADAM_AHEAD];
#pragma unroll
    for (int j = 0; j < ADAM_AHEAD; ++j) {
      const int64_t i = first + j * stride;
      g[j] = i < n ? load_texel(grad, i) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < ADAM_AHEAD; ++j) {
      if (g[j].x == 0.f && g[j].y == 0.f && g[j].z == 0.f && g[j].w == 0.f) continue;
      adam_texel(a, texels, grad, moments, hits, first + j * stride, g[j]);
    }
  }
}

}  // namespace

extern "C" {

int ego_msi_layers(const float* z, const float* alpha, int32_t alpha_stride, const float* rgb, int64_t N, int32_t S, const float* bounds,
                   int32_t L, int64_t first, int64_t texels, int32_t texel_type, void* layers, void* stream) {
  EGO_TRACE("ego_msi_layers");
  EGO_REQUIRE(N >= 0 && S >= 1 && L >= 1, "msi_layers: N < 0, S < 1 or L < 1");
  if (alpha_stride == 0) alpha_stride = S;
  EGO_REQUIRE(alpha_stride >= S, "msi_layers: alpha_stride < S");
  EGO_REQUIRE(texel_type == EGO_MSI_F32 || texel_type == EGO_MSI_F16, "msi_layers: unknown texel type");
  EGO_REQUIRE(first >= 0 && texels >= 1 && first <= texels && N <= texels - first, "msi_layers: texel window [first, first + N) outside the image");
  EGO_REQUIRE(N * (int64_t)L < (1ll << 31) * 256, "msi_layers: N * L too large for one launch");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(z && alpha && rgb && bounds && layers, "msi_layers: null argument");
  EGO_REQUIRE(((uintptr_t)layers & (texel_type == EGO_MSI_F32 ? 15 : 7)) == 0, "msi_layers: layers must be aligned to one texel (16 B float, 8 B half)");
  const unsigned blocks = nblk(N * (int64_t)L, 256);
  if (texel_type == EGO_MSI_F32)
    k_msi_layers<float><<<blocks, 256, 0, (hipStream_t)stream>>>(z, alpha, alpha_stride, rgb, N, S, bounds, L, first, texels, (float*)layers);
  else
    k_msi_layers<_Float16><<<blocks, 256, 0, (hipStream_t)stream>>>(z, alpha, alpha_stride, rgb, N, S, bounds, L, first, texels, (_Float16*)layers);
  return ego_launch_status("k_msi_layers");
}

int ego_msi_render(const float* rays, int64_t N, float cx, float cy, float cz, const float* radii, int32_t L, int32_t Hm, int32_t Wm,
                   int32_t texel_type, const void* layers, const void* background, float* rgb, float* depth, void* stream) {
  EGO_TRACE("ego_msi_render");
  EGO_REQUIRE(N >= 0 && L >= 1 && Hm >= 1 && Wm >= 1, "msi_render: N < 0, or L, Hm or Wm < 1");
  EGO_REQUIRE(cx == cx && cy == cy && cz == cz, "msi_render: NaN centre");
  EGO_REQUIRE(texel_type == EGO_MSI_F32 || texel_type == EGO_MSI_F16, "msi_render: unknown texel type");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(rays && radii && layers && rgb && depth, "msi_render: null argument");
  const uintptr_t mask = texel_type == EGO_MSI_F32 ? 15 : 7;
  EGO_REQUIRE(((uintptr_t)rays & 7) == 0 && ((uintptr_t)layers & mask) == 0 && ((uintptr_t)background & mask) == 0,
              "msi_render: rays must be 8-byte aligned, layers and background aligned to one texel (16 B float, 8 B half)");
  const unsigned blocks = nblk(N, 256);
  if (texel_type == EGO_MSI_F32)
    k_msi_render<float><<<blocks, 256, 0, (hipStream_t)stream>>>(rays, N, cx, cy, cz, radii, L, Hm, Wm, (const float*)layers,
                                                                 (const float*)background, rgb, depth);
  else
    k_msi_render<_Float16><<<blocks, 256, 0, (hipStream_t)stream>>>(rays, N, cx, cy, cz, radii, L, Hm, Wm, (const _Float16*)layers,
                                                                    (const _Float16*)background, rgb, depth);
  return ego_launch_status("k_msi_render");
}

int64_t ego_msi_render_backward_workspace_bytes(int64_t N, int32_t L) {
  if (N < 0 || L < 1) return -1;
  return N * (int64_t)L * (int64_t)sizeof(float);
}

int ego_msi_render_backward(const float* rays, int64_t N, float cx, float cy, float cz, const float* radii, int32_t L, int32_t Hm, int32_t Wm,
                            int32_t texel_type, const void* layers, const void* background, const float* g_rgb, float* g_layers,
                            float* g_background, void* workspace, int64_t workspace_bytes, void* stream) {
  EGO_TRACE("ego_msi_render_backward");
  EGO_REQUIRE(N >= 0 && L >= 1 && Hm >= 1 && Wm >= 1, "msi_render_backward: N < 0, or L, Hm or Wm < 1");
  EGO_REQUIRE(cx == cx && cy == cy && cz == cz, "msi_render_backward: NaN centre");
  EGO_REQUIRE(texel_type == EGO_MSI_F32 || texel_type == EGO_MSI_F16, "msi_render_backward: unknown texel type");
  EGO_REQUIRE(texel_type == EGO_MSI_F32, "msi_render_backward: half texels have no gradient (convert the image to float32 texels)");
  EGO_REQUIRE((int64_t)Hm * Wm < (1ll << 31), "msi_render_backward: Hm * Wm must stay below 2^31");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(rays && radii && layers && g_rgb && (g_layers || g_background), "msi_render_backward: null argument");
  EGO_REQUIRE(!g_background || background, "msi_render_backward: g_background without a background");
  EGO_REQUIRE(((uintptr_t)rays & 7) == 0 && ((uintptr_t)layers & 15) == 0 && ((uintptr_t)background & 15) == 0 &&
                  ((uintptr_t)g_layers & 15) == 0 && ((uintptr_t)g_background & 15) == 0 && ((uintptr_t)g_rgb & 3) == 0,
              "msi_render_backward: rays must be 8-byte aligned, layers, background and their gradients aligned to one texel (16 B)");
  EGO_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0 && workspace_bytes >= ego_msi_render_backward_workspace_bytes(N, L),
              "msi_render_backward: workspace missing, misaligned or smaller than ego_msi_render_backward_workspace_bytes(N, L)");
  k_msi_render_bwd<<<nblk(N, 256), 256, 0, (hipStream_t)stream>>>(rays, N, cx, cy, cz, radii, L, Hm, Wm, (const float*)layers, (const float*)background,
                                                                  g_rgb, g_layers, g_background, (float*)workspace);
  return ego_launch_status("k_msi_render_bwd");
}

int ego_msi_project(float* texels, int64_t n_texels, void* stream) {
  EGO_TRACE("ego_msi_project");
  EGO_REQUIRE(n_texels >= 0 && n_texels < (1ll << 31) * 256, "msi_project: n_texels < 0 or too large for one launch");
  if (n_texels == 0) return EGO_OK;
  EGO_REQUIRE(texels, "msi_project: null argument");
  EGO_REQUIRE(((uintptr_t)texels & 15) == 0, "msi_project: texels must be aligned to one texel (16 B float)");
  k_msi_project<<<nblk(n_texels, 256), 256, 0, (hipStream_t)stream>>>(texels, n_texels);
  return ego_launch_status("k_msi_project");
}

int ego_msi_adam_step(float* texels, float* grad, float* moments, int32_t* hits, int64_t n_texels, float lr, float beta1, float beta2,
                      float eps, const float* bias, int32_t n_bias, int32_t flags, void* stream) {
  EGO_TRACE("ego_msi_adam_step");
  // the strided launch itself has no limit; the bound is ego_msi_project's, so that the two entry points take the same tensors
  EGO_REQUIRE(n_texels >= 0 && n_texels < (1ll << 31) * 256, "msi_adam_step: n_texels < 0 or too large (2^39 texels, ego_msi_project's limit)");
  EGO_REQUIRE((flags & ~(EGO_TEXEL_ADAM_PROJECT | EGO_TEXEL_ADAM_ZERO_GRAD)) == 0, "msi_adam_step: unknown flag bits");
  EGO_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "msi_adam_step: betas must lie in [0, 1)");
  EGO_REQUIRE(eps > 0.f, "msi_adam_step: eps must be positive");
  EGO_REQUIRE(n_bias >= 1, "msi_adam_step: n_bias < 1");
  if (n_texels == 0) return EGO_OK;
  EGO_REQUIRE(texels && grad && moments && hits && bias, "msi_adam_step: null argument");
  EGO_REQUIRE(((uintptr_t)texels & 15) == 0 && ((uintptr_t)grad & 15) == 0 && ((uintptr_t)moments & 15) == 0 && ((uintptr_t)hits & 3) == 0 &&
                  ((uintptr_t)bias & 7) == 0,
              "msi_adam_step: texels, grad and moments must be aligned to one texel (16 B), hits to 4 B, bias to one entry (8 B)");
  TexelAdam a;
  a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.c1 = 1.f - beta1; a.c2 = 1.f - beta2; a.eps = eps;
  a.bias = (const f32x2*)bias; a.n_bias = n_bias; a.flags = flags;
  const unsigned blocks = (unsigned)std::min<int64_t>(nblk(n_texels, 256), ADAM_MAX_BLOCKS);
  k_msi_adam<<<blocks, 256, 0, (hipStream_t)stream>>>(texels, grad, moments, hits, n_texels, a);
  return ego_launch_status("k_msi_adam");
}

}  // extern "C"
