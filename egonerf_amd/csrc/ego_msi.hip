// Multi-sphere images (include/egonerf_hip.h: ego_msi_layers, ego_msi_render): a scene integrated once into L concentric
// shells of premultiplied RGBA around a centre, and views from nearby positions composited from the shells alone - L sphere
// intersections, L bilinear taps and an "over" per pixel, no tables and no MLP.
//
// k_msi_layers runs once per baked chunk: one thread per (texel, layer), layer-major so that a wave's stores are one contiguous run of
// whole texels; the thread finds its run of the ray's ascending z by bisection and folds it in sample order.  k_msi_render is the playback
// hot path: one thread per ray, wave64, no LDS; a tap is four loads of one whole texel (16 B float, 8 B half), neighbouring pixels hit
// neighbouring texels, the radii are wave-uniform.  All arithmetic is fp32 and - like the whole library (-ffp-contract=off) and once more
// by the pragma below - never contracted: tests/msi_ref.py restates both kernels operation by operation.
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

// One thread per ray.  p = o - c, d = the unit direction; layer k is crossed (from inside) at t_k = -b + sqrt(b b - p.p + R_k R_k),
// b = p.d, and skipped when the eye is not inside it (R_k <= |p|); the "over" runs front to back through every layer - no early exit.
template <typename T>
__global__ __launch_bounds__(256) void k_msi_render(const float* __restrict__ rays, int64_t N, float cx, float cy, float cz,
                                                    const float* __restrict__ radii, int L, int Hm, int Wm, const T* __restrict__ layers,
                                                    const T* __restrict__ background, float* __restrict__ rgb, float* __restrict__ depth) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const f32x2* in = (const f32x2*)(rays + i * 6);   // 24 bytes per row, 8-byte aligned (checked by the entry point)
  const f32x2 q0 = in[0], q1 = in[1], q2 = in[2];
  const float px = q0.x - cx, py = q0.y - cy, pz = q1.x - cz;
  // the direction is normalised first - exact for a direction of length exactly 1, a rounding otherwise - so that the pinhole cameras'
  // rays, which are not normalised, cross the shells where they should; depth is reported in the GIVEN ray's parameter, as a model does
  const float dn = __fsqrt_rn((q1.y * q1.y + q2.x * q2.x) + q2.y * q2.y);
  const float dx = q1.y / dn, dy = q2.x / dn, dz = q2.y / dn;
  const float pp = (px * px + py * py) + pz * pz;
  const float b = (px * dx + py * dy) + pz * dz;
  const float bb_pp = b * b - pp;
  const float pn = __fsqrt_rn(pp);
  const int64_t texels = (int64_t)Hm * Wm;
  float T_ = 1.f, r = 0.f, g = 0.f, bl = 0.f, dp = 0.f;
  for (int k = 0; k < L; ++k) {
    const float R = radii[k];
    if (R <= pn) continue;
    const float tk = __fsqrt_rn(fmaxf(bb_pp + R * R, 0.f)) - b;
    const MsiTap tap = msi_tap((px + tk * dx) / R, (py + tk * dy) / R, (pz + tk * dz) / R, Hm, Wm);
    const f32x4 v = msi_sample(layers + (int64_t)k * texels * 4, tap);
    r = r + T_ * v.x;
    g = g + T_ * v.y;
    bl = bl + T_ * v.z;
    dp = dp + (T_ * v.w) * (tk / dn);
    T_ = T_ * (1.f - v.w);
  }
  if (background) {   // the shell at infinity, seen in the ray's direction; its alpha is taken as 1
    const f32x4 v = msi_sample(background, msi_tap(dx, dy, dz, Hm, Wm));
    r = r + T_ * v.x;
    g = g + T_ * v.y;
    bl = bl + T_ * v.z;
  }
  rgb[i * 3] = r; rgb[i * 3 + 1] = g; rgb[i * 3 + 2] = bl;
  depth[i] = dp;
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

}  // extern "C"
