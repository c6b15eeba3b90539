// libegonerf_hip.so: the separately callable stages (rows A-E, G-J, M of SURVEY 8a), the table pooling and the equirectangular
// camera rays.  gfx950 only.
#include "ego_device.h"
#include "ego_host.h"
#include "ego_density.h"

// =============================================================================================
// Row A  — sample schedule -> points (sched_z: ego_device.h)      models/EgoNeRF.py:56-87
// =============================================================================================
__global__ void k_sample_ray_exp(const float* __restrict__ rays, const float* __restrict__ r_sched,
                                 const float* __restrict__ jitter, float near_, int64_t N, int S,
                                 float* __restrict__ xyz, float* __restrict__ z_out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * S) return;
  const int64_t ray = idx / S;
  const int s = (int)(idx - ray * S);
  const float z = sched_z(r_sched, jitter, ray, s, S, near_);
  if (z_out) z_out[idx] = z;
  if (xyz) {
    const float* R = rays + ray * 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) xyz[idx * 3 + k] = __fadd_rn(R[k], __fmul_rn(R[3 + k], z));
  }
}

// =============================================================================================
// Rows B, C
// =============================================================================================
__global__ void k_from_cartesian(DevCoords c, const float* __restrict__ xyz, int64_t M, float* __restrict__ c7) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const YinYang y = yinyang_from_xyz(xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], c);
  float* o = c7 + i * 7;
  const int b = y.yang ? 3 : 0, nb = y.yang ? 0 : 3;
  o[b] = y.r; o[b + 1] = y.th; o[b + 2] = y.ph;
  o[nb] = 0.f; o[nb + 1] = 0.f; o[nb + 2] = 0.f;
  o[6] = y.yang ? 1.f : 0.f;
}

__global__ void k_normalize_coord(DevCoords c, const float* __restrict__ c7, int64_t M, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const float* p = c7 + i * 7;
  float* o = out + i * 7;
#pragma unroll
  for (int b = 0; b < 6; b += 3) {
    o[b] = normalize_r(p[b], c.r_lut, c.n_lut, c.n_r);
    o[b + 1] = normalize_ang(p[b + 1], c.th_near, c.th_inv);
    o[b + 2] = normalize_ang(p[b + 2], c.ph_near, c.ph_inv);
  }
  o[6] = p[6];
}

// =============================================================================================
// Row D / D' — density feature: sum_i relu(sum_c P_ic * L_ic)      models/EgoNeRF.py:291-347, 232-289
// lane = sample; the lookup itself is density_lookup<C> (ego_density.h).
// =============================================================================================
template <int C>
__global__ void k_density_feature(DevField F, const float* __restrict__ c7n, int64_t M, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const float* p = c7n + i * 7;
  const int g = (p[6] == 0.f) ? 0 : 1;
  const int b = g ? 3 : 0;
  out[i] = density_lookup<C>(F, g, p[b], p[b + 1], p[b + 2]);
}

// =============================================================================================
// Row E
// =============================================================================================
__global__ void k_feature2density(const float* __restrict__ f, int64_t M, int softplus, float shift,
                                  float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  out[i] = softplus ? softplus_shift(f[i], shift) : fmaxf(f[i], 0.f);
}

// one wave per ray; transmittance = exclusive product of (1 - alpha + 1e-10)   tensorBase.py:22-27
__global__ void k_raw2alpha(const float* __restrict__ sigma, const float* __restrict__ dist, int64_t N, int S,
                            float* __restrict__ alpha, float* __restrict__ weight, float* __restrict__ bg) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (ray >= N) return;
  float carry = 1.f;
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int s = s0 + lane;
    const bool ok = s < S;
    const PassT p = transmittance_step(ok, ok ? sigma[ray * S + s] * dist[ray * S + s] : 0.f, lane);
    if (ok) {
      if (alpha) alpha[ray * S + s] = p.a;
      if (weight) weight[ray * S + s] = p.a * (carry * p.exc);
    }
    carry *= p.tot;
  }
  if (bg && lane == 0) bg[ray] = carry;
}

// Row M — occupancy lookup (occ_sample, ego_device.h)      models/EgoNeRF.py:11-24
__global__ void k_alpha_mask_sample(DevOcc O, const float* __restrict__ c7n, int64_t M, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const float* p = c7n + i * 7;
  const int g = (p[6] == 0.f) ? 0 : 1;
  const int b = g ? 3 : 0;
  out[i] = occ_sample(O, g, p[b], p[b + 1], p[b + 2]);
}

// =============================================================================================
// Row J — environment map     models/envmap.py:6-14, 26-34
// =============================================================================================
__global__ void k_envmap(const float* __restrict__ em, int h, const float* __restrict__ dirs, int64_t N,
                         float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float o[3];
  envmap_lookup(em, h, dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2], o);
  out[i * 3] = o[0]; out[i * 3 + 1] = o[1]; out[i * 3 + 2] = o[2];
}

// backward of bg_weight * sigmoid(bilinear(emission)) into d(emission); thread per ray, 12 float atomics
__global__ void k_envmap_bwd(int h, const float* __restrict__ dirs, int dstride, const float* __restrict__ g_rgb,
                             const float* __restrict__ rgb_raw, const float* __restrict__ bgw,
                             const float* __restrict__ env_map, int64_t N, float* __restrict__ g_em) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float dx = dirs[i * dstride], dy = dirs[i * dstride + 1], dz = dirs[i * dstride + 2];
  const EnvTaps t = envmap_taps(dx, dy, dz, h);
  const Lin1 &X = t.X, &Y = t.Y;
  const float b = bgw[i];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float raw = rgb_raw[i * 3 + ch];
    const float g = (raw >= 0.f && raw <= 1.f) ? g_rgb[i * 3 + ch] : 0.f;  // clamp(0,1) backward
    const float e = env_map[i * 3 + ch];
    const float ge = g * b * e * (1.f - e);
    if (ge == 0.f) continue;
    float* E = g_em + (int64_t)ch * 2 * h * h;
    unsafeAtomicAdd(E + (int64_t)Y.i0 * h + X.i0, ge * Y.w0 * X.w0);
    unsafeAtomicAdd(E + (int64_t)Y.i0 * h + X.i1, ge * Y.w0 * X.w1);
    unsafeAtomicAdd(E + (int64_t)Y.i1 * h + X.i0, ge * Y.w1 * X.w0);
    unsafeAtomicAdd(E + (int64_t)Y.i1 * h + X.i1, ge * Y.w1 * X.w1);
  }
}

// Row G alternative — SHRender (models/tensorBase.py:30-34 + models/sh.py:87-112, degree 2): rgb_c = relu(sum_k Y_k(d) f[9c+k] + 0.5)
__global__ void k_sh_render(const float* __restrict__ dirs, const float* __restrict__ feat, int64_t M, float* __restrict__ rgb) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const float x = dirs[i * 3], y = dirs[i * 3 + 1], z = dirs[i * 3 + 2];
  const float xx = __fmul_rn(x, x), yy = __fmul_rn(y, y), zz = __fmul_rn(z, z);
  const float xy = __fmul_rn(x, y), yz = __fmul_rn(y, z), xz = __fmul_rn(x, z);
  float Y[9];
  Y[0] = 0.28209479177387814f;
  Y[1] = __fmul_rn(-0.4886025119029199f, y);
  Y[2] = __fmul_rn(0.4886025119029199f, z);
  Y[3] = __fmul_rn(-0.4886025119029199f, x);
  Y[4] = __fmul_rn(1.0925484305920792f, xy);
  Y[5] = __fmul_rn(-1.0925484305920792f, yz);
  Y[6] = __fmul_rn(0.31539156525252005f, __fsub_rn(__fsub_rn(__fmul_rn(2.0f, zz), xx), yy));
  Y[7] = __fmul_rn(-1.0925484305920792f, xz);
  Y[8] = __fmul_rn(0.5462742152960396f, __fsub_rn(xx, yy));
  const float* f = feat + i * 27;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) s = __fadd_rn(s, __fmul_rn(Y[k], f[9 * c + k]));
    rgb[i * 3 + c] = fmaxf(__fadd_rn(s, 0.5f), 0.f);
  }
}

// =============================================================================================
// Row H — compositing, one wave per ray      models/EgoNeRF.py:579-598
// =============================================================================================
__global__ void k_composite(const float* __restrict__ em, int em_h, const float* __restrict__ rays,
                            const float* __restrict__ z, const float* __restrict__ weight,
                            const float* __restrict__ bgw, const float* __restrict__ rgb, int64_t N, int S,
                            float* __restrict__ rgb_map, float* __restrict__ depth, float* __restrict__ bg_map,
                            float* __restrict__ env_map, float* __restrict__ rgb_raw, float shade_above) {
  const int lane = threadIdx.x & 63, j = lane & 31, half = lane >> 5;
  const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (ray >= N) return;
  // Summation order = the folded shade kernel's (ego_shade_composite, csrc/ego_shade.hip): lane j of a half adds samples j, j + 32, j + 64,
  // ... in that order (separately rounded products), then the 32 lanes of the half are added as a balanced tree.  The two forms of
  // ego_render_forward therefore return the same bits, and a batch renders identically whichever form its size selects.  Half 0 sums
  // the colours, half 1 the depth; both sum the weights.
  float acc = 0.f, cr = 0.f, cg = 0.f, cb = 0.f, dp = 0.f;
  for (int s = j; s < S; s += 32) {
    const int64_t o = ray * S + s;
    const float w = weight[o];
    acc += w;
    if (half) {
      dp += w * z[o];
    } else if (w > shade_above) {
      // colour only from samples above the threshold (tensorBase.py:482-487; 0 without one: weights are >= 0, and tiles
      // skipped by ego_shade - mask / early termination / all below the threshold - never wrote their rgb)
      cr += w * rgb[o * 3];
      cg += w * rgb[o * 3 + 1];
      cb += w * rgb[o * 3 + 2];
    }
  }
#pragma unroll
  for (int d = 1; d <= 16; d <<= 1) {
    acc += __shfl_xor(acc, d, 64); cr += __shfl_xor(cr, d, 64); cg += __shfl_xor(cg, d, 64); cb += __shfl_xor(cb, d, 64); dp += __shfl_xor(dp, d, 64);
  }
  dp = __shfl(dp, 32, 64);
  if (lane != 0) return;
  const float* R = rays + ray * 6;
  if (em) {
    float e[3];
    envmap_lookup(em, em_h, R[3], R[4], R[5], e);
    const float b = bgw[ray];
    const float bx = b * e[0], by = b * e[1], bz = b * e[2];
    cr += bx; cg += by; cb += bz;
    if (bg_map) { bg_map[ray * 3] = bx; bg_map[ray * 3 + 1] = by; bg_map[ray * 3 + 2] = bz; }
    if (env_map) { env_map[ray * 3] = e[0]; env_map[ray * 3 + 1] = e[1]; env_map[ray * 3 + 2] = e[2]; }
  }
  if (rgb_raw) { rgb_raw[ray * 3] = cr; rgb_raw[ray * 3 + 1] = cg; rgb_raw[ray * 3 + 2] = cb; }
  rgb_map[ray * 3] = fminf(fmaxf(cr, 0.f), 1.f);
  rgb_map[ray * 3 + 1] = fminf(fmaxf(cg, 0.f), 1.f);
  rgb_map[ray * 3 + 2] = fminf(fmaxf(cb, 0.f), 1.f);
  if (depth) depth[ray] = dp + (1.f - acc) * R[5];  // (1-acc) * d_z: reference quirk, EgoNeRF.py:598
}

// =============================================================================================
// update_coarse_sigma_grid — 2x average pooling of a channel-last table    models/EgoNeRF.py:124-131
// =============================================================================================
__global__ void k_avgpool(const float* __restrict__ src, int H, int W, int C, float* __restrict__ dst) {
  const int Ho = H / 2, Wo = (W == 1) ? 1 : W / 2;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)Ho * Wo * C) return;
  const int ch = (int)(idx % C);
  const int x = (int)((idx / C) % Wo);
  const int y = (int)(idx / ((int64_t)C * Wo));
  if (W == 1) {
    dst[idx] = (src[((int64_t)2 * y) * C + ch] + src[((int64_t)2 * y + 1) * C + ch]) * 0.5f;
  } else {
    const float* r0 = src + ((int64_t)(2 * y) * W + 2 * x) * C + ch;
    const float* r1 = src + ((int64_t)(2 * y + 1) * W + 2 * x) * C + ch;
    dst[idx] = (((r0[0] + r0[C]) + r1[0]) + r1[C]) * 0.25f;
  }
}

// all tables of a field in one launch (update_coarse_sigma_grid runs after every training step: 12 launches of ~5 us otherwise)
struct PoolJobs {
  const float* src[12];
  float* dst[12];
  int32_t H[12], W[12];
  int32_t C, n;
};

__global__ void k_avgpool_many(PoolJobs J) {
  const int jb = blockIdx.y;
  const int H = J.H[jb], W = J.W[jb], C = J.C;
  const int Ho = H / 2, Wo = (W == 1) ? 1 : W / 2;
  const float* __restrict__ src = J.src[jb];
  float* __restrict__ dst = J.dst[jb];
  const int64_t total = (int64_t)Ho * Wo * C;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(idx % C);
    const int x = (int)((idx / C) % Wo);
    const int y = (int)(idx / ((int64_t)C * Wo));
    if (W == 1) {
      dst[idx] = (src[((int64_t)2 * y) * C + ch] + src[((int64_t)2 * y + 1) * C + ch]) * 0.5f;
    } else {
      const float* r0 = src + ((int64_t)(2 * y) * W + 2 * x) * C + ch;
      const float* r1 = src + ((int64_t)(2 * y + 1) * W + 2 * x) * C + ch;
      dst[idx] = (((r0[0] + r0[C]) + r1[0]) + r1[C]) * 0.25f;
    }
  }
}

// =============================================================================================
// Equirectangular camera rays on the device   dataLoader/ray_utils.py:24-40 (directions), :85-113 (pose)
// =============================================================================================
struct Pose34 { float m[12]; };

__global__ void k_erp_rays(int H, int W, int row0, int n_rows, Pose34 c2w, int normalize, float* __restrict__ rays) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n_rows * W) return;
  const int col = (int)(idx % W), row = row0 + (int)(idx / W);
  erp_ray(H, W, row, col, c2w.m, normalize, rays + idx * 6);   // ego_device.h: shared with the ray-bank gather (csrc/ego_batch.hip)
}

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int ego_sample_ray_exp(const float* rays, const float* r_sched, const float* jitter, float near_, int64_t N, int32_t S,
                       float* xyz, float* z, void* stream) {
  EGO_TRACE("ego_sample_ray_exp");
  EGO_REQUIRE(rays && r_sched && N >= 0 && S >= 2, "sample_ray_exp: null input or S < 2");
  if (N == 0) return EGO_OK;
  k_sample_ray_exp<<<nblk(N * S, 256), 256, 0, (hipStream_t)stream>>>(rays, r_sched, jitter, near_, N, S, xyz, z);
  return ego_launch_status("k_sample_ray_exp");
}

int ego_erp_rays(int32_t H, int32_t W, int32_t row0, int32_t n_rows, const float* c2w, int32_t normalize, float* rays,
                 void* stream) {
  EGO_TRACE("ego_erp_rays");
  EGO_REQUIRE(H >= 1 && W >= 1 && row0 >= 0 && n_rows >= 0 && row0 + n_rows <= H, "erp_rays: bad image window");
  if (n_rows == 0) return EGO_OK;
  EGO_REQUIRE(c2w && rays, "erp_rays: null argument");
  Pose34 p;
  for (int i = 0; i < 12; ++i) p.m[i] = c2w[i];
  k_erp_rays<<<nblk((int64_t)n_rows * W, 256), 256, 0, (hipStream_t)stream>>>(H, W, row0, n_rows, p, normalize, rays);
  return ego_launch_status("k_erp_rays");
}

int ego_from_cartesian(const ego_scene* sc, const float* xyz, int64_t M, float* c7, void* stream) {
  EGO_TRACE("ego_from_cartesian");
  EGO_REQUIRE(M >= 0, "from_cartesian: M < 0");
  if (M == 0) return EGO_OK;
  EGO_REQUIRE(sc && xyz && c7, "from_cartesian: null argument");
  k_from_cartesian<<<nblk(M, 256), 256, 0, (hipStream_t)stream>>>(make_coords(*sc), xyz, M, c7);
  return ego_launch_status("k_from_cartesian");
}

int ego_normalize_coord(const ego_scene* sc, const float* c7, int64_t M, float* c7n, void* stream) {
  EGO_TRACE("ego_normalize_coord");
  EGO_REQUIRE(M >= 0, "normalize_coord: M < 0");
  if (M == 0) return EGO_OK;
  EGO_REQUIRE(sc && c7 && c7n && sc->r_lut, "normalize_coord: null argument");
  k_normalize_coord<<<nblk(M, 256), 256, 0, (hipStream_t)stream>>>(make_coords(*sc), c7, M, c7n);
  return ego_launch_status("k_normalize_coord");
}

int ego_density_feature(const ego_scene* sc, const float* c7n, int64_t M, int32_t coarse, float* out, void* stream) {
  EGO_TRACE("ego_density_feature");
  EGO_REQUIRE(M >= 0, "density_feature: M < 0");
  if (M == 0) return EGO_OK;
  EGO_REQUIRE(sc && c7n && out, "density_feature: null argument");
  const ego_vm_field& f = coarse ? sc->density_coarse : sc->density;
  if (int e = check_field(f, "density_feature")) return e;
  // one instance per component count of the any-shape envelope (multiples of 4 up to 48: what the march, the scatters and the
  // backward of this op take), the count a compile-time number so that a tap's C / 4 loads unroll
  switch (f.n_comp) {
#define EGO_DENSITY_FEATURE_CASE(C) \
    case C: k_density_feature<C><<<nblk(M, 256), 256, 0, (hipStream_t)stream>>>(make_field(f), c7n, M, out); break;
    EGO_DENSITY_FEATURE_CASE(4) EGO_DENSITY_FEATURE_CASE(8) EGO_DENSITY_FEATURE_CASE(12) EGO_DENSITY_FEATURE_CASE(16)
    EGO_DENSITY_FEATURE_CASE(20) EGO_DENSITY_FEATURE_CASE(24) EGO_DENSITY_FEATURE_CASE(28) EGO_DENSITY_FEATURE_CASE(32)
    EGO_DENSITY_FEATURE_CASE(36) EGO_DENSITY_FEATURE_CASE(40) EGO_DENSITY_FEATURE_CASE(44) EGO_DENSITY_FEATURE_CASE(48)
#undef EGO_DENSITY_FEATURE_CASE
    default: return ego_fail(EGO_E_UNSUPPORTED, "density_feature: n_comp %d (supported: multiples of 4 up to 48)", f.n_comp);
  }
  return ego_launch_status("k_density_feature");
}

int ego_feature2density(const ego_scene* sc, const float* feat, int64_t M, float* sigma, void* stream) {
  EGO_TRACE("ego_feature2density");
  EGO_REQUIRE(M >= 0, "feature2density: M < 0");
  if (M == 0) return EGO_OK;
  EGO_REQUIRE(sc && feat && sigma, "feature2density: null argument");
  k_feature2density<<<nblk(M, 256), 256, 0, (hipStream_t)stream>>>(feat, M, sc->act_softplus, sc->density_shift, sigma);
  return ego_launch_status("k_feature2density");
}

int ego_raw2alpha(const float* sigma, const float* dist, int64_t N, int32_t S, float* alpha, float* weight,
                  float* bg_weight, void* stream) {
  EGO_TRACE("ego_raw2alpha");
  EGO_REQUIRE(N >= 0 && S >= 1, "raw2alpha: bad size");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(sigma && dist, "raw2alpha: null argument");
  k_raw2alpha<<<nblk(N, 4), 256, 0, (hipStream_t)stream>>>(sigma, dist, N, S, alpha, weight, bg_weight);
  return ego_launch_status("k_raw2alpha");
}

int ego_envmap_radiance(const ego_scene* sc, const float* dirs, int64_t N, float* out, void* stream) {
  EGO_TRACE("ego_envmap_radiance");
  EGO_REQUIRE(N >= 0, "envmap_radiance: N < 0");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(sc && dirs && out && sc->envmap && sc->envmap_h >= 2, "envmap_radiance: no envmap / null argument");
  k_envmap<<<nblk(N, 256), 256, 0, (hipStream_t)stream>>>(sc->envmap, sc->envmap_h, dirs, N, out);
  return ego_launch_status("k_envmap");
}

int ego_envmap_backward(const ego_scene* sc, const float* dirs, int32_t dir_stride, const float* g_rgb, const float* rgb_raw, const float* bg_weight,
                        const float* env_map, int64_t N, float* g_emission, void* stream) {
  EGO_TRACE("ego_envmap_backward");
  EGO_REQUIRE(N >= 0, "envmap_backward: N < 0");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(sc && dirs && dir_stride >= 3 && g_rgb && rgb_raw && bg_weight && env_map && g_emission && sc->envmap_h >= 2,
              "envmap_backward: no envmap / null argument");
  k_envmap_bwd<<<nblk(N, 256), 256, 0, (hipStream_t)stream>>>(sc->envmap_h, dirs, dir_stride, g_rgb, rgb_raw, bg_weight, env_map, N, g_emission);
  return ego_launch_status("k_envmap_bwd");
}

int ego_sh_render(const float* viewdirs, const float* features, int64_t M, float* rgb, void* stream) {
  EGO_TRACE("ego_sh_render");
  EGO_REQUIRE(M >= 0, "sh_render: M < 0");
  if (M == 0) return EGO_OK;
  EGO_REQUIRE(viewdirs && features && rgb, "sh_render: null argument");
  k_sh_render<<<nblk(M, 256), 256, 0, (hipStream_t)stream>>>(viewdirs, features, M, rgb);
  return ego_launch_status("k_sh_render");
}

int ego_alpha_mask_sample(const ego_scene* sc, const float* c7n, int64_t M, float* out, void* stream) {
  EGO_TRACE("ego_alpha_mask_sample");
  EGO_REQUIRE(M >= 0, "alpha_mask_sample: M < 0");
  if (M == 0) return EGO_OK;
  EGO_REQUIRE(sc && c7n && out && sc->occ && sc->occ_res[0] >= 2 && sc->occ_res[1] >= 2 && sc->occ_res[2] >= 2,
              "alpha_mask_sample: no occupancy volume / null argument");
  k_alpha_mask_sample<<<nblk(M, 256), 256, 0, (hipStream_t)stream>>>(make_occ(*sc, 0), c7n, M, out);
  return ego_launch_status("k_alpha_mask_sample");
}

int ego_avgpool_table(const float* src, int32_t H, int32_t W, int32_t C, float* dst, void* stream) {
  EGO_TRACE("ego_avgpool_table");
  EGO_REQUIRE(src && dst && H >= 2 && W >= 1 && C >= 1, "avgpool_table: bad argument");
  const int64_t n = (int64_t)(H / 2) * (W == 1 ? 1 : W / 2) * C;
  k_avgpool<<<nblk(n, 256), 256, 0, (hipStream_t)stream>>>(src, H, W, C, dst);
  return ego_launch_status("k_avgpool");
}

int ego_avgpool_field(const ego_vm_field* src, const ego_vm_field* dst, void* stream) {
  EGO_TRACE("ego_avgpool_field");
  EGO_REQUIRE(src && dst && src->n_comp >= 1 && dst->n_comp == src->n_comp, "avgpool_field: null field or component counts differ");
  EGO_REQUIRE(vm_tables_complete(*src) && vm_tables_complete(*dst), "avgpool_field: null table");
  PoolJobs J{};
  J.C = src->n_comp; J.n = 12;
  int64_t most = 0;
  for (int g = 0; g < 2; ++g)
    for (int i = 0; i < 3; ++i) {
      // plane i: [res[y axis]][res[x axis]][C]; line i: [res[line axis]][C]
      const int px = vm_plane_x(i), py = vm_plane_y(i), la = vm_line_ax(i);
      EGO_REQUIRE(dst->res[0] == src->res[0] / 2 && dst->res[1] == src->res[1] / 2 && dst->res[2] == src->res[2] / 2 && dst->res[0] >= 1 &&
                  dst->res[1] >= 1 && dst->res[2] >= 1, "avgpool_field: dst.res must be src.res / 2");
      const int a = g * 6 + i, b = g * 6 + 3 + i;
      J.src[a] = src->plane[g][i]; J.dst[a] = (float*)dst->plane[g][i]; J.H[a] = src->res[py]; J.W[a] = src->res[px];
      J.src[b] = src->line[g][i]; J.dst[b] = (float*)dst->line[g][i]; J.H[b] = src->res[la]; J.W[b] = 1;
      const int64_t n = (int64_t)(J.H[a] / 2) * (J.W[a] / 2) * J.C;
      most = n > most ? n : most;
    }
  const unsigned bx = nblk(most, 256) < 1024u ? nblk(most, 256) : 1024u;
  k_avgpool_many<<<dim3(bx ? bx : 1u, 12), 256, 0, (hipStream_t)stream>>>(J);
  return ego_launch_status("k_avgpool_many");
}

int ego_composite(const ego_scene* sc, const float* rays, const float* z, const float* weight, const float* bg_weight,
                  const float* rgb, int64_t N, int32_t S, float* rgb_map, float* depth, float* bg_map, float* env_map,
                  float* rgb_raw, void* stream) {
  EGO_TRACE("ego_composite");
  EGO_REQUIRE(sc && rays && z && weight && rgb && rgb_map && N >= 0 && S >= 1, "composite: null argument");
  EGO_REQUIRE(!sc->envmap || bg_weight, "composite: envmap needs bg_weight");
  if (N == 0) return EGO_OK;
  k_composite<<<nblk(N, 4), 256, 0, (hipStream_t)stream>>>(sc->envmap, sc->envmap_h, rays, z, weight, bg_weight, rgb, N, S,
                                                          rgb_map, depth, bg_map, env_map, rgb_raw, fmaxf(sc->weight_thres, 0.f));
  return ego_launch_status("k_composite");
}

}  // extern "C"
