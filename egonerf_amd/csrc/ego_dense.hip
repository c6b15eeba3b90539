// libegonerf_hip.so: the baked node grid of a 16-component density field (ego_scene.density_dense / density_coarse_dense), read by the
// dense form of the density march (csrc/ego_march.hip, k_march_density with DENSE).  gfx950 only.
//
// Per lookup i of a grid the factored density feature is dot_i(x) = sum_c bilerp(plane_i,c)(x_a, x_b) * lerp(line_i,c)(x_c)
// (EgoNeRF.py:291-347).  Plane and line interpolate on the same lattice along independent axes, so dot_i is the trilinear
// interpolation of G_i[phi][theta][r] = sum_c plane_i,c[node] * line_i,c[node], zero padding included (an out-of-range tap has weight
// 0 in either form).  The ReLU sits outside the interpolation, per lookup: three grids, interleaved as (G_0, G_1, G_2, 0) so that one
// cell corner is one 16-byte load.  The 16-channel products are then paid once per table version instead of once per sample.
#include "ego_device.h"
#include "ego_host.h"

// One thread per voxel of [grid][N_phi][N_theta][N_r].  Six 64-byte rows per voxel (three plane texels, three line texels), each read as
// four float4; the sum over the 16 channels is ONE chain of fused multiply-adds in ascending channel order, starting from 0.
__global__ __launch_bounds__(256) void k_bake_density_dense(DevField F, f32x4* __restrict__ out, int64_t n_grid) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= 2 * n_grid) return;
  const int g = v >= n_grid ? 1 : 0;
  int64_t rem = v - (int64_t)g * n_grid;
  int idx[3];   // per axis: 0 r, 1 theta, 2 phi
  idx[0] = (int)(rem % F.res[0]); rem /= F.res[0];
  idx[1] = (int)(rem % F.res[1]);
  idx[2] = (int)(rem / F.res[1]);
  float G[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int64_t po = ((int64_t)idx[VM_PLANE_Y(i)] * F.res[VM_PLANE_X(i)] + idx[VM_PLANE_X(i)]) * 16;
    const int64_t lo = (int64_t)idx[VM_LINE_AX(i)] * 16;
    const float* P = (g ? F.plane[1][i] : F.plane[0][i]) + po;
    const float* L = (g ? F.line[1][i] : F.line[0][i]) + lo;
    float acc = 0.f;
#pragma unroll
    for (int c4 = 0; c4 < 16; c4 += 4) {
      const f32x4 p = tap4(P, c4), l = tap4(L, c4);
      acc = __fmaf_rn(p.x, l.x, acc);
      acc = __fmaf_rn(p.y, l.y, acc);
      acc = __fmaf_rn(p.z, l.z, acc);
      acc = __fmaf_rn(p.w, l.w, acc);
    }
    G[i] = acc;
  }
  out[v] = f32x4{G[0], G[1], G[2], 0.f};
}

// ---- the baked node grid of the appearance features (ego_scene.app_f16 = EGO_APP_DENSE), read by the dense gather of k_shade_h (csrc/ego_shade.hip) ----
// The 27 features of a grid are basis . concat_i(bilerp(plane_i) * lerp(line_i)): the same identity one linear map further, so they are
// the trilinear interpolation of F[g][phi][theta][r][27] = basis_g . concat_i(plane_i[node] * line_i[node]).  A node is 128 bytes, eight
// quads of four floats: quad 2 q + h holds slots 4 q .. 4 q + 3 of lane half h, slot s of half h is feature 2 s + h (the fe registers of
// ego_tuned.h); slots without a feature (s >= 14, and s = 13 of half 1) are 0.  The halves interleave by quad so that the two lanes of
// a sample read the same 64-byte line in every load instruction (app_channel's reason).
constexpr int APPD_K = 144, APPD_F = 27, APPD_FP = 28;   // products per node, features, padded row of the LDS basis
__host__ __device__ constexpr int app_dense_float(int f) { return (2 * ((f >> 1) >> 2) + (f & 1)) * 4 + ((f >> 1) & 3); }   // feature -> float of the node

// One thread per node of one grid (blockIdx.y).  The basis goes to LDS as float64, [k][28]; the thread walks the 144 channels in the
// basis' column order (plane-major, k = 48 i + c): the product plane * line is exact in float64 (24 x 24 significant bits), and every
// feature is ONE chain acc = fma(basis[f][k], product_k, acc) in float64 from 0, rounded to float32 once at the end.
__global__ __launch_bounds__(256) void k_bake_app_dense(DevField F, const float* __restrict__ basis0, const float* __restrict__ basis1,
                                                        f32x4* __restrict__ out, int64_t n_grid) {
  __shared__ double B[APPD_K * APPD_FP];
  const int g = blockIdx.y;
  const float* basis = g ? basis1 : basis0;   // [27][144] row-major (nn.Linear(144, 27).weight)
  for (int e = threadIdx.x; e < APPD_K * APPD_FP; e += 256) {
    const int k = e / APPD_FP, f = e % APPD_FP;
    B[e] = f < APPD_F ? (double)basis[f * APPD_K + k] : 0.0;
  }
  __syncthreads();
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n_grid) return;
  int64_t rem = v;
  int idx[3];   // per axis: 0 r, 1 theta, 2 phi
  idx[0] = (int)(rem % F.res[0]); rem /= F.res[0];
  idx[1] = (int)(rem % F.res[1]);
  idx[2] = (int)(rem / F.res[1]);
  double acc[APPD_FP];
#pragma unroll
  for (int f = 0; f < APPD_FP; ++f) acc[f] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int64_t po = ((int64_t)idx[VM_PLANE_Y(i)] * F.res[VM_PLANE_X(i)] + idx[VM_PLANE_X(i)]) * 48;
    const int64_t lo = (int64_t)idx[VM_LINE_AX(i)] * 48;
    const float* P = (g ? F.plane[1][i] : F.plane[0][i]) + po;
    const float* L = (g ? F.line[1][i] : F.line[0][i]) + lo;
    for (int c4 = 0; c4 < 48; c4 += 4) {
      const f32x4 p = tap4(P, c4), l = tap4(L, c4);
      const double pr[4] = {(double)p.x * (double)l.x, (double)p.y * (double)l.y, (double)p.z * (double)l.z, (double)p.w * (double)l.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double* row = B + (i * 48 + c4 + e) * APPD_FP;
#pragma unroll
        for (int f = 0; f < APPD_FP; ++f) acc[f] = __fma_rn(row[f], pr[e], acc[f]);
      }
    }
  }
  float node[32];
#pragma unroll
  for (int s = 0; s < 32; ++s) node[s] = 0.f;
#pragma unroll
  for (int f = 0; f < APPD_F; ++f) node[app_dense_float(f)] = (float)acc[f];
  f32x4* o = out + ((int64_t)g * n_grid + v) * 8;
#pragma unroll
  for (int q = 0; q < 8; ++q) o[q] = f32x4{node[4 * q], node[4 * q + 1], node[4 * q + 2], node[4 * q + 3]};
}

extern "C" {

int ego_bake_app_dense(const ego_vm_field* f, const float* basis_yin, const float* basis_yang, int32_t app_dim, float* out, void* stream) {
  EGO_TRACE("ego_bake_app_dense");
  EGO_REQUIRE(f && basis_yin && basis_yang && out, "bake_app_dense: null argument");
  if (f->n_comp != 48) return ego_fail(EGO_E_UNSUPPORTED, "bake_app_dense: n_comp %d (the dense gather is the 48-component one)", f->n_comp);
  if (app_dim != APPD_F) return ego_fail(EGO_E_UNSUPPORTED, "bake_app_dense: app_dim %d (supported: 27)", app_dim);
  const int64_t n_grid = (int64_t)f->res[0] * f->res[1] * f->res[2];
  EGO_REQUIRE(f->res[0] >= 2 && f->res[1] >= 2 && f->res[2] >= 2, "bake_app_dense: resolution < 2");
  EGO_REQUIRE(2 * n_grid * 128 < ((int64_t)1 << 32), "bake_app_dense: the grid must stay under 4 GB (the gather addresses it with 32-bit byte offsets)");
  EGO_REQUIRE(((uintptr_t)out & 15) == 0, "bake_app_dense: out must be 16-byte aligned");
  if (int e = check_field(*f, "bake_app_dense")) return e;
  k_bake_app_dense<<<dim3(nblk(n_grid, 256), 2), 256, 0, (hipStream_t)stream>>>(make_field(*f), basis_yin, basis_yang, (f32x4*)out, n_grid);
  return ego_launch_status("k_bake_app_dense");
}

int ego_bake_density_dense(const ego_vm_field* f, float* out, void* stream) {
  EGO_TRACE("ego_bake_density_dense");
  EGO_REQUIRE(f && out, "bake_density_dense: null argument");
  if (int e = check_field(*f, "bake_density_dense")) return e;
  if (f->n_comp != 16) return ego_fail(EGO_E_UNSUPPORTED, "bake_density_dense: n_comp %d (the dense march is the 16-component one)", f->n_comp);
  EGO_REQUIRE(((uintptr_t)out & 15) == 0, "bake_density_dense: out must be 16-byte aligned");
  const int64_t n_grid = (int64_t)f->res[0] * f->res[1] * f->res[2];
  EGO_REQUIRE(2 * n_grid * 16 < ((int64_t)1 << 32), "bake_density_dense: the grid must stay under 4 GB (the march addresses it with 32-bit byte offsets)");
  k_bake_density_dense<<<nblk(2 * n_grid, 256), 256, 0, (hipStream_t)stream>>>(make_field(*f), (f32x4*)out, n_grid);
  return ego_launch_status("k_bake_density_dense");
}

}  // extern "C"
