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

extern "C" {

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
