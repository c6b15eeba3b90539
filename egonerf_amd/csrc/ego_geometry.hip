// libegonerf_hip.so, ray geometry: per-ray surface normal, accumulated weight and quantile depth from the density field.
// No reference counterpart: the reference's only geometric output is the expected depth sum_s w_s z_s.
//   k_ray_geometry  g_s = grad_xyz of the density feature sum_i relu(sum_c P_c L_c) at every sample (plane_terms<true> + chart_jt, the ray
//                   gradients' own pieces: ego_vm_grad.h), n_s = -g_s / |g_s|, normal = sum_s w_s n_s, acc = sum_s w_s, and the distance of
//                   the first sample at which the running weight reaches a quantile
#include "ego_device.h"
#include "ego_host.h"
#include "ego_vm_grad.h"

namespace {

struct GeometryArgs {
  DevField dens;
  DevCoords co;
  const float* rays;     // [N][6]
  const float* z;        // [N][S]
  const float* coords;   // [N][S][4]
  const float* weight;   // [N][S]
  float* normal;         // [N][3] or null
  float* acc;            // [N] or null
  float* z_quantile;     // [N] or null
  float* grad_out;       // [N][S][3] or null
  int64_t N;
  int32_t S, Cd, normalize;
  float quantile;
};

// wave64 inclusive additive scan: wave_scan_mul's DPP steps (ego_device.h) with the identity 0
__device__ __forceinline__ float wave_scan_add(float v) {
#define EGO_SCAN_STEP(ctrl, rmask) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rmask, 0xf, false))
  EGO_SCAN_STEP(0x111, 0xf);  // row_shr:1
  EGO_SCAN_STEP(0x112, 0xf);  // row_shr:2
  EGO_SCAN_STEP(0x114, 0xf);  // row_shr:4
  EGO_SCAN_STEP(0x118, 0xf);  // row_shr:8
  EGO_SCAN_STEP(0x142, 0xa);  // row_bcast:15 -> rows 1, 3
  EGO_SCAN_STEP(0x143, 0xc);  // row_bcast:31 -> rows 2, 3
#undef EGO_SCAN_STEP
  return v;
}

// Work split: k_ray_grad's (a wave owns a ray, a 16-lane row a sample, lane = channel 16 at a time, row_sum16 over channels), behind a
// lane = sample pass over each 64 samples of the ray: their weights, distances and coordinates are read coalesced (one 64 ahead) and
// handed to the rows by cross-lane reads, the weights are scanned for the running sum (acc, the quantile) and balloted, and
// only the samples with w != 0 are dealt to the four rows, in sample order (the k-th live sample of the 64 goes to row k % 4).  A ray's
// normal is summed down each row in that order and the rows are added in row order: a fixed order that does not depend on whether the
// w == 0 samples are gathered too (grad_out: a second deal of the same 64, which adds nothing), no atomics, two calls return the same bits.
constexpr int GEO_WAVES = 4;

__global__ __launch_bounds__(64 * GEO_WAVES) void k_ray_geometry(GeometryArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, row = lane >> 4, c16 = lane & 15;
  const bool lut_lds = A.co.n_lut <= RG_LUT_LDS;
  const float* lut = lut_lds ? lds : A.co.r_lut;
  if (lut_lds)
    for (int e = tid; e < A.co.n_lut; e += 64 * GEO_WAVES) lds[e] = A.co.r_lut[e];
  __syncthreads();
  const int64_t n_units = (A.N + GEO_WAVES - 1) / GEO_WAVES;
  for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const int64_t n = unit * GEO_WAVES + wave;
    if (n >= A.N) continue;   // (no workgroup barrier below)
    const float ox = A.rays[n * 6], oy = A.rays[n * 6 + 1], oz = A.rays[n * 6 + 2];
    const float dx = A.rays[n * 6 + 3], dy = A.rays[n * 6 + 4], dz = A.rays[n * 6 + 5];
    const bool gather = A.normal || A.grad_out;
    const f32x4 no_dk[8] = {};
    float nrm[3] = {0.f, 0.f, 0.f};   // this row's part of sum_s w_s n_s
    float run = 0.f, zq = 0.f;        // the running weight in front of this 64, the quantile's distance (wave-uniform)
    bool found = false;

    // the samples base + (set bits of mask), four at a time, one per row
    auto deal = [&](uint64_t mask, int base, bool live, const float wl, const float zl, const f32x4 cl) {
      while (mask) {   // wave-uniform
        int mine = -1;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (mask) {
            const int b = __ffsll((unsigned long long)mask) - 1;
            mask &= mask - 1;
            if (row == r) mine = b;
          }
        // the sample's coordinates, distance and weight come out of the lane = sample registers: six cross-lane reads with every lane
        // active (a row without a sample reads lane 0 and drops it), not a dependent memory phase per round
        const int src = mine >= 0 ? mine : 0;
        const f32x4 cc = {__shfl(cl.x, src, 64), __shfl(cl.y, src, 64), __shfl(cl.z, src, 64), __shfl(cl.w, src, 64)};
        const float zs = __shfl(zl, src, 64), w = __shfl(wl, src, 64);
        if (mine >= 0) {
          const int64_t m = n * A.S + base + mine;
          const int g = cc.w != 0.f;
          const LinD ax[3] = {lind_setup(cc.x, A.dens.res[0]), lind_setup(cc.y, A.dens.res[1]), lind_setup(cc.z, A.dens.res[2])};
          float q[3] = {0.f, 0.f, 0.f};
#pragma unroll
          for (int i = 0; i < 3; ++i) {   // relu per plane (EgoNeRF.py:340,346)
            float qi[3] = {0.f, 0.f, 0.f};
            const float dot = row_sum16(plane_terms<true>(A.dens, A.Cd, g, i, ax, c16, nullptr, no_dk, qi));
            if (dot > 0.f) { q[0] += qi[0]; q[1] += qi[1]; q[2] += qi[2]; }
          }
          q[0] = row_sum16(q[0]); q[1] = row_sum16(q[1]); q[2] = row_sum16(q[2]);
          float gs[3];
          chart_jt(A.co, lut, g, cc.x, __fadd_rn(ox, __fmul_rn(dx, zs)), __fadd_rn(oy, __fmul_rn(dy, zs)), __fadd_rn(oz, __fmul_rn(dz, zs)), q, gs);
          if (A.grad_out && c16 < 3) A.grad_out[m * 3 + c16] = c16 == 0 ? gs[0] : (c16 == 1 ? gs[1] : gs[2]);
          if (live) {
            float u[3];
            unit3(gs, u);
#pragma unroll
            for (int j = 0; j < 3; ++j) nrm[j] = fmaf(w, -u[j], nrm[j]);
          }
        }
      }
    };

    // 64 samples, lane = sample: weight, distance and coordinates, coalesced, one 64 ahead of the 64 in work
    auto load64 = [&](int base, float& wl, float& zl, f32x4& cl) {
      const int s = base + lane;
      const int64_t m = n * A.S + (s < A.S ? s : A.S - 1);
      wl = s < A.S ? A.weight[m] : 0.f;
      zl = A.z[m];
      cl = gather ? ((const f32x4*)A.coords)[m] : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    float wl_n, zl_n;
    f32x4 cl_n;
    load64(0, wl_n, zl_n, cl_n);
    for (int base = 0; base < A.S; base += 64) {
      const bool valid = base + lane < A.S;
      const float wl = wl_n, zl = zl_n;
      const f32x4 cl = cl_n;
      if (base + 64 < A.S) load64(base + 64, wl_n, zl_n, cl_n);
      const float cum = run + wave_scan_add(wl);
      const uint64_t reached = __ballot(valid && cum >= A.quantile);
      const float z_first = __shfl(zl, reached ? __ffsll((unsigned long long)reached) - 1 : 0, 64);
      if (!found && reached) {
        found = true;
        zq = z_first;
      }
      run = __shfl(cum, 63, 64);
      if (gather) {
        const uint64_t live = __ballot(valid && wl != 0.f);
        deal(live, base, true, wl, zl, cl);
        if (A.grad_out) deal(__ballot(valid) & ~live, base, false, wl, zl, cl);
      }
    }
    // rows 0..3 in order (every lane of a row holds the row's sums)
    float tot[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
      tot[j] = ((__shfl(nrm[j], 0, 64) + __shfl(nrm[j], 16, 64)) + __shfl(nrm[j], 32, 64)) + __shfl(nrm[j], 48, 64);
    if (lane == 0) {
      if (A.normal) {
        float o[3] = {tot[0], tot[1], tot[2]};
        if (A.normalize) unit3(tot, o);
        A.normal[n * 3] = o[0]; A.normal[n * 3 + 1] = o[1]; A.normal[n * 3 + 2] = o[2];
      }
      if (A.acc) A.acc[n] = run;
      if (A.z_quantile) A.z_quantile[n] = zq;
    }
  }
}

}  // namespace

extern "C" {

int ego_ray_geometry(const ego_scene* sc, const float* rays, const float* z, const float* coords, const float* weight, int64_t N, int32_t S,
                     int32_t normalize, float quantile, float* normal, float* acc, float* z_quantile, float* grad_out, void* stream) {
  EGO_TRACE("ego_ray_geometry");
  EGO_REQUIRE(sc, "ray_geometry: null scene");
  EGO_REQUIRE(normal || acc || z_quantile || grad_out, "ray_geometry: every output is null");
  EGO_REQUIRE(N >= 0 && S >= 1, "ray_geometry: N < 0 or S < 1");
  EGO_REQUIRE(N * (int64_t)S < (1ll << 31), "ray_geometry: N S must be below 2^31");
  EGO_REQUIRE(quantile > 0.f && quantile < 1.f, "ray_geometry: quantile must lie in (0, 1)");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(rays && z && coords && weight, "ray_geometry: null argument");
  EGO_REQUIRE(((uintptr_t)coords & 15) == 0, "ray_geometry: coords must be 16-byte aligned");
  EGO_REQUIRE(sc->r_lut && sc->n_r_lut >= 2 && sc->n_r >= 1, "ray_geometry: the scene has no radius LUT");
  if (int e = check_vm_field(sc->density, "ray_geometry", "density ", true, true)) return e;
  GeometryArgs a{};
  a.dens = make_field(sc->density); a.Cd = sc->density.n_comp;
  a.co = make_coords(*sc);
  a.rays = rays; a.z = z; a.coords = coords; a.weight = weight;
  a.normal = normal; a.acc = acc; a.z_quantile = z_quantile; a.grad_out = grad_out;
  a.N = N; a.S = S; a.normalize = normalize != 0; a.quantile = quantile;
  const size_t lds_bytes = sizeof(float) * ((a.co.n_lut <= RG_LUT_LDS ? a.co.n_lut : 0) + 4);
  const int64_t units = (N + GEO_WAVES - 1) / GEO_WAVES;
  const unsigned grid = (unsigned)(units < 4096 ? units : 4096);
  k_ray_geometry<<<grid, 64 * GEO_WAVES, lds_bytes, (hipStream_t)stream>>>(a);
  return ego_launch_status("k_ray_geometry");
}

}  // extern "C"
