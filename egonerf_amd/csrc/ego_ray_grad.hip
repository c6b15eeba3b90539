// libegonerf_hip.so, ray gradients: d loss / d (origin, direction) of the training render.  No reference counterpart:
// there the coordinates are detached before grid_sample, so the positional part is zero by construction.
//   k_view_grad  d loss / d viewdir per sample through the head's first layer and the view encodings (tensorBase.py:68-75)
//   k_ray_grad   d loss / d (r^, theta^, phi^) per sample through both VM lookups (F.grid_sample's backward with respect to the grid),
//                the chart's Jacobian back to xyz, and the per-ray sums; the envmap's direction term
// lind_setup, PlaneTaps, envmap_taps and row_sum16 are ego_device.h's: the same definitions the forward lookups use; plane_terms and
// chart_jt are ego_vm_grad.h's.
#include "ego_device.h"
#include "ego_host.h"
#include "ego_generic.h"
#include "ego_vm_grad.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
// d loss / d viewdir.  x = [feat | view | sin, cos(feat pe) | sin, cos(view pe)] (tensorBase.py:68-75), dx = W1^T dh1, and
//   v_j = dx[D + j] + sum_f 2^f (cos(2^f d_j) dx[sin column] - sin(2^f d_j) dx[cos column]).
// The direction belongs to the ray, so the three vectors A_j[unit] = d x / d d_j . W1[unit] are built once per ray (LDS) and a sample
// costs three dot products with its dh1 row: workgroup = ray, thread = unit for A, then thread = sample.
struct ViewArgs {
  const float* rays;     // [N][6]
  const float* w1;       // [HID][mlp_in], the reference's layout
  const void* dh1;
  const float* dh_scale; // layout 2: [M]
  float* d_view;         // [M][3]
  int64_t N;
  int32_t S, hid, mlp_in, app_dim, fea_pe, view_pe, layout;
  uint8_t unit_of[128];  // layout 2: logical column of the scaled-fp16 dump -> hidden unit (ego_train_layout(1))
};

__global__ __launch_bounds__(256) void k_view_grad(ViewArgs A) {
  __shared__ float Aj[3][128];
  const int tid = threadIdx.x, HID = A.hid;
  const int col_view = A.app_dim, col_sin = A.app_dim + 3 + 2 * A.app_dim * A.fea_pe, col_cos = col_sin + 3 * A.view_pe;
  for (int64_t n = blockIdx.x; n < A.N; n += gridDim.x) {
    __syncthreads();   // the previous ray's samples are done with Aj
    if (tid < HID) {
      const int unit = A.layout == 2 ? A.unit_of[tid] : tid;
      const float* w = A.w1 + (int64_t)unit * A.mlp_in;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float d = A.rays[n * 6 + 3 + j];
        float a = w[col_view + j], band = 1.f;
        for (int f = 0; f < A.view_pe; ++f) {
          float s, c;
          sincos_f32(d * band, s, c);
          a += band * (c * w[col_sin + j * A.view_pe + f] - s * w[col_cos + j * A.view_pe + f]);
          band += band;
        }
        Aj[j][tid] = a;
      }
    }
    __syncthreads();
    for (int s = tid; s < A.S; s += 256) {
      const int64_t m = n * A.S + s;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
      if (A.layout == 2) {   // [tile = m / 32][k-step][lane = 32 h + m % 32][8 halves], element e = column 8 (2 ks + e / 4) + 4 h + e % 4
        const uint4* base = (const uint4*)A.dh1 + (m >> 5) * 8 * 64 + (m & 31);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const uint4 q = base[ks * 64 + 32 * h];
            const uint32_t wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const uint16_t bits = (uint16_t)(wds[e >> 1] >> (16 * (e & 1)));
              const float v = (float)__builtin_bit_cast(_Float16, bits);
              const int col = 8 * (2 * ks + (e >> 2)) + 4 * h + (e & 3);
              a0 = fmaf(v, Aj[0][col], a0); a1 = fmaf(v, Aj[1][col], a1); a2 = fmaf(v, Aj[2][col], a2);
            }
          }
        const float sc = A.dh_scale[m];
        a0 *= sc; a1 *= sc; a2 *= sc;
      } else {
        const f32x4* row = (const f32x4*)((const float*)A.dh1 + m * HID);
        for (int k = 0; k < HID / 4; ++k) {
          const f32x4 q = row[k];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a0 = fmaf(q[e], Aj[0][4 * k + e], a0); a1 = fmaf(q[e], Aj[1][4 * k + e], a1); a2 = fmaf(q[e], Aj[2][4 * k + e], a2);
          }
        }
      }
      A.d_view[m * 3] = a0; A.d_view[m * 3 + 1] = a1; A.d_view[m * 3 + 2] = a2;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct RayGradArgs {
  DevField dens, app;
  DevCoords co;
  const float* basis[2];   // [app_dim][3 C_app] per grid (nn.Linear.weight)
  const float* rays;       // [N][6]
  const float* z;          // [N][S]
  const float* coords;     // [N][S][4]
  const float* dfeat;      // [M] or null
  const float* dfe;        // [M][ldfe] or null
  const float* d_view;     // [M][3] or null
  const float* g_rgb;      // envmap term: all four or none
  const float* rgb_raw;
  const float* bg_weight;
  const float* env_map;
  const float* envmap;     // emission [3][2h][h]
  float* d_xyz;            // [M][3] or null
  float* g_rays;           // [N][6]
  int64_t N;
  int32_t S, Cd, Ca, app_dim, ldfe, envmap_h;
  int8_t slot_of[32];      // ldfe == 32: dfe column -> feature (-1: padding; ego_train_layout(2))
};

// plane_terms (with BT_LD, the leading dimension of the basis columns in LDS), chart_jt and RG_LUT_LDS: ego_vm_grad.h, shared with
// csrc/ego_geometry.hip

// d (bg_weight sigmoid(bilinear(emission, (u, v))))/d direction through F.normalize, u = (n_z + 1) / 2, v = (atan2(n_y, n_x) + pi) / 2 pi
__device__ __forceinline__ void envmap_dir_grad(const RayGradArgs& A, int64_t n, float out[3]) {
  out[0] = out[1] = out[2] = 0.f;
  const int h = A.envmap_h;
  const float dx = A.rays[n * 6 + 3], dy = A.rays[n * 6 + 4], dz = A.rays[n * 6 + 5];
  const EnvTaps t = envmap_taps(dx, dy, dz, h);
  const float nx = t.nx, ny = t.ny, nz = t.nz, nrm = t.nrm;
  const LinD &X = t.X, &Y = t.Y;
  const float b = A.bg_weight[n];
  float gx = 0.f, gy = 0.f;   // d / d (x^, y^) of the lookup
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float raw = A.rgb_raw[n * 3 + ch];
    const float g = (raw >= 0.f && raw <= 1.f) ? A.g_rgb[n * 3 + ch] : 0.f;   // clamp(0, 1) backward, as ego_envmap_backward
    const float e = A.env_map[n * 3 + ch];
    const float ge = g * b * e * (1.f - e);
    const float* E = A.envmap + (int64_t)ch * 2 * h * h;
    const float e00 = E[(int64_t)Y.i0 * h + X.i0], e01 = E[(int64_t)Y.i0 * h + X.i1], e10 = E[(int64_t)Y.i1 * h + X.i0],
                e11 = E[(int64_t)Y.i1 * h + X.i1];
    gx += ge * ((e00 * X.d0 + e01 * X.d1) * Y.w0 + (e10 * X.d0 + e11 * X.d1) * Y.w1);
    gy += ge * ((e00 * X.w0 + e01 * X.w1) * Y.d0 + (e10 * X.w0 + e11 * X.w1) * Y.d1);
  }
  // x^ = n_z; y^ = atan2(n_y, n_x) / pi
  const float rho2 = nx * nx + ny * ny;
  const float k = rho2 > 0.f ? gy / (3.14159265358979323846f * rho2) : 0.f;
  const float Gx = -k * ny, Gy = k * nx, Gz = gx;
  const float nG = nx * Gx + ny * Gy + nz * Gz;
  const float ox = (Gx - nx * nG) / nrm, oy = (Gy - ny * nG) / nrm, oz = (Gz - nz * nG) / nrm;
  if (fabsf(ox) < INFINITY && fabsf(oy) < INFINITY && fabsf(oz) < INFINITY) { out[0] = ox; out[1] = oy; out[2] = oz; }
}

// Work split: a wave owns a ray, its four 16-lane rows take the ray's samples s = row, row + 4, ...; inside a row lane = channel, 16
// at a time, so a tap is one 64-byte read per row (three in a row for 48 channels: the 192-byte tap).  The per-sample sums over channels are
// row reductions on the DPP path; the per-ray sums run down each row in sample order and the four rows are added in row order at the end.
// No atomics, no order that depends on the machine: two calls return the same bits.  LDS: both basis matrices, transposed (a channel's
// column contiguous, in the column order of dfe) - g_v costs a lane eight 16-byte reads and 32 multiply-adds per channel.
constexpr int RG_WAVES = 4;     // 190 VGPRs, two waves per SIMD: two 4-wave workgroups share a CU (one 8-wave workgroup would fill it alone)

__global__ __launch_bounds__(64 * RG_WAVES) void k_ray_grad(RayGradArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, row = lane >> 4, c16 = lane & 15;
  const int D = A.app_dim, ncol = 3 * A.Ca;
  float* basis_l = lds;                                   // [2][3 Ca][BT_LD]: slot t of column c = basis[feature of dfe column t][c], 0 for padding
  float* lut_l = lds + (A.dfe ? 2 * ncol * BT_LD : 0);    // the radius LUT, when it is small enough
  const bool lut_lds = A.co.n_lut <= RG_LUT_LDS;
  const float* lut = lut_lds ? lut_l : A.co.r_lut;
  if (lut_lds)
    for (int e = tid; e < A.co.n_lut; e += 64 * RG_WAVES) lut_l[e] = A.co.r_lut[e];
  if (!A.dfe) __syncthreads();
  if (A.dfe) {
    for (int e = tid; e < 2 * ncol * 32; e += 64 * RG_WAVES) {
      const int t = e & 31, gc = e >> 5, g = gc >= ncol, col = gc - g * ncol;
      const int k = A.ldfe == 32 ? A.slot_of[t] : (t < D ? t : -1);
      basis_l[gc * BT_LD + t] = k >= 0 ? A.basis[g][k * ncol + col] : 0.f;
    }
    __syncthreads();
  }
  const int64_t n_units = (A.N + RG_WAVES - 1) / RG_WAVES;
  for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const int64_t n = unit * RG_WAVES + wave;
    if (n >= A.N) continue;   // (no workgroup barrier below)
    const float ox = A.rays[n * 6], oy = A.rays[n * 6 + 1], oz = A.rays[n * 6 + 2];
    const float dx = A.rays[n * 6 + 3], dy = A.rays[n * 6 + 4], dz = A.rays[n * 6 + 5];
    float go[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f};
    const f32x4 no_dk[8] = {};
    const bool same_res = !A.dfeat || (A.dens.res[0] == A.app.res[0] && A.dens.res[1] == A.app.res[1] && A.dens.res[2] == A.app.res[2]);
    // a sample's coordinates, distance and density gradient are fetched one round ahead: one dependent memory phase less per sample
    auto fetch = [&](int s, f32x4& cc, float& zs, float& df) {
      const int64_t m = n * A.S + (s < A.S ? s : A.S - 1);
      cc = ((const f32x4*)A.coords)[m];
      zs = A.z[m];
      df = A.dfeat ? A.dfeat[m] : 0.f;
    };
    f32x4 cc_n;
    float zs_n, df_n;
    fetch(row, cc_n, zs_n, df_n);
    for (int s = row; s < A.S; s += 4) {
      const int64_t m = n * A.S + s;
      const f32x4 cc = cc_n;
      const float zs = zs_n, df = df_n;
      fetch(s + 4, cc_n, zs_n, df_n);
      const int g = cc.w != 0.f;
      float q[3] = {0.f, 0.f, 0.f};
      // one tap set-up for both fields where they have one resolution (every shipped config)
      const DevField& F0 = A.dfeat ? A.dens : A.app;
      LinD ax[3] = {lind_setup(cc.x, F0.res[0]), lind_setup(cc.y, F0.res[1]), lind_setup(cc.z, F0.res[2])};
      if (df != 0.f) {   // density: relu per plane (EgoNeRF.py:340,346) - dfeat carries no mask
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          float qi[3] = {0.f, 0.f, 0.f};
          const float dot = row_sum16(plane_terms<true>(A.dens, A.Cd, g, i, ax, c16, nullptr, no_dk, qi));
          if (dot > 0.f) { q[0] = fmaf(df, qi[0], q[0]); q[1] = fmaf(df, qi[1], q[1]); q[2] = fmaf(df, qi[2], q[2]); }
        }
      }
      if (A.dfe) {
        // the sample's 32 feature-slot gradients (its own grid's half of dfe64): the row's lanes read the same 128 bytes
        const f32x4* dr = (const f32x4*)(A.dfe + m * A.ldfe + (A.ldfe == 64 ? 32 * g : 0));
        f32x4 dk[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) dk[j] = dr[j];
        if (!same_res) { ax[0] = lind_setup(cc.x, A.app.res[0]); ax[1] = lind_setup(cc.y, A.app.res[1]); ax[2] = lind_setup(cc.z, A.app.res[2]); }
        const float* bg = basis_l + g * ncol * BT_LD;
#pragma unroll
        for (int i = 0; i < 3; ++i) plane_terms<false>(A.app, A.Ca, g, i, ax, c16, bg, dk, q);
      }
      q[0] = row_sum16(q[0]); q[1] = row_sum16(q[1]); q[2] = row_sum16(q[2]);
      float dxyz[3];
      chart_jt(A.co, lut, g, cc.x, __fadd_rn(ox, __fmul_rn(dx, zs)), __fadd_rn(oy, __fmul_rn(dy, zs)), __fadd_rn(oz, __fmul_rn(dz, zs)), q, dxyz);
      if (A.d_xyz && c16 < 3) A.d_xyz[m * 3 + c16] = c16 == 0 ? dxyz[0] : (c16 == 1 ? dxyz[1] : dxyz[2]);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        go[j] += dxyz[j];
        gd[j] = fmaf(zs, dxyz[j], gd[j]);
        if (A.d_view) gd[j] += A.d_view[m * 3 + j];
      }
    }
    // rows 0..3 in order (every lane of a row holds the row's sums)
    float tot[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const float v = j < 3 ? go[j] : gd[j - 3];
      tot[j] = ((__shfl(v, 0, 64) + __shfl(v, 16, 64)) + __shfl(v, 32, 64)) + __shfl(v, 48, 64);
    }
    if (lane == 0) {
      if (A.envmap) {
        float e[3];
        envmap_dir_grad(A, n, e);
        tot[3] += e[0]; tot[4] += e[1]; tot[5] += e[2];
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) A.g_rays[n * 6 + j] = tot[j];
    }
  }
}

}  // namespace

extern "C" {

int ego_view_grad(const ego_scene* sc, const float* rays, int32_t S, int64_t M, const void* dh1, int32_t dh_layout, const float* dh_scale,
                  float* d_view, void* stream) {
  EGO_TRACE("ego_view_grad");
  EGO_REQUIRE(sc && S >= 1 && M >= 0 && M % S == 0 && M < (1ll << 31), "view_grad: null scene or bad size");
  if (M == 0) return EGO_OK;
  EGO_REQUIRE(rays && dh1 && d_view, "view_grad: null argument");
  EGO_REQUIRE(sc->head == EGO_HEAD_MLP_FEA && sc->mlp_w[0], "view_grad: the head has no network (RGB head: the view gradient is zero)");
  EGO_REQUIRE(dh_layout == 0 || dh_layout == 2, "view_grad: dh_layout must be 0 (row-major fp32) or 2 (ego_shade_backward's scaled fp16)");
  if (int e = check_head_shape(sc, "view_grad", EGO_E_BADARG)) return e;
  EGO_REQUIRE(dh_layout == 0 || (sc->mlp_hidden == 128 && dh_scale && ((uintptr_t)dh1 & 15) == 0),
              "view_grad: layout 2 needs 128 hidden units, dh_scale and a 16-byte aligned dh1");
  EGO_REQUIRE(dh_layout == 2 || ((uintptr_t)dh1 & 15) == 0, "view_grad: dh1 must be 16-byte aligned");
  ViewArgs a{};
  a.rays = rays; a.w1 = sc->mlp_w[0]; a.dh1 = dh1; a.dh_scale = dh_scale; a.d_view = d_view; a.N = M / S; a.S = S;
  a.hid = sc->mlp_hidden; a.mlp_in = sc->mlp_in; a.app_dim = sc->app_dim; a.fea_pe = sc->fea_pe; a.view_pe = sc->view_pe; a.layout = dh_layout;
  if (dh_layout == 2) {
    int32_t unit[128];
    if (int e = ego_train_layout(1, unit, 128)) return e;
    for (int c = 0; c < 128; ++c) a.unit_of[c] = (uint8_t)unit[c];
  }
  const unsigned grid = (unsigned)(a.N < 8192 ? a.N : 8192);
  k_view_grad<<<grid, 256, 0, (hipStream_t)stream>>>(a);
  return ego_launch_status("k_view_grad");
}

int ego_ray_grad(const ego_scene* sc, const float* rays, const float* z, const float* coords, const float* dfeat, const float* dfe, int32_t ldfe,
                 const float* d_view, const float* g_rgb, const float* rgb_raw, const float* bg_weight, const float* env_map, int64_t N, int32_t S,
                 int32_t fine_pass, float* d_xyz, float* g_rays, void* stream) {
  EGO_TRACE("ego_ray_grad");
  EGO_REQUIRE(sc && N >= 0 && S >= 1 && N * (int64_t)S < (1ll << 31), "ray_grad: null scene or bad size");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(rays && z && coords && g_rays, "ray_grad: null argument");
  EGO_REQUIRE(((uintptr_t)coords & 15) == 0, "ray_grad: coords must be 16-byte aligned");
  EGO_REQUIRE(sc->r_lut && sc->n_r_lut >= 2 && sc->n_r >= 1, "ray_grad: the scene has no radius LUT");
  const int envs = (g_rgb != nullptr) + (rgb_raw != nullptr) + (bg_weight != nullptr) + (env_map != nullptr);
  EGO_REQUIRE(envs == 0 || (envs == 4 && sc->envmap && sc->envmap_h >= 2), "ray_grad: the four envmap arguments come together, with a scene that has an envmap");
  RayGradArgs a{};
  if (dfeat) {
    if (int e = check_vm_field(sc->density, "ray_grad", "density ", true, true)) return e;
    a.dens = make_field(sc->density); a.Cd = sc->density.n_comp;
  }
  if (dfe) {
    if (int e = check_vm_field(sc->app, "ray_grad", "appearance ", true, true)) return e;
    EGO_REQUIRE(sc->basis[0] && sc->basis[1] && sc->app_dim >= 1 && sc->app_dim <= 32, "ray_grad: basis matrices missing or app_dim > 32");
    EGO_REQUIRE(ldfe == 32 || ldfe == 64, "ray_grad: ldfe must be 32 (ego_shade_backward's dfe) or 64 (ego_shade_backward_generic's dfe64)");
    EGO_REQUIRE(((uintptr_t)dfe & 15) == 0, "ray_grad: dfe must be 16-byte aligned");
    a.app = make_field(sc->app); a.Ca = sc->app.n_comp;
    if (ldfe == 32) {
      int32_t slot[32];
      if (int e = ego_train_layout(2, slot, 32)) return e;
      for (int c = 0; c < 32; ++c) a.slot_of[c] = (int8_t)(slot[c] < sc->app_dim ? slot[c] : -1);
    }
  }
  a.co = make_coords(*sc, fine_pass != 0);
  a.basis[0] = sc->basis[0]; a.basis[1] = sc->basis[1];
  a.rays = rays; a.z = z; a.coords = coords; a.dfeat = dfeat; a.dfe = dfe; a.d_view = d_view;
  a.g_rgb = g_rgb; a.rgb_raw = rgb_raw; a.bg_weight = bg_weight; a.env_map = env_map; a.envmap = envs ? sc->envmap : nullptr;
  a.d_xyz = d_xyz; a.g_rays = g_rays; a.N = N; a.S = S; a.app_dim = sc->app_dim; a.ldfe = ldfe; a.envmap_h = sc->envmap_h;
  const size_t lds_bytes = sizeof(float) * ((dfe ? (size_t)2 * 3 * a.Ca * BT_LD : 0) + (a.co.n_lut <= RG_LUT_LDS ? a.co.n_lut : 0) + 4);
  const int64_t units = (N + RG_WAVES - 1) / RG_WAVES;
  const unsigned grid = (unsigned)(units < 4096 ? units : 4096);
  k_ray_grad<<<grid, 64 * RG_WAVES, lds_bytes, (hipStream_t)stream>>>(a);
  return ego_launch_status("k_ray_grad");
}

}  // extern "C"
