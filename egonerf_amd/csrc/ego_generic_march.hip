// libegonerf_hip.so, part 7 (ego_generic.hip): the density march for component counts other than the shipped 16.
#include "ego_device.h"
#include "ego_host.h"
#include "ego_generic.h"
#include "ego_generic_dev.h"

namespace {

// ---- generic march: the round-2 structure without teams (lane = sample gathers its own taps), any C % 4 == 0 -----------------
struct GenMarchArgs {
  DevCoords c;
  DevField F;
  const float* rays; const float* z_in; const float* r_sched; const float* jitter;
  float* z_out; float* alpha; float* weight; float* bg; float* coords_out; float* sigma_out; uint8_t* tile_active;
  DevOcc occ;   // cell = nullptr: the exact trilinear test (occ_sample)
  int64_t N;
  int32_t S, C, alpha_stride, softplus;
  float near_, shift, dscale, term_eps, shade_above;
};

__global__ __launch_bounds__(256) void k_march_generic(GenMarchArgs A) {
  __shared__ float lut[1024];
  for (int i = threadIdx.x; i < A.c.n_lut; i += blockDim.x) lut[i] = A.c.r_lut[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= A.N) return;
  const float* R = A.rays + ray * 6;
  const float ox = R[0], oy = R[1], oz = R[2], dx = R[3], dy = R[4], dz = R[5];
  const int S = A.S, C = A.C;
  float carry = 1.f;
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int s = min(s0 + lane, S - 1);
    const bool ok = (s0 + lane) < S;
    const int sn = (s < S - 1) ? s + 1 : s - 1;
    float z, zn;
    if (A.z_in) { z = A.z_in[ray * S + s]; zn = A.z_in[ray * S + sn]; }
    else {
      // sched_z (ego_device.h) spelled out: inlined from there (its parameters are __restrict__, which k_march_density relies on) this
      // kernel's tap loads are scheduled one wait per load instead of six in flight: 4096 x 512, 8 components, 0.086 -> 0.121 ms
      const auto zz = [&](int k) {
        float r = A.r_sched[k];
        if (A.jitter) {
          const float step = (k < S - 1) ? __fsub_rn(A.r_sched[k + 1], r) : __fsub_rn(r, A.r_sched[S - 2]);
          r = __fadd_rn(r, __fmul_rn(step, A.jitter[ray * S + k]));
        }
        return __fadd_rn(A.near_, r);
      };
      z = zz(s); zn = zz(sn);
    }
    const float dist = (s < S - 1) ? __fsub_rn(zn, z) : __fsub_rn(z, zn);
    const float px = __fadd_rn(ox, __fmul_rn(dx, z)), py = __fadd_rn(oy, __fmul_rn(dy, z)), pz = __fadd_rn(oz, __fmul_rn(dz, z));
    const YinYang y = yinyang_from_xyz(px, py, pz, A.c);
    const float a_r = normalize_r(y.r, lut, A.c.n_lut, A.c.n_r);
    const float a_th = normalize_ang(y.th, A.c.th_near, A.c.th_inv);
    const float a_ph = normalize_ang(y.ph, A.c.ph_near, A.c.ph_inv);
    const bool occupied = !A.occ.vol || occ_sample(A.occ, y.yang, a_r, a_th, a_ph) > 0.f;
    float sg = 0.f;
    if (occupied) {
#pragma clang fp contract(fast)
      // density_lookup (csrc/ego_stages.hip) with C at run time; spelled out: called as one shared body this kernel's tap loads are
      // scheduled differently (125 VGPRs and 35 spilled SGPRs where this form has 145 and 4), as with sched_z above
      const VMTaps t = vm_setup(a_r, a_th, a_ph, A.F.res);
      const int g = y.yang;
      float feat = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const PlaneTaps T = EGO_PLANE_TAPS_OF(A.F, C, g, i, t.ax);
        float dot = 0.f;
        for (int c4 = 0; c4 < C; c4 += 4) {
          const f32x4 pv = tap4(T.p00, c4) * T.w00 + tap4(T.p01, c4) * T.w01 + tap4(T.p10, c4) * T.w10 + tap4(T.p11, c4) * T.w11;
          const f32x4 lv = tap4(T.l0, c4) * T.wl0 + tap4(T.l1, c4) * T.wl1;
          const f32x4 mm = pv * lv;
          dot += (mm.x + mm.y) + (mm.z + mm.w);
        }
        feat += fmaxf(dot, 0.f);
      }
      sg = A.softplus ? softplus_shift(feat, A.shift) : fmaxf(feat, 0.f);
    }
    const float a = ok ? alpha_from(sg * __fmul_rn(dist, A.dscale)) : 0.f;
    const float tt = ok ? __fadd_rn(__fsub_rn(1.f, a), 1e-10f) : 1.f;
    const float inc = wave_scan_mul(tt, lane);
    float exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = 1.f;
    const float T = carry * exc;
    const float wgt = (A.term_eps > 0.f && T < A.term_eps) ? 0.f : a * T;
    if (A.tile_active) {
      const unsigned long long nz = __ballot(ok && wgt > A.shade_above);
      const int64_t o = ray * S + s;
      if ((S & 31) == 0) {
        if (ok && (lane & 31) == 0) A.tile_active[o >> 5] = (nz >> (lane & 32) & 0xffffffffull) != 0ull ? 1 : 0;
      } else if (ok && (nz >> (lane & 32) & 0xffffffffull) != 0ull && ((lane & 31) == 0 || (o & 31) == 0)) {
        A.tile_active[o >> 5] = 1;
      }
    }
    if (ok) {
      const int64_t o = ray * S + s;
      if (A.z_out) A.z_out[o] = z;
      if (A.coords_out) ((f32x4*)A.coords_out)[o] = f32x4{a_r, a_th, a_ph, y.yang ? 1.f : 0.f};
      if (A.sigma_out) A.sigma_out[o] = sg;
      if (A.alpha) A.alpha[ray * A.alpha_stride + s] = a;
      if (A.weight) A.weight[o] = wgt;
    }
    carry *= __shfl(inc, 63, 64);
  }
  if (A.alpha && lane < A.alpha_stride - S) A.alpha[ray * A.alpha_stride + S + lane] = 1.f;
  if (A.bg && lane == 0) A.bg[ray] = carry;
}

}  // namespace

int ego_generic_march(const ego_scene* sc, const ego_vm_field& f, bool fine_lut, const float* rays, int64_t N, int32_t S, const float* z_in,
                      const float* r_sched, const float* jitter, float near_, const uint8_t* occ, float* z_out, float* alpha, int32_t alpha_stride,
                      float* weight, float* bg_weight, float* coords_out, float* sigma_out, uint8_t* tile_active, void* stream) {
  const int C = f.n_comp;
  if (int e = check_generic_n_comp(C, "march_density")) return e;
  GenMarchArgs a{};
  a.c = make_coords(*sc, fine_lut); a.F = make_field(f);
  a.rays = rays; a.z_in = z_in; a.r_sched = r_sched; a.jitter = jitter; a.z_out = z_out; a.alpha = alpha; a.weight = weight; a.bg = bg_weight;
  a.coords_out = coords_out; a.sigma_out = sigma_out; a.tile_active = tile_active; a.occ.vol = occ;
  a.occ.res[0] = sc->occ_res[0]; a.occ.res[1] = sc->occ_res[1]; a.occ.res[2] = sc->occ_res[2];
  a.N = N; a.S = S; a.C = C; a.alpha_stride = alpha_stride; a.softplus = sc->act_softplus;
  a.near_ = near_; a.shift = sc->density_shift; a.dscale = sc->distance_scale; a.term_eps = sc->term_eps; a.shade_above = fmaxf(sc->weight_thres, 0.f);
  k_march_generic<<<(unsigned)((N + 3) / 4), 256, 0, (hipStream_t)stream>>>(a);
  return ego_launch_status("k_march_generic");
}
