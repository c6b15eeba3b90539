// libegonerf_hip.so, part 7 (ego_generic.hip): the density march for component counts other than the shipped 16.
#include "ego_device.h"
#include "ego_host.h"
#include "ego_generic.h"
#include "ego_march.h"

namespace {

// ---- generic march: the round-2 structure without teams (lane = sample gathers its own taps), any C % 4 == 0.  Phase A, the
// transmittance step and the trailing stores are the text it shares with k_march_density (ego_march.h, ego_device.h); three pieces keep
// their own text here, each with what sharing it measured ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_march_generic(MarchArgs A) {
  __shared__ float lut[1024];
  for (int i = threadIdx.x; i < A.c.n_lut; i += blockDim.x) lut[i] = A.c.r_lut[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= A.N) return;
  const MarchRay R = march_ray(A.rays, ray);
  const int S = A.S, C = A.C;
  float carry = 1.f;
  for (int s0 = 0; s0 < S; s0 += 64) {
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
    MarchSample m = march_distances(A.z_in, ray, s0, lane, S, zz);
    march_coords(m, A.c, R, [&](float r) { return normalize_r(r, lut, A.c.n_lut, A.c.n_r); });
    const bool occupied = !A.occ.vol || occ_sample(A.occ, m.yang, m.a_r, m.a_th, m.a_ph) > 0.f;
    float sg = 0.f;
    if (occupied) {
#pragma clang fp contract(fast)
      // density_lookup (csrc/ego_stages.hip) with C at run time; spelled out: called as one shared body this kernel's tap loads are
      // scheduled differently (125 VGPRs and 35 spilled SGPRs where this form has 145 and 4), as with sched_z above
      const VMTaps t = vm_setup(m.a_r, m.a_th, m.a_ph, A.F.res);
      const int g = m.yang;
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
    const PassT p = transmittance_step(m.ok, sg * __fmul_rn(m.dist, A.dscale), lane);
    // march_emit and march_store_sample (csrc/ego_march.hip: the tile-flag rule is explained there) spelled out, one block of stores
    // behind the flags: through the two functions this kernel takes 150 VGPRs for 144 and, alternated with this form five times each,
    // 90.2 - 90.5 us for 88.9 - 89.2 at 4096 x 512 and 103.8 - 104.1 for 103.0 - 103.2 at 16384 x 128 (8 components)
    const float T = carry * p.exc;
    const float wgt = (A.term_eps > 0.f && T < A.term_eps) ? 0.f : p.a * T;
    const int64_t o = ray * S + m.s;
    if (A.tile_active) {
      const unsigned long long nz = __ballot(m.ok && wgt > A.shade_above);
      if ((S & 31) == 0) {
        if (m.ok && (lane & 31) == 0) A.tile_active[o >> 5] = (nz >> (lane & 32) & 0xffffffffull) != 0ull ? 1 : 0;
      } else if (m.ok && (nz >> (lane & 32) & 0xffffffffull) != 0ull && ((lane & 31) == 0 || (o & 31) == 0)) {
        A.tile_active[o >> 5] = 1;
      }
    }
    if (m.ok) {
      if (A.z_out) A.z_out[o] = m.z;
      if (A.coords_out) ((f32x4*)A.coords_out)[o] = f32x4{m.a_r, m.a_th, m.a_ph, m.yang ? 1.f : 0.f};
      if (A.sigma_out) A.sigma_out[o] = sg;
      if (A.alpha) A.alpha[ray * A.alpha_stride + m.s] = p.a;
      if (A.weight) A.weight[o] = wgt;
    }
    carry *= p.tot;
  }
  march_store_tail(A, ray, lane, carry, true, true);
}

}  // namespace

int ego_generic_march(const MarchArgs& a, void* stream) {
  if (int e = check_generic_n_comp(a.C, "march_density")) return e;
  k_march_generic<<<nblk(a.N, 4), 256, 0, (hipStream_t)stream>>>(a);
  return ego_launch_status("k_march_generic");
}
