// Internal: what the two density marches share - k_march_density (csrc/ego_march.hip, 16 density components) and k_march_generic
// (csrc/ego_generic_march.hip, any other count): the one kernel-argument block, and the pieces of a 64-sample pass that are the same
// text in both (lane = sample): phase A (distances, normalised coordinates) and the stores behind a ray's last pass.  The
// transmittance step between them is transmittance_step (ego_device.h), which k_raw2alpha uses too.  What k_march_generic does NOT
// share stays spelled out there, each piece with what sharing it measured: the schedule distance, the density sum, the weight / tile
// flag / output stores.
// Further down: the pieces of k_march_density's dense one-wave form that the shade kernel's in-wave march shares with it (LUT hints,
// normalize_r_fast, the stores of phase C, density_dense) and that march itself (march_wave_rays).
#pragma once
#include "ego_device.h"

// Everything a march launch reads, by value in the kernel-argument segment (wave-uniform: SGPRs).  Filled by ego_march_density
// (csrc/ego_march.hip) alone.  A member cannot promise __restrict__ (the qualifier tells the compiler nothing there); the pieces that
// gain from it take the pointer as a __restrict__ parameter of their own (sched_z, density_dense).
// The ORDER of the members is measured, not taste: it decides which members one scalar load fetches together and with that the
// kernels' SGPR allocation.  In this order (the kernels' parameter order before there was a block) every instance is as fast as it
// was; with the pointers, the sizes and the scalars grouped, the dense one-wave instance took 62.5 us for 61.5 at 16384 x 128.
struct MarchArgs {
  DevCoords c;
  DevField F;
  const char* dense;           // the field's baked node grid (csrc/ego_dense.hip) or null; k_march_density's dense form only
  uint32_t dense_grid_bytes;   // bytes of one grid of it: the yang grid follows the yin grid
  const float* rays;
  int64_t N;
  int32_t S, C;                // samples per ray; density components (k_march_generic: k_march_density is compiled for 16)
  const float* z_in; const float* r_sched; const float* jitter;   // explicit distances, or the schedule and its optional jitter
  float near_;
  int32_t softplus;
  float shift, dscale;
  float* z_out; float* alpha;
  int32_t alpha_stride;
  float* weight; float* bg; float* coords_out; float* sigma_out;
  DevOcc occ;                  // k_march_generic always takes the exact trilinear test (occ_sample) and never reads `cell`
  float term_eps, shade_above;
  uint8_t* tile_active;
};

struct MarchRay {
  float ox, oy, oz, dx, dy, dz;
};
__device__ __forceinline__ MarchRay march_ray(const float* rays, int64_t ray) {
  const float* R = rays + ray * 6;
  return {R[0], R[1], R[2], R[3], R[4], R[5]};
}

// ---- phase A: lane = sample ------------------------------------------------------------------------------------------------------
struct MarchSample {
  int s;       // the lane's sample, clamped to the ray's last one
  bool ok;     // ... which is its own (false: an idle lane of the tail pass, which computes the last sample again and stores nothing)
  float z, dist;
  float a_r, a_th, a_ph;   // march_coords
  int yang;
};

// z[s] and the distance to its right neighbour (left neighbour for the last sample: dists repeat the last interval), from explicit
// distances or, without them, from the caller's schedule `zz(k)`
template <class SchedZ>
__device__ __forceinline__ MarchSample march_distances(const float* z_in, int64_t ray, int s0, int lane, int S, SchedZ zz) {
  MarchSample m;
  m.s = min(s0 + lane, S - 1);
  m.ok = (s0 + lane) < S;
  const int sn = (m.s < S - 1) ? m.s + 1 : m.s - 1;
  float zn;
  if (z_in) {
    m.z = z_in[ray * S + m.s];
    zn = z_in[ray * S + sn];
  } else {
    m.z = zz(m.s);
    zn = zz(sn);
  }
  m.dist = (m.s < S - 1) ? __fsub_rn(zn, m.z) : __fsub_rn(m.z, zn);
  return m;
}

// the sample point, its yin-yang coordinates and their normalisation; the radius through the caller's `norm_r(r)`
template <class NormR>
__device__ __forceinline__ void march_coords(MarchSample& m, const DevCoords& c, const MarchRay& R, NormR norm_r) {
  const float px = __fadd_rn(R.ox, __fmul_rn(R.dx, m.z)), py = __fadd_rn(R.oy, __fmul_rn(R.dy, m.z)), pz = __fadd_rn(R.oz, __fmul_rn(R.dz, m.z));
  const YinYang y = yinyang_from_xyz(px, py, pz, c);
  m.a_r = norm_r(y.r);
  m.a_th = normalize_ang(y.th, c.th_near, c.th_inv);
  m.a_ph = normalize_ang(y.ph, c.ph_near, c.ph_inv);
  m.yang = y.yang;
}

// ---- behind a ray's last pass: with an environment map the reference appends a column of ones to alpha (EgoNeRF.py:587); the
// background weight is the transmittance behind the last sample
__device__ __forceinline__ void march_store_tail(const MarchArgs& A, int64_t ray, int lane, float carry, bool ones, bool bg) {
  if (ones && A.alpha && lane < A.alpha_stride - A.S) A.alpha[ray * A.alpha_stride + A.S + lane] = 1.f;
  if (bg && A.bg && lane == 0) A.bg[ray] = carry;
}

struct LutHints {   // derived per workgroup from the LUT itself (so any monotone LUT works: the estimate is only a starting point)
  float r0;         // first knot spacing (lut[1] - lut[0])
  float lin_end;    // last knot of the arithmetic run
  float inv_l2r;    // 1 / log2(ratio) of the exponential tail
  float shift;      // tail knots: shift + r0' * ratio^k
  float inv_r0;
  float tail_k0;    // index offset of the tail estimate
};

// Workgroup prologue (every thread calls it; three workgroup barriers): copies the radius LUT into `lut` and derives the hints from it.
__device__ __forceinline__ LutHints lut_hints(const DevCoords& c, float* lut) {
  __shared__ int s_nlin;
  __shared__ LutHints s_hints;
  for (int i = threadIdx.x; i < c.n_lut; i += blockDim.x) lut[i] = c.r_lut[i];
  if (threadIdx.x == 0) s_nlin = c.n_lut - 1;
  __syncthreads();
  // arithmetic run = the leading intervals equal to lut[1] - lut[0] up to float32 rounding of k * r0 (the reference replaces
  // every shell thinner than r0 by a step of r0): the first interval that is not ends it
  const float r0 = lut[1] - lut[0];
  int first_other = c.n_lut - 1;
  for (int i = threadIdx.x; i + 1 < c.n_lut; i += blockDim.x)
    if (!(fabsf((lut[i + 1] - lut[i]) - r0) <= r0 * 1e-3f)) first_other = min(first_other, i);
  if (first_other < c.n_lut - 1) atomicMin(&s_nlin, first_other);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n = c.n_lut, nl = s_nlin;
    LutHints H;
    H.r0 = r0; H.inv_r0 = 1.f / r0; H.lin_end = lut[nl];
    // tail: lut[k] = shift + a * ratio^k: ratio from the last three knots, shift from the last two
    float ratio = 2.f, sh = 0.f;
    if (n - nl >= 4) {
      const float a = lut[n - 3], b = lut[n - 2], cc = lut[n - 1];
      ratio = (cc - b) / (b - a);
      sh = b - (cc - b) / (ratio - 1.f);
    }
    H.shift = sh;
    H.inv_l2r = 1.f / __log2f(fmaxf(ratio, 1.0000001f));
    // kf = log2(r - shift) * inv_l2r + tail_k0 must give kf = k for r = lut[k]: calibrate on the last knot
    H.tail_k0 = (float)(n - 1) - __log2f(fmaxf(lut[n - 1] - sh, 1e-30f)) * H.inv_l2r;
    if (n - nl < 4) { H.lin_end = 3.0e38f; }   // (almost) all linear: never take the tail form
    s_hints = H;
  }
  __syncthreads();
  // wave-uniform: keep the six values in SGPRs (read from LDS they would occupy six VGPRs for the whole kernel)
  const auto sf = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
  LutHints H;
  H.r0 = sf(s_hints.r0); H.lin_end = sf(s_hints.lin_end); H.inv_l2r = sf(s_hints.inv_l2r); H.shift = sf(s_hints.shift);
  H.inv_r0 = sf(s_hints.inv_r0); H.tail_k0 = sf(s_hints.tail_k0);
  return H;
}

// searchsorted(lut, r, right) clamped to [1, n - 1] (coordinates.py:125-127) without the 10-step dependent search: estimate the
// knot from the closed forms, read the four knots around it, accept if they bracket r, else search.  Bit-identical to normalize_r.
__device__ __forceinline__ float normalize_r_fast(float r, const float* lut, int n_lut, int n_r, const LutHints& H) {
  float kf;
  if (r < H.lin_end) kf = r * H.inv_r0;
  else kf = fmaf(__log2f(fmaxf(r - H.shift, 1e-30f)), H.inv_l2r, H.tail_k0);
  kf = fminf(fmaxf(kf, 0.f), (float)(n_lut - 1));
  const int c0 = (int)kf + 1;                      // estimate of lo = #{i : lut[i] <= r}
  // knots c0 - 2 .. c0 + 1; virtual knots below index 0 are <= r, beyond the end are > r
  int lo = c0 - 2;
  bool ok = r == r;
#pragma unroll
  for (int d = -2; d <= 1; ++d) {
    const int j = c0 + d;
    const bool in = (unsigned)j < (unsigned)n_lut;
    const float v = lut[in ? j : 0];
    const bool le = in ? (v <= r) : (j < 0);
    lo += le ? 1 : 0;
    if (d == -2) ok = ok && le;                    // the window's first knot must not exceed r
    if (d == 1) ok = ok && (!le || j >= n_lut - 1);  // and its last one must (unless it is the LUT's end)
  }
  if (!ok) {   // rare: estimate off by more than a knot (or NaN): the reference's search
    int l = 0, h = n_lut;
    while (l < h) {
      const int mid = (l + h) >> 1;
      if (!(lut[mid] > r)) l = mid + 1; else h = mid;
    }
    lo = l;
  }
  const int k_out = lo < 1 ? 1 : (lo > n_lut - 1 ? n_lut - 1 : lo);
  const int k_in = k_out - 1;
  const float g0 = lut[k_in], g1 = lut[k_out];
  const float frac = __fdiv_rn(__fsub_rn(r, g0), __fsub_rn(g1, g0));
  const float v = __fdiv_rn(__fadd_rn((float)k_in, frac), (float)n_r);
  return __fsub_rn(__fmul_rn(v, 2.0f), 1.0f);
}

// ---- phase C behind the transmittance step: lane = sample.  (k_march_generic holds the same rules in one block of its own: through these
// two functions it measured slower, csrc/ego_generic_march.hip.)
// what does not depend on the transmittance in front of the sample
__device__ __forceinline__ void march_store_sample(const MarchArgs& A, int64_t ray, const MarchSample& m, float sg, float a) {
  if (!m.ok) return;
  const int64_t o = ray * A.S + m.s;
  if (A.z_out) A.z_out[o] = m.z;
  if (A.coords_out) ((f32x4*)A.coords_out)[o] = f32x4{m.a_r, m.a_th, m.a_ph, m.yang ? 1.f : 0.f};
  if (A.sigma_out) A.sigma_out[o] = sg;
  if (A.alpha) A.alpha[ray * A.alpha_stride + m.s] = a;
}

// weights and tile flags of the pass at s0 from (alpha, in-pass exclusive product) and the transmittance `carry` in front of the pass
__device__ __forceinline__ void march_emit(const MarchArgs& A, int64_t ray, int s0, int lane, float carry, float a, float exc) {
  const int S = A.S, s = min(s0 + lane, S - 1);
  const bool ok = (s0 + lane) < S;
  const float T = carry * exc;
  const float wgt = (A.term_eps > 0.f && T < A.term_eps) ? 0.f : a * T;  // early termination (opt-in)
  if (A.tile_active) {
    // 32-sample shade tiles are cut from the flat [N*S] order: lanes 0-31 / 32-63 of this pass are (parts of) tiles
    // a tile is shaded iff it holds a sample whose colour is read: weight > shade_above (0, or rayMarch_weight_thres)
    const unsigned long long nz = __ballot(ok && wgt > A.shade_above);
    const int64_t o = ray * S + s;
    if ((S & 31) == 0) {
      // whole tiles per pass half: written unconditionally (0 or 1), so the caller need not clear the flags first
      if (ok && (lane & 31) == 0) A.tile_active[o >> 5] = (nz >> (lane & 32) & 0xffffffffull) != 0ull ? 1 : 0;
    } else if (ok && (nz >> (lane & 32) & 0xffffffffull) != 0ull && ((lane & 31) == 0 || (o & 31) == 0)) {
      A.tile_active[o >> 5] = 1;  // tiles straddle rays: flags are pre-zeroed by the caller and only set here
    }
  }
  if (ok && A.weight) A.weight[ray * S + s] = wgt;
}

// A pass that lies behind exactly zero transmittance (see may_stop in the kernel): its distances, zero weights, cleared whole tiles
__device__ __forceinline__ void store_stopped(const MarchArgs& A, int64_t ray, const MarchSample& m, int lane) {
  if (!m.ok) return;
  const int64_t o = ray * A.S + m.s;
  if (A.z_out) A.z_out[o] = m.z;
  if (A.coords_out) ((f32x4*)A.coords_out)[o] = f32x4{0.f, 0.f, 0.f, 0.f};  // never shaded (tile flags stay 0); defined values anyway
  if (A.weight) A.weight[o] = 0.f;
  if (A.tile_active && (A.S & 31) == 0 && (lane & 31) == 0) A.tile_active[o >> 5] = 0;
}

// DENSE (inference scenes that carry ego_scene.density_dense, csrc/ego_dense.hip): phase B reads the baked node grid instead of the
// 18 table taps.  Per plane i the factored feature dot_i = sum_c bilerp(plane_i,c) * lerp(line_i,c) is the trilinear interpolation of
// G_i[phi][theta][r] = sum_c plane_i,c[node] * line_i,c[node] - plane and line interpolate on one lattice along independent axes, and an
// out-of-range tap has weight 0 in either form - so with lane = sample a pass needs 8 loads of 16 B per lane, one per cell corner
// carrying (G_0, G_1, G_2, 0), and no LDS hand-over: no stage / fres slabs, no wave barriers, far fewer registers (WPE waves per SIMD
// instead of 3).  Everything around the density feature is the same text for both forms.
//
// ---- phase B, dense form: lane = sample.  The eight corners of the sample's cell as base + 32-bit byte offset, all eight loads
// issued before the first use; interpolation along r, then theta, then phi, with lin_setup's weights (out-of-range taps: clamped
// index, weight 0); relu per plane, planes summed in order.
// In two steps, so that a caller with several samples per lane (march_wave_rays) can issue the loads of all of them first:
// density_dense_load = the addresses and the eight loads, density_dense_finish = the interpolation; density_dense is one behind the other.
struct DenseCorners {
  f32x4 g000, g001, g010, g011, g100, g101, g110, g111;
};
__device__ __forceinline__ DenseCorners density_dense_load(const char* __restrict__ dense, uint32_t dense_grid_bytes, const int32_t res[3], int yang,
                                                           const VMTaps& t) {
  const Lin1 &Rr = t.ax[0], &Tt = t.ax[1], &Pp = t.ax[2];
  const uint32_t nr16 = (uint32_t)res[0] * 16u, gb = yang != 0 ? dense_grid_bytes : 0u;
  const uint32_t row00 = gb + ((uint32_t)Pp.i0 * (uint32_t)res[1] + (uint32_t)Tt.i0) * nr16;
  const uint32_t row01 = gb + ((uint32_t)Pp.i0 * (uint32_t)res[1] + (uint32_t)Tt.i1) * nr16;
  const uint32_t row10 = gb + ((uint32_t)Pp.i1 * (uint32_t)res[1] + (uint32_t)Tt.i0) * nr16;
  const uint32_t row11 = gb + ((uint32_t)Pp.i1 * (uint32_t)res[1] + (uint32_t)Tt.i1) * nr16;
  const uint32_t c0 = (uint32_t)Rr.i0 * 16u, c1 = (uint32_t)Rr.i1 * 16u;
  DenseCorners g;
  g.g000 = *(const f32x4*)(dense + (row00 + c0)); g.g001 = *(const f32x4*)(dense + (row00 + c1));
  g.g010 = *(const f32x4*)(dense + (row01 + c0)); g.g011 = *(const f32x4*)(dense + (row01 + c1));
  g.g100 = *(const f32x4*)(dense + (row10 + c0)); g.g101 = *(const f32x4*)(dense + (row10 + c1));
  g.g110 = *(const f32x4*)(dense + (row11 + c0)); g.g111 = *(const f32x4*)(dense + (row11 + c1));
  return g;
}
template <bool OCC>
__device__ __forceinline__ float density_dense_finish(const DenseCorners& g, const VMTaps& t, bool occupied) {
#pragma clang fp contract(fast)
  const Lin1 &Rr = t.ax[0], &Tt = t.ax[1], &Pp = t.ax[2];
  // every weight in a register of its own (see `issue` in density_factored: a packed multiply must broadcast the LOW half of its operand pair)
  float w6[6] = {Rr.w0, Rr.w1, Tt.w0, Tt.w1, Pp.w0, Pp.w1};
#pragma unroll
  for (int k = 0; k < 6; ++k) asm volatile("" : "+v"(w6[k]));
  const f32x4 v00 = g.g000 * w6[0] + g.g001 * w6[1], v01 = g.g010 * w6[0] + g.g011 * w6[1];
  const f32x4 v10 = g.g100 * w6[0] + g.g101 * w6[1], v11 = g.g110 * w6[0] + g.g111 * w6[1];
  const f32x4 u0 = v00 * w6[2] + v01 * w6[3], u1 = v10 * w6[2] + v11 * w6[3];
  const f32x4 d = u0 * w6[4] + u1 * w6[5];
  const float f = (fmaxf(d.x, 0.f) + fmaxf(d.y, 0.f)) + fmaxf(d.z, 0.f);   // relu per plane (EgoNeRF.py:340,346)
  return OCC && !occupied ? 0.f : f;                                       // sample masked out: sigma stays 0 (feature unused)
}
template <bool OCC>
__device__ __forceinline__ float density_dense(const char* __restrict__ dense, uint32_t dense_grid_bytes, const int32_t res[3], int yang,
                                               const VMTaps& t, bool occupied) {
  return density_dense_finish<OCC>(density_dense_load(dense, dense_grid_bytes, res, yang, t), t, occupied);
}

__device__ __forceinline__ void wave_handover() {   // what the wave's lanes wrote to its LDS slab is what its lanes read behind this
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the dense one-wave march inside another kernel (k_shade_h with MARCH, csrc/ego_shade.hip): one wave marches rays [ray0, ray1)
// of a launch whose block `A` asks for no mask and no early termination by `term_eps`; tile flags (`A.tile_active`) only with whole tiles
// per ray (S a multiple of 32): march_emit / store_stopped then write every flag of the wave's rays unconditionally and the same wave
// reads them back, no flag byte belongs to two waves and none has to be cleared beforehand.  It is k_march_density's
// one-wave dense loop (NSPLIT = 1, OCC off) made of the same functions in the same order per sample and per ray, so every output has
// the bits of that kernel; what differs is the schedule: P consecutive passes of a ray are evaluated side by side - a pass's alpha and
// in-pass product do not depend on the transmittance in front of it (Park rests on the same fact) - so that the coordinate chains, the LUT reads
// and the 8 corner loads of P passes are in flight together, and only the emit walks the passes in sample order with the carry.  A
// group's last passes beyond the ray's end evaluate the ray's last pass again and store nothing (the code stays straight-line).  A pass
// that turns out to lie behind exactly zero transmittance is stored as k_march_density stores it (store_stopped), evaluated or not.
template <int P>
__device__ __forceinline__ void march_wave_rays(const MarchArgs& A, const float* lut, const LutHints& H, int64_t ray0, int64_t ray1, int lane0) {
  const int S = A.S, n_pass = (S + 63) >> 6;
  const bool may_stop = !A.alpha && !A.sigma_out;
  for (int64_t ray = ray0; ray < ray1; ++ray) {
    const MarchRay R = march_ray(A.rays, ray);
    float carry = 1.f;
    for (int k0 = 0; k0 < n_pass; k0 += P) {
      int lane = lane0;
      asm volatile("" : "+v"(lane));
      MarchSample m[P];
#pragma unroll
      for (int p = 0; p < P; ++p)
        m[p] = march_distances(A.z_in, ray, min(k0 + p, n_pass - 1) * 64, lane, S, [&](int k) { return sched_z(A.r_sched, A.jitter, ray, k, S, A.near_); });
      if (may_stop && carry == 0.f) {  // wave-uniform
#pragma unroll
        for (int p = 0; p < P; ++p)
          if (k0 + p < n_pass) store_stopped(A, ray, m[p], lane);
        continue;
      }
      VMTaps t[P];
#pragma unroll
      for (int p = 0; p < P; ++p) {
        march_coords(m[p], A.c, R, [&](float r) { return normalize_r_fast(r, lut, A.c.n_lut, A.c.n_r, H); });
        t[p] = vm_setup(m[p].a_r, m[p].a_th, m[p].a_ph, A.F.res);
      }
      float f[P];
      DenseCorners g[P];  // the corner loads of all P passes ahead of the first interpolation
#pragma unroll
      for (int p = 0; p < P; ++p) g[p] = density_dense_load(A.dense, A.dense_grid_bytes, A.F.res, m[p].yang, t[p]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < P; ++p) f[p] = density_dense_finish<false>(g[p], t[p], true);
      float sg[P];
      PassT ps[P];
#pragma unroll
      for (int p = 0; p < P; ++p) {
        sg[p] = A.softplus ? softplus_shift(f[p], A.shift) : fmaxf(f[p], 0.f);
        ps[p] = transmittance_step(m[p].ok, sg[p] * __fmul_rn(m[p].dist, A.dscale), lane);
      }
#pragma unroll
      for (int p = 0; p < P; ++p) {
        if (k0 + p >= n_pass) break;
        if (may_stop && carry == 0.f) {
          store_stopped(A, ray, m[p], lane);
        } else {
          march_store_sample(A, ray, m[p], sg[p], ps[p].a);
          march_emit(A, ray, (k0 + p) * 64, lane, carry, ps[p].a, ps[p].exc);
          carry *= ps[p].tot;
        }
      }
    }
    march_store_tail(A, ray, lane0, carry, true, true);
  }
}

// host side (csrc/ego_march.hip): validates a march call as ego_march_density does and fills its argument block, launching nothing.
// EGO_OK with *tuned = whether k_march_density (16 components) would serve it.
int ego_march_fill_args(const ego_scene* sc, const float* rays, int64_t N, int32_t S, const float* z_in, const float* r_sched, const float* jitter,
                        float near_, int32_t coarse, float* z_out, float* alpha, int32_t alpha_stride, float* weight, float* bg_weight,
                        float* coords_out, float* sigma_out, uint8_t* tile_active, MarchArgs* out, bool* tuned);
// csrc/ego_shade.hip: the one-launch eval render - does the scene qualify (no device work), and the launch: the folded dense shade kernel
// whose waves march the rays of block `m` themselves ahead of their tiles
bool ego_can_march_in_shade(const ego_scene* sc, int32_t S);
int ego_march_shade_composite(const ego_scene* sc, const MarchArgs& m, float* rgb_map, float* depth, float* bg_map, float* env_map, void* stream);
