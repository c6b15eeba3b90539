// libegonerf_hip.so: the fused density march of the tuned shape (16 density components): rows A+B+C+D+E of SURVEY 8a for one ray
// per wave (or two waves), in its factored form (18 table taps per sample) and its dense form (8 taps of a baked node grid,
// csrc/ego_dense.hip), and its entry point ego_march_density.  gfx950 only.
//
// k_march_density is a loop over a ray's 64-sample passes whose steps are named functions, in this file or shared with k_march_generic
// (ego_march.h) and k_raw2alpha (ego_device.h):
//   lut_hints            workgroup prologue: the radius LUT into LDS and the closed forms of its knots (LutHints, normalize_r_fast)
//   march_distances      phase A: z and the interval to the neighbour                                            [ego_march.h]
//   store_stopped        a pass behind exactly zero transmittance: distances and zero weights only
//   march_coords         phase A: point, yin-yang coordinates, normalisation                                     [ego_march.h]
//   sample_occupied      the occupancy mask's decision for the sample
//   density_factored /   phase B, the density feature: 18 table taps through the wave's LDS slab, or 8 corners of the baked node
//   density_dense        grid; one `if constexpr` chooses
//   transmittance_step   phase C: alpha, in-pass exclusive product, pass total                                   [ego_device.h]
//   march_store_sample   z, coordinates, sigma, alpha
//   march_emit           weights and tile flags, from the transmittance in front of the pass
//   Park                 a deferred segment's passes waiting in LDS for that transmittance (NSPLIT > 1)
//   march_store_tail     the column of ones and the background weight                                            [ego_march.h]
#include <stdlib.h>
#include "ego_device.h"
#include "ego_host.h"
#include "ego_generic.h"
#include "ego_march.h"

// =============================================================================================
// Fused: rows A+B+C+D+E for one ray per wave.  models/EgoNeRF.py:507-529 (coarse) / 544-553 (fine)
//
// A pass = 64 consecutive samples of the ray, in three phases that hand data over through the wave's own LDS slab:
//   A  lane = sample: distance, point, yin-yang coordinates, radius normalisation (O(1) knot estimate from the LUT's own linear
//      run / exponential tail, checked against the four knots around it, binary search only if the check fails), the three axis
//      tap set-ups -> byte offsets (grid table offsets folded in) + weights to LDS (6 x 16 B per sample)
//   B  lane = (team t = lane >> 2, part p = lane & 3), four rounds of 16 samples x three planes: a team reads its sample's set-up
//      (6 x ds_read_b128 per round: no per-lane recomputation of the set-up, no cross-lane bpermute, no table select), gathers
//      the 18 taps as whole 64-byte lines (part p = one float4 of each) in a two-deep software pipeline (loads of stage k + 1
//      issued before the arithmetic of stage k), reduces inside the quad with DPP; its leader leaves the feature in LDS
//   C  lane = sample: softplus, alpha, DPP transmittance scan with carry, weights, tile flags, outputs
// Round 2's form did phase B with four rounds of five __shfl hand-overs (ds_bpermute + wait each), two more per plane for the
// channel reduction and six in the scan, and recomputed the tap set-up in each of a team's four lanes: 1 256 VALU instructions and
// 66 LDS-queue round trips per pass against 1 000 and 32 here.  Measured (tools/march_timing.py, us old -> new): 4096 x 512
// 106.1 -> 105.2, 16384 x 128 on the pooled tables 106.0 -> 99.7, 16384 x 256 with explicit distances 207.3 -> 183.2; with the
// tap loads replaced by register values 52 us: the kernel is co-limited by the vector L1's 16 clk per load instruction (72 loads
// per pass = 64 us at 16 waves per CU) and VALU issue, which overlap only partly.  Three waves per SIMD (167 VGPRs): at four the
// two 24-register load buffers spill (92 B of scratch per lane, 31 MB per launch through L2: 124 us).  DESIGN.md 4.4.
// =============================================================================================
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

// NSPLIT (1, 2): a ray's passes are dealt to NSPLIT waves of the workgroup (segments of consecutive passes).  One wave per ray
// leaves the launch quantised by wave slots: 3 waves per SIMD = 3 072 slots, so 4 096 rays take a full round and a third of one, 106 us
// where 3 072 rays take 76 and the sustained rate (19.6 us per 1 024 rays) would give 80 (tools/march_timing.py sweep).  Shorter waves
// pack the slots better: 4 096 x 512 with two waves per ray 98 us.  Each wave pays the workgroup prologue (LUT, hints) and the hand-over,
// so it only pays with few rounds of slots and long rays (four waves per ray: 109 us; 16 384 x 128 split in two: 101 -> 118 us); wave
// priorities by phase (+7 %) and a staggered start of the waves of a SIMD (+-0) were measured and are not in the kernel.  Segment 0 streams as before (it knows the transmittance in front of it); a later segment evaluates its
// passes with the transmittance unknown, parks (alpha, in-pass exclusive product) per sample and the pass totals in LDS, and turns
// them into weights once its predecessor has published the carry - with the same multiplications in the same order as the
// one-wave form, so z / alpha / weight / bg / tile flags are bit-identical for every NSPLIT.  One documented difference:
// `coords_out` of passes that the one-wave form stops evaluating (transmittance exactly 0 in front of them, no per-sample alpha asked
// for) holds zeros there and the real coordinates in a deferred segment, which cannot know yet; those samples have weight 0, their
// tiles are never shaded, and tests/test_hip_march_split.py compares coordinates where a colour is read.
constexpr int MARCH_MAXP = 4;   // passes per deferred segment (LDS parking space)
constexpr int MARCH_WAVES = 3;        // waves per SIMD of the factored form (167 VGPRs, see above)
// ... and of the dense form (78-93 VGPRs, 4-12 KB of LDS per workgroup); march_nsplit counts the wave slots of the form it launches.
// Measured, 4096 x 512 step in ms, two runs each: 3 waves 0.4977 / 0.4971, 4: 0.4895 / 0.4888, 5: 0.4878 / 0.4868, 6: 0.4865 / 0.4863
// (factored form: 0.5313 / 0.5304); at 6 the masked one-wave instance spills 20 B per lane, so 5 (NOTEBOOK 12.1).
constexpr int MARCH_DENSE_WAVES = 5;

// The parking space of the workgroup's deferred segments and the slots the carry travels through, in LDS of its own (an NSPLIT = 1
// kernel never touches it and carries none of it).  One object per wave `wv`.
struct Park {
  float (*ax)[2][64];   // this wave's parked passes: alpha, in-pass exclusive product
  float* tot;           // ... and their pass totals
  float* carry;         // this wave's slot: the transmittance behind its segment, once it knows it (its predecessor's lies in front)
  __device__ __forceinline__ explicit Park(int wv) {
    __shared__ float s_ax[4][MARCH_MAXP][2][64];
    __shared__ float s_tot[4][MARCH_MAXP];
    __shared__ float s_carry[4];
    ax = s_ax[wv]; tot = s_tot[wv]; carry = s_carry + wv;
  }
  __device__ __forceinline__ void put(int kp, int lane, const PassT& p) {
    ax[kp][0][lane] = p.a;
    ax[kp][1][lane] = p.exc;
    if (lane == 0) tot[kp] = p.tot;
  }
  __device__ __forceinline__ PassT get(int kp, int lane) const { return {ax[kp][0][lane], ax[kp][1][lane], tot[kp]}; }
  __device__ __forceinline__ void publish(float c) { *carry = c; }              // one lane calls it
  __device__ __forceinline__ float carry_in_front() const { return carry[-1]; }  // behind a workgroup barrier after the predecessor's publish
};

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

// occupancy mask (opt-in): unoccupied samples keep sigma = 0.  Dense form: the field's own taps `t`, which phase B needs anyway, serve
// the mask too where it has the field's resolution (the factored form sets its taps up behind the decision and passes none)
template <bool OCC, bool DENSE>
__device__ __forceinline__ bool sample_occupied(const DevOcc& occ, const DevField& F, const MarchSample& m, const VMTaps& t) {
  if (!OCC || !occ.vol) return true;
  if constexpr (DENSE) {
    const bool same_res = occ.res[0] == F.res[0] && occ.res[1] == F.res[1] && occ.res[2] == F.res[2];   // wave-uniform
    if (same_res) return occ_occupied_taps(occ, m.yang, t.ax[0], t.ax[1], t.ax[2]);
  }
  return occ_occupied(occ, m.yang, m.a_r, m.a_th, m.a_ph);
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
template <bool OCC>
__device__ __forceinline__ float density_dense(const char* __restrict__ dense, uint32_t dense_grid_bytes, const int32_t res[3], int yang,
                                               const VMTaps& t, bool occupied) {
#pragma clang fp contract(fast)
  const Lin1 &Rr = t.ax[0], &Tt = t.ax[1], &Pp = t.ax[2];
  const uint32_t nr16 = (uint32_t)res[0] * 16u, gb = yang != 0 ? dense_grid_bytes : 0u;
  const uint32_t row00 = gb + ((uint32_t)Pp.i0 * (uint32_t)res[1] + (uint32_t)Tt.i0) * nr16;
  const uint32_t row01 = gb + ((uint32_t)Pp.i0 * (uint32_t)res[1] + (uint32_t)Tt.i1) * nr16;
  const uint32_t row10 = gb + ((uint32_t)Pp.i1 * (uint32_t)res[1] + (uint32_t)Tt.i0) * nr16;
  const uint32_t row11 = gb + ((uint32_t)Pp.i1 * (uint32_t)res[1] + (uint32_t)Tt.i1) * nr16;
  const uint32_t c0 = (uint32_t)Rr.i0 * 16u, c1 = (uint32_t)Rr.i1 * 16u;
  const f32x4 g000 = *(const f32x4*)(dense + (row00 + c0)), g001 = *(const f32x4*)(dense + (row00 + c1));
  const f32x4 g010 = *(const f32x4*)(dense + (row01 + c0)), g011 = *(const f32x4*)(dense + (row01 + c1));
  const f32x4 g100 = *(const f32x4*)(dense + (row10 + c0)), g101 = *(const f32x4*)(dense + (row10 + c1));
  const f32x4 g110 = *(const f32x4*)(dense + (row11 + c0)), g111 = *(const f32x4*)(dense + (row11 + c1));
  // every weight in a register of its own (see `issue` in density_factored: a packed multiply must broadcast the LOW half of its operand pair)
  float w6[6] = {Rr.w0, Rr.w1, Tt.w0, Tt.w1, Pp.w0, Pp.w1};
#pragma unroll
  for (int k = 0; k < 6; ++k) asm volatile("" : "+v"(w6[k]));
  const f32x4 v00 = g000 * w6[0] + g001 * w6[1], v01 = g010 * w6[0] + g011 * w6[1];
  const f32x4 v10 = g100 * w6[0] + g101 * w6[1], v11 = g110 * w6[0] + g111 * w6[1];
  const f32x4 u0 = v00 * w6[2] + v01 * w6[3], u1 = v10 * w6[2] + v11 * w6[3];
  const f32x4 d = u0 * w6[4] + u1 * w6[5];
  const float f = (fmaxf(d.x, 0.f) + fmaxf(d.y, 0.f)) + fmaxf(d.z, 0.f);   // relu per plane (EgoNeRF.py:340,346)
  return OCC && !occupied ? 0.f : f;                                       // sample masked out: sigma stays 0 (feature unused)
}

__device__ __forceinline__ void wave_handover() {   // what the wave's lanes wrote to its LDS slab is what its lanes read behind this
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- phase B, factored form, with the tail of phase A that only it needs (the set-up hand-over); owns the LDS slabs of the
// workgroup's four waves.  All 64 lanes of wave `wv` call it, or none (wave-uniform: the software pipeline is either run completely
// or not at all, so its wait counts stay exact).  -> the lane's sample's density feature
template <int C, bool OCC>
__device__ __forceinline__ float density_factored(const DevField& F, int wv, int lane, const MarchSample& m, bool occupied) {
  __shared__ __attribute__((aligned(16))) f32x4 stage[4][6][64];   // per wave: the pass's tap set-ups
  __shared__ float fres[4][64];                                    // per wave: the pass's density features
  const int team = lane >> 2, part = lane & 3;
  {
    // byte offsets of every tap row / line of the sample's grid (the grid's table offsets folded in here, once per sample, so
    // that phase B needs no per-lane table select) + column offsets + the six axis weights
    const Lin1 Rr = lin_setup(m.a_r, F.res[0]), Tt = lin_setup(m.a_th, F.res[1]), Pp = lin_setup(m.a_ph, F.res[2]);
    const auto fu = [](uint32_t v) { return __uint_as_float(v); };
    const bool yg = m.yang != 0;
    const uint32_t pb0 = yg ? F.poff[1][0] : F.poff[0][0], pb1 = yg ? F.poff[1][1] : F.poff[0][1], pb2 = yg ? F.poff[1][2] : F.poff[0][2];
    const uint32_t lb0 = yg ? F.loff[1][0] : F.loff[0][0], lb1 = yg ? F.loff[1][1] : F.loff[0][1], lb2 = yg ? F.loff[1][2] : F.loff[0][2];
    constexpr uint32_t TX = C * 4;   // bytes per texel
    const int nr64 = F.res[0] * (C * 4), nth64 = F.res[1] * (C * 4);
    stage[wv][0][lane] = f32x4{fu(Rr.i0 * TX), fu(Rr.i1 * TX), fu(Tt.i0 * TX), fu(Tt.i1 * TX)};                             // columns: r | theta
    stage[wv][1][lane] = f32x4{fu(pb0 + Tt.i0 * nr64), fu(pb0 + Tt.i1 * nr64), fu(pb1 + Pp.i0 * nr64), fu(pb1 + Pp.i1 * nr64)};  // rows: plane 0 | plane 1
    stage[wv][2][lane] = f32x4{fu(pb2 + Pp.i0 * nth64), fu(pb2 + Pp.i1 * nth64), fu(lb0 + Pp.i0 * TX), fu(lb0 + Pp.i1 * TX)};   // rows: plane 2 | line 0 (phi)
    stage[wv][3][lane] = f32x4{fu(lb1 + Tt.i0 * TX), fu(lb1 + Tt.i1 * TX), fu(lb2 + Rr.i0 * TX), fu(lb2 + Rr.i1 * TX)};         // line 1 (theta) | line 2 (r)
    stage[wv][4][lane] = f32x4{Rr.w0, Rr.w1, Tt.w0, Tt.w1};
    stage[wv][5][lane] = f32x4{Pp.w0, Pp.w1, fu(occupied ? 1u : 0u), 0.f};
  }
  wave_handover();
  // ---- lane = (team, part), four rounds of 16 samples x three planes = 12 stages of six 16-byte loads -------------------------
  // Software pipeline: the loads of stage k + 1 are issued before the arithmetic of stage k (two 6-register-quad buffers), so
  // six to twelve loads stay in flight instead of the queue draining once per plane; a round's set-up (6 x ds_read_b128) is
  // fetched while the previous round's last plane computes.
  {
#pragma clang fp contract(fast)
    f32x4 raw[2][6];
    float wgt6[2][6];
    f32x4 q[6];
    float feat = 0.f;
    const uint32_t p16 = 16u * (uint32_t)part;
    const auto ui = [](float v) { return __float_as_uint(v); };
    auto fetch_setup = [&](int rd, f32x4* dst) {
      const int src = 16 * rd + team;
#pragma unroll
      for (int k = 0; k < 6; ++k) dst[k] = stage[wv][k][src];
    };
    auto issue = [&](const f32x4* Q, int i, f32x4* r6, float* w6) {
      // plane i: columns (x axis), rows (y axis, table offset included), line taps; weights of x / y / line axis
      const uint32_t c0 = ui(i == 2 ? Q[0].z : Q[0].x) + p16, c1 = ui(i == 2 ? Q[0].w : Q[0].y) + p16;
      const uint32_t r0 = ui(i == 0 ? Q[1].x : (i == 1 ? Q[1].z : Q[2].x)), r1 = ui(i == 0 ? Q[1].y : (i == 1 ? Q[1].w : Q[2].y));
      const uint32_t l0 = ui(i == 0 ? Q[2].z : (i == 1 ? Q[3].x : Q[3].z)) + p16, l1 = ui(i == 0 ? Q[2].w : (i == 1 ? Q[3].y : Q[3].w)) + p16;
      const float xw0 = i == 2 ? Q[4].z : Q[4].x, xw1 = i == 2 ? Q[4].w : Q[4].y;
      const float yw0 = i == 0 ? Q[4].z : Q[5].x, yw1 = i == 0 ? Q[4].w : Q[5].y;
      const float lw0 = i == 0 ? Q[5].x : (i == 1 ? Q[4].z : Q[4].x), lw1 = i == 0 ? Q[5].y : (i == 1 ? Q[4].w : Q[4].y);
      r6[0] = *(const f32x4*)(F.base + (r0 + c0)); r6[1] = *(const f32x4*)(F.base + (r0 + c1));
      r6[2] = *(const f32x4*)(F.base + (r1 + c0)); r6[3] = *(const f32x4*)(F.base + (r1 + c1));
      r6[4] = *(const f32x4*)(F.base + l0); r6[5] = *(const f32x4*)(F.base + l1);
      w6[0] = __fmul_rn(yw0, xw0); w6[1] = __fmul_rn(yw0, xw1); w6[2] = __fmul_rn(yw1, xw0); w6[3] = __fmul_rn(yw1, xw1);
      w6[4] = lw0; w6[5] = lw1;
      // every weight in a register of its own: a packed multiply then broadcasts the LOW half of its operand pair; the high-half
      // broadcast form (op_sel without op_sel_hi) is the code-generation feature DESIGN.md 5.1 ties to non-reproducible results
#pragma unroll
      for (int k = 0; k < 6; ++k) asm volatile("" : "+v"(w6[k]));
    };
    auto finish = [&](const f32x4* r6, const float* w6) {
      const f32x4 pv = r6[0] * w6[0] + r6[1] * w6[1] + r6[2] * w6[2] + r6[3] * w6[3];
      const f32x4 lv = r6[4] * w6[4] + r6[5] * w6[5];
      const f32x4 mm = pv * lv;
      float dot = (mm.x + mm.y) + (mm.z + mm.w);
      // the team's four lanes are one DPP quad: two quad_perm adds (no LDS round trip, unlike __shfl_xor's ds_bpermute)
      dot += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(dot), 0xB1 /* quad_perm [1,0,3,2] */, 0xf, 0xf, true));
      dot += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(dot), 0x4E /* quad_perm [2,3,0,1] */, 0xf, 0xf, true));
      feat += fmaxf(dot, 0.f);         // relu per plane (EgoNeRF.py:340,346)
    };
    fetch_setup(0, q);
    issue(q, 0, raw[0], wgt6[0]);
    bool masked = OCC && !(__float_as_int(q[5].z) & 1), masked_next = false;
#pragma unroll
    for (int st = 0; st < 12; ++st) {
      const int rd = st / 3, i = st % 3;
      if (st + 1 < 12) issue(q, (st + 1) % 3, raw[(st + 1) & 1], wgt6[(st + 1) & 1]);
      if (i == 1 && rd + 1 < 4) {   // the set-up is dead once the round's last plane has been issued: fetch the next round's
        fetch_setup(rd + 1, q);
        masked_next = OCC && !(__float_as_int(q[5].z) & 1);
      }
      __builtin_amdgcn_sched_barrier(0);
      finish(raw[st & 1], wgt6[st & 1]);
      if (i == 2) {
        if (masked) feat = 0.f;   // sample masked out: sigma stays 0 (feature unused)
        if (part == 0) fres[wv][16 * rd + team] = feat;
        feat = 0.f;
        masked = masked_next;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  wave_handover();
  return fres[wv][lane];
}

template <int C, bool OCC, int NSPLIT, bool DENSE, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void k_march_density(MarchArgs A) {
  static_assert(C == 16, "one texel = one 64-byte line = the team's four float4 parts");
  __shared__ float lut[1024];
  const LutHints H = lut_hints(A.c, lut);
  // the wave index is wave-uniform: readfirstlane puts it - and with it the ray index and every per-ray base address - into SGPRs
  const int lane0 = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int seg = NSPLIT > 1 ? (wv & (NSPLIT - 1)) : 0;
  const int64_t ray_raw = (int64_t)blockIdx.x * (4 / NSPLIT) + wv / NSPLIT;
  const bool live = ray_raw < A.N;
  if (NSPLIT == 1 && !live) return;            // split launches meet at workgroup barriers below: nobody leaves early
  const int64_t ray = live ? ray_raw : A.N - 1;
  const int S = A.S, n_pass = (S + 63) >> 6, per_seg = (n_pass + NSPLIT - 1) / NSPLIT;
  const int pass0 = seg * per_seg, pass1 = live ? min(n_pass, pass0 + per_seg) : pass0;
  const bool defer = NSPLIT > 1 && seg > 0;    // wave-uniform
  const MarchRay R = march_ray(A.rays, ray);
  float carry = 1.f;   // the transmittance in front of the pass (segment 0; a deferred segment learns it at the hand-over)
  // Exact early termination: once the transmittance in front of a pass is exactly 0 (fp32 underflow behind opaque samples), every
  // remaining weight is a * 0 = 0 and bg stays 0, so the rest of the ray only needs its distances and zero weights - unless the
  // caller wants per-sample alpha / sigma, which are independent of what lies in front.
  const bool may_stop = !A.alpha && !A.sigma_out && !defer;
  for (int s0 = pass0 * 64; s0 < pass1 * 64; s0 += 64) {
    // lane-derived values (team, part, LDS slab addresses, ...) are recomputed per pass from an opaque copy of the lane index:
    // hoisted out of the loop they cost a dozen VGPRs for the whole kernel, which then spill around the 48-register load buffers
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    MarchSample m = march_distances(A.z_in, ray, s0, lane, S, [&](int k) { return sched_z(A.r_sched, A.jitter, ray, k, S, A.near_); });
    if (may_stop && carry == 0.f) {  // wave-uniform
      store_stopped(A, ray, m, lane);
      continue;
    }
    march_coords(m, A.c, R, [&](float r) { return normalize_r_fast(r, lut, A.c.n_lut, A.c.n_r, H); });
    VMTaps t;
    if constexpr (DENSE) t = vm_setup(m.a_r, m.a_th, m.a_ph, A.F.res);
    const bool occupied = sample_occupied<OCC, DENSE>(A.occ, A.F, m, t);
    // a pass whose 64 samples are ALL masked out skips the set-up hand-over and the whole gather; sigma is 0 for every lane then
    const bool pass_occupied = !OCC || __ballot(occupied) != 0ull;
    float f = 0.f;
    if (pass_occupied) {
      if constexpr (DENSE) f = density_dense<OCC>(A.dense, A.dense_grid_bytes, A.F.res, m.yang, t, occupied);
      else f = density_factored<C, OCC>(A.F, wv, lane, m, occupied);
    }
    float sg = 0.f;
    if (occupied) sg = A.softplus ? softplus_shift(f, A.shift) : fmaxf(f, 0.f);
    const PassT p = transmittance_step(m.ok, sg * __fmul_rn(m.dist, A.dscale), lane);
    march_store_sample(A, ray, m, sg, p.a);
    if (!defer) {
      march_emit(A, ray, s0, lane, carry, p.a, p.exc);
      carry *= p.tot;
    } else if constexpr (NSPLIT > 1) {
      Park(wv).put((s0 >> 6) - pass0, lane, p);
    }
  }
  if constexpr (NSPLIT > 1) {
    // the carry travels down the ray's segments: segment k turns its parked passes into weights once segment k - 1 has published
    Park park(wv);
    if (!defer && lane0 == 0) park.publish(carry);
#pragma unroll
    for (int k = 1; k < NSPLIT; ++k) {
      __syncthreads();
      if (seg == k && live) {
        carry = park.carry_in_front();
        for (int kp = 0; kp < pass1 - pass0; ++kp) {
          int lane = lane0;
          asm volatile("" : "+v"(lane));
          const PassT p = park.get(kp, lane);
          march_emit(A, ray, (pass0 + kp) * 64, lane, carry, p.a, p.exc);
          carry *= p.tot;
        }
        if (lane0 == 0) park.publish(carry);
      }
    }
  }
  if (live) march_store_tail(A, ray, lane0, carry, seg == 0, seg == NSPLIT - 1);
}

// Rays split over two waves when one wave per ray would leave the launch quantised by wave slots (see k_march_density): fewer than
// two rounds of slots and at least two passes per half (at most MARCH_MAXP in the deferred half).
static int march_nsplit(int64_t N, int n_pass, int waves_per_simd) {
  // wave slots (waves_per_simd of the variant that is launched, on 4 SIMDs per CU) of the current device
  const int slots = device_cus() * 4 * waves_per_simd;
  int nsplit = ((double)N / slots < 2.0 && n_pass >= 4 && (n_pass + 1) / 2 <= MARCH_MAXP) ? 2 : 1;
  // experiments and tests/test_hip_march_split.py (which flips it between calls of one process, hence read per launch: a getenv is
  // ~50 ns against a 5 us launch): EGO_MARCH_SPLIT forces 1 or 2 where the shape allows it
  if (const char* e = getenv("EGO_MARCH_SPLIT")) {
    const int forced = atoi(e);
    if (forced == 1 || (forced == 2 && n_pass >= 2 && (n_pass + 1) / 2 <= MARCH_MAXP)) nsplit = forced;
  }
  return nsplit;
}

// the kernel-argument block of a march of field `f` of the scene (coarse & 1: its pooled tables, & 2: the fine LUT); the call's own
// buffers and sizes are the entry point's to add
static MarchArgs march_args(const ego_scene& sc, const ego_vm_field& f, int coarse) {
  MarchArgs a{};
  a.c = make_coords(sc, (coarse & 2) != 0);
  a.F = make_field(f);
  a.dense = (const char*)((coarse & 1) ? sc.density_coarse_dense : sc.density_dense);
  a.occ = make_occ(sc, coarse & 1);
  a.C = f.n_comp; a.softplus = sc.act_softplus;
  a.shift = sc.density_shift; a.dscale = sc.distance_scale; a.term_eps = sc.term_eps; a.shade_above = fmaxf(sc.weight_thres, 0.f);
  return a;
}

template <bool OCC, int NSPLIT, bool DENSE>
static void launch_march(const MarchArgs& a, hipStream_t st) {
  k_march_density<16, OCC, NSPLIT, DENSE, DENSE ? MARCH_DENSE_WAVES : MARCH_WAVES><<<nblk(a.N, 4 / NSPLIT), 256, 0, st>>>(a);
}
// (mask, waves per ray, form) -> the instantiation
static void launch_march(const MarchArgs& a, int nsplit, hipStream_t st) {
  switch ((a.occ.vol ? 4 : 0) | (nsplit == 2 ? 2 : 0) | (a.dense ? 1 : 0)) {
    case 0: return launch_march<false, 1, false>(a, st);
    case 1: return launch_march<false, 1, true>(a, st);
    case 2: return launch_march<false, 2, false>(a, st);
    case 3: return launch_march<false, 2, true>(a, st);
    case 4: return launch_march<true, 1, false>(a, st);
    case 5: return launch_march<true, 1, true>(a, st);
    case 6: return launch_march<true, 2, false>(a, st);
    default: return launch_march<true, 2, true>(a, st);
  }
}

extern "C" {

int ego_march_density(const ego_scene* sc, const float* rays, int64_t N, int32_t S, const float* z_in,
                      const float* r_sched, const float* jitter, float near_, int32_t coarse, float* z_out,
                      float* alpha, int32_t alpha_stride, float* weight, float* bg_weight, float* coords_out, float* sigma_out,
                      uint8_t* tile_active, void* stream) {
  EGO_TRACE("ego_march_density");
  EGO_REQUIRE(sc && rays && N >= 0 && S >= 2, "march_density: null argument or S < 2");
  if (alpha_stride == 0) alpha_stride = S;
  EGO_REQUIRE(alpha_stride >= S && alpha_stride <= S + 64, "march_density: alpha_stride must be in [S, S+64]");
  EGO_REQUIRE(z_in || r_sched, "march_density: need z_in or r_sched");
  EGO_REQUIRE(sc->r_lut && sc->n_r_lut >= 2 && sc->n_r_lut <= 1024, "march_density: r_lut missing or > 1024 entries");
  const ego_vm_field& f = (coarse & 1) ? sc->density_coarse : sc->density;
  if (int e = check_field(f, "march_density")) return e;
  if (N == 0) return EGO_OK;
  MarchArgs a = march_args(*sc, f, coarse);
  a.rays = rays; a.z_in = z_in; a.r_sched = r_sched; a.jitter = jitter; a.near_ = near_;
  a.z_out = z_out; a.alpha = alpha; a.weight = weight; a.bg = bg_weight; a.coords_out = coords_out; a.sigma_out = sigma_out;
  a.tile_active = tile_active;
  a.N = N; a.S = S; a.alpha_stride = alpha_stride;
  if (f.n_comp != 16) return ego_generic_march(a, stream);   // any other component count: the compatibility kernel (csrc/ego_generic_march.hip)
  // the dense form (k_march_density, DENSE): the scene carries the baked node grid of the field this call marches
  if (a.dense) {
    const uint64_t grid_bytes = (uint64_t)f.res[0] * (uint64_t)f.res[1] * (uint64_t)f.res[2] * 16u;
    EGO_REQUIRE(((uintptr_t)a.dense & 15) == 0, "march_density: the dense density grid must be 16-byte aligned");
    EGO_REQUIRE(2 * grid_bytes < ((uint64_t)1 << 32), "march_density: the dense density grid must stay under 4 GB (32-bit byte offsets)");
    a.dense_grid_bytes = (uint32_t)grid_bytes;
  }
  launch_march(a, march_nsplit(N, (S + 63) / 64, a.dense ? MARCH_DENSE_WAVES : MARCH_WAVES), (hipStream_t)stream);
  return ego_launch_status("k_march_density");
}

}  // extern "C"
