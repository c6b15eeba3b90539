// libegonerf_hip.so: the fused density march of the tuned shape (16 density components): rows A+B+C+D+E of SURVEY 8a for one ray
// per wave (or two waves), in its factored form (18 table taps per sample) and its dense form (8 taps of a baked node grid,
// csrc/ego_dense.hip), and its entry point ego_march_density.  gfx950 only.
//
// k_march_density is a loop over a ray's 64-sample passes whose steps are named functions, in this file or shared with k_march_generic
// (ego_march.h) and k_raw2alpha (ego_device.h):
//   lut_hints            workgroup prologue: the radius LUT into LDS and the closed forms of its knots (LutHints, normalize_r_fast)   [ego_march.h]
//   march_distances      phase A: z and the interval to the neighbour                                            [ego_march.h]
//   store_stopped        a pass behind exactly zero transmittance: distances and zero weights only                [ego_march.h]
//   march_coords         phase A: point, yin-yang coordinates, normalisation                                     [ego_march.h]
//   sample_occupied      the occupancy mask's decision for the sample
//   density_factored /   phase B, the density feature: 18 table taps through the wave's LDS slab, or 8 corners of the baked node
//   density_dense        grid; one `if constexpr` chooses                                                   [density_dense: ego_march.h]
//   transmittance_step   phase C: alpha, in-pass exclusive product, pass total                                   [ego_device.h]
//   march_store_sample   z, coordinates, sigma, alpha                                                             [ego_march.h]
//   march_emit           weights and tile flags, from the transmittance in front of the pass                      [ego_march.h]
//   Park                 a deferred segment's passes waiting in LDS for that transmittance (NSPLIT > 1)
//   march_store_tail     the column of ones and the background weight                                            [ego_march.h]
// The pieces marked [ego_march.h] are also those of the march that runs inside the folded dense shade kernel (march_wave_rays there;
// k_shade_h with MARCH, csrc/ego_shade.hip).
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

// ego_march_density's checks and its argument block without its launch (ego_march.h): the march that runs inside the shade kernel
// (csrc/ego_shade.hip, MARCH) is described by the same block
int ego_march_fill_args(const ego_scene* sc, const float* rays, int64_t N, int32_t S, const float* z_in, const float* r_sched, const float* jitter,
                        float near_, int32_t coarse, float* z_out, float* alpha, int32_t alpha_stride, float* weight, float* bg_weight,
                        float* coords_out, float* sigma_out, uint8_t* tile_active, MarchArgs* out, bool* tuned) {
  EGO_REQUIRE(sc && rays && N >= 0 && S >= 2, "march_density: null argument or S < 2");
  if (alpha_stride == 0) alpha_stride = S;
  EGO_REQUIRE(alpha_stride >= S && alpha_stride <= S + 64, "march_density: alpha_stride must be in [S, S+64]");
  EGO_REQUIRE(z_in || r_sched, "march_density: need z_in or r_sched");
  EGO_REQUIRE(sc->r_lut && sc->n_r_lut >= 2 && sc->n_r_lut <= 1024, "march_density: r_lut missing or > 1024 entries");
  const ego_vm_field& f = (coarse & 1) ? sc->density_coarse : sc->density;
  if (int e = check_field(f, "march_density")) return e;
  *tuned = f.n_comp == 16;
  *out = MarchArgs{};
  if (N == 0) return EGO_OK;   // an empty call asks nothing of the baked grid
  MarchArgs a = march_args(*sc, f, coarse);
  a.rays = rays; a.z_in = z_in; a.r_sched = r_sched; a.jitter = jitter; a.near_ = near_;
  a.z_out = z_out; a.alpha = alpha; a.weight = weight; a.bg = bg_weight; a.coords_out = coords_out; a.sigma_out = sigma_out;
  a.tile_active = tile_active;
  a.N = N; a.S = S; a.alpha_stride = alpha_stride;
  // the dense form (k_march_density, DENSE): the scene carries the baked node grid of the field this call marches
  if (*tuned && a.dense) {
    const uint64_t grid_bytes = (uint64_t)f.res[0] * (uint64_t)f.res[1] * (uint64_t)f.res[2] * 16u;
    EGO_REQUIRE(((uintptr_t)a.dense & 15) == 0, "march_density: the dense density grid must be 16-byte aligned");
    EGO_REQUIRE(2 * grid_bytes < ((uint64_t)1 << 32), "march_density: the dense density grid must stay under 4 GB (32-bit byte offsets)");
    a.dense_grid_bytes = (uint32_t)grid_bytes;
  }
  *out = a;
  return EGO_OK;
}

extern "C" {

int ego_march_density(const ego_scene* sc, const float* rays, int64_t N, int32_t S, const float* z_in,
                      const float* r_sched, const float* jitter, float near_, int32_t coarse, float* z_out,
                      float* alpha, int32_t alpha_stride, float* weight, float* bg_weight, float* coords_out, float* sigma_out,
                      uint8_t* tile_active, void* stream) {
  EGO_TRACE("ego_march_density");
  MarchArgs a;
  bool tuned = false;
  if (int e = ego_march_fill_args(sc, rays, N, S, z_in, r_sched, jitter, near_, coarse, z_out, alpha, alpha_stride, weight, bg_weight, coords_out,
                                  sigma_out, tile_active, &a, &tuned)) return e;
  if (N == 0) return EGO_OK;
  if (!tuned) return ego_generic_march(a, stream);   // any other component count: the compatibility kernel (csrc/ego_generic_march.hip)
  launch_march(a, march_nsplit(N, (S + 63) / 64, a.dense ? MARCH_DENSE_WAVES : MARCH_WAVES), (hipStream_t)stream);
  return ego_launch_status("k_march_density");
}

}  // extern "C"
