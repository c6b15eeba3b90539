// libegonerf_hip.so, part 7: the render path for model shapes OTHER than the one every shipped config resolves to
// (opt.py:87-100 lets a user set n_lamb_sigma / n_lamb_sh, data_dim_color, featureC, view_pe, fea_pe).  The MFMA kernels of
// ego_shade.hip / ego_train.hip (shape: ego_tuned.h) bake 48 appearance components, app_dim 27, a 150 -> 128 -> 128 -> 3 MLP with two encoding frequencies and 16
// density components into their register layouts; these kernels take the shape as runtime numbers (hidden width as a template
// parameter) and compute in plain fp32 with the reference's operation order, so that any reference checkpoint renders on the
// device.  They are a compatibility path, an order of magnitude slower than the tuned one (forward AND, since round 4, backward); the
// host layer picks them exactly when ego_shape_is_tuned() is false.
//
//   this file             : weight packing and the forward head, inference and training (k_generic_pack, k_shade_generic)
//   ego_generic_train.hip : the backward chain and the atomic table scatter (k_shade_generic_bwd, k_scatter_generic)
//   ego_generic_march.hip : k_march_generic, rows A-E for C density components (multiple of 4, <= 48), lane = sample, wave per ray
//   ego_generic_dev.h     : what the three share on the device (blob layout, pipelined loads, slab synchronisation, sincos)
//
//   k_shade_generic : rows F, G (EgoNeRF.py:349-413, tensorBase.py:54-78): appearance gather + per-grid basis + positional
//                     encoding + MLP_Fea for n_comp <= 48 (multiple of 4), app_dim <= 32, featureC in {64, 128}, view_pe, fea_pe <= 8
#include "ego_device.h"
#include "ego_host.h"
#include "ego_generic.h"
#include "ego_generic_dev.h"

namespace {

struct GenShadeArgs {
  DevField F;
  const float* gp;       // generic packed weights (ego_generic_pack)
  const float* rays;     // SHADE: [N][6]
  const float* coords;   // SHADE: [M][4]
  const float* c7n;      // APP: [M][7]
  const float* feat;     // MLP: [M][app_dim]
  const float* dirs;     // MLP: [M][3]
  float* out;
  const uint8_t* tile_active;
  int64_t M;
  int32_t S, app_dim, n_comp, in_c, view_pe, fea_pe;
  int32_t head;          // EGO_HEAD_MLP_FEA: features -> MLP -> sigmoid; EGO_HEAD_RGB: colour = features 0..2 (RGBRender, tensorBase.py:37-39)
  // training forward (DUMP): row-major per-sample activations for the backward pass / the weight-gradient products
  float* dump_x;   // [M][ldx]: the MLP input row in the reference's column order (tensorBase.py:68-75)
  float* dump_h1;  // [M][ldh]: relu(h1)
  float* dump_h2;  // [M][ldh]: relu(h2)
  float* dump_v;   // [M][ldv]: plane x line products, column = plane * C + channel
  int32_t ldx, ldh, ldv;
};

__global__ void k_generic_pack(const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                               const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ b3,
                               const float* __restrict__ basis_yin, const float* __restrict__ basis_yang, int in_c, int hid, int n_comp,
                               int app_dim, float* __restrict__ out) {
  const GenLayout L = gen_layout(in_c, hid, n_comp);
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= L.total) return;
  float v = 0.f;
  if (idx < L.b1) { const int k = (int)(idx / hid), j = (int)(idx % hid); v = w1[(int64_t)j * in_c + k]; }
  else if (idx < L.w2t) v = b1[idx - L.b1];
  else if (idx < L.b2) { const int64_t e = idx - L.w2t; const int k = (int)(e / hid), j = (int)(e % hid); v = w2[(int64_t)j * hid + k]; }
  else if (idx < L.w3) v = b2[idx - L.b2];
  else if (idx < L.b3) v = w3[idx - L.w3];
  else if (idx < L.basis) { const int c = (int)(idx - L.b3); v = (c < 3 && b3) ? b3[c] : 0.f; }   // b3 == null: EGO_HEAD_RGB (hid = in_c = 0)
  else if (idx < L.w1n) {
    const int64_t e = idx - L.basis;
    const int f = (int)(e & 31), col = (int)((e >> 5) % (3 * n_comp)), g = (int)((e >> 5) / (3 * n_comp));
    if (f < app_dim) v = (g ? basis_yang : basis_yin)[(int64_t)f * (3 * n_comp) + col];
  }
  else if (idx < L.w2n) v = w1[idx - L.w1n];
  else if (idx < L.basisn) v = w2[idx - L.w2n];
  else {
    const int64_t e = idx - L.basisn;
    const int ncol = 3 * n_comp, col = (int)(e % ncol), f = (int)((e / ncol) & 31), g = (int)(e / ((int64_t)32 * ncol));
    if (f < app_dim) v = (g ? basis_yang : basis_yin)[(int64_t)f * ncol + col];
  }
  out[idx] = v;
}

// one wave = 64 samples (lane = sample); 2 waves per workgroup; per wave an LDS slab [HID][64] that first stages chunks of the MLP
// input and then holds relu(h1)
template <int HID, int MODE, bool DUMP = false>
__global__ __launch_bounds__(128) void k_shade_generic(GenShadeArgs A) {
  // the weight blob through the CONSTANT address space: the dumping variant's stores may alias a plain global pointer as far as the
  // compiler can tell, the uniform weight rows then come through VECTOR loads (128 VGPRs per row) instead of scalar ones and the kernel
  // spills 434 registers (restrict-qualified locals did not convince it); nothing writes the blob while a kernel reads it
  const gen_cfloat* gp = (const gen_cfloat*)A.gp;
  float* dump_x = A.dump_x;
  float* dump_h1 = A.dump_h1;
  float* dump_h2 = A.dump_h2;
  float* dump_v = A.dump_v;
  float* outp = A.out;
  __shared__ float slab[2][HID][64];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float (*sl)[64] = slab[wv];
  const GenLayout L = gen_layout(A.in_c, A.head == EGO_HEAD_RGB ? 0 : HID, A.n_comp);   // no MLP block in the RGB head's blob
  const int64_t n_units = (A.M + 63) >> 6;
  for (int64_t unit = (int64_t)blockIdx.x * 2 + wv; unit < n_units; unit += (int64_t)gridDim.x * 2) {
    if (MODE == G_SHADE && A.tile_active) {   // two 32-sample tiles per unit (the last unit of a ragged M may hold one): skip when neither is read
      const int64_t n_tiles = (A.M + 31) >> 5, t1 = 2 * unit + 1;
      if (!A.tile_active[2 * unit] && !(t1 < n_tiles && A.tile_active[t1])) continue;
    }
    const int64_t m_raw = unit * 64 + lane;
    const bool valid = m_raw < A.M;
    const int64_t m = valid ? m_raw : A.M - 1;
    float feat[32];
#pragma unroll
    for (int f = 0; f < 32; ++f) feat[f] = 0.f;
    float vd[3] = {0.f, 0.f, 0.f};
    const int l31 = lane & 31, kk = lane >> 5;
    const float* gw = A.gp;
    // slab element (row, sample): the column is swizzled with the row so that the 32 lanes of a D tile (32 rows, one sample) hit 32 banks
    auto SL = [&](int row, int col) -> float& { return sl[row][col ^ (row & 31)]; };
    if (MODE == G_MLP) {
#pragma unroll
      for (int f = 0; f < 32; ++f)
        if (f < A.app_dim) feat[f] = A.feat[m * A.app_dim + f];
      vd[0] = A.dirs[m * 3]; vd[1] = A.dirs[m * 3 + 1]; vd[2] = A.dirs[m * 3 + 2];
    } else {
      // ---- rows F: appearance gather (EgoNeRF.py:349-413) + this sample's grid's basis (EgoNeRF.py:99-100) ----
      float a[3];
      int g;
      if (MODE == G_APP) {
        const float* p = A.c7n + m * 7;
        g = (p[6] == 0.f) ? 0 : 1;
        const int b = g ? 3 : 0;
        a[0] = p[b]; a[1] = p[b + 1]; a[2] = p[b + 2];
      } else {
        const f32x4 cc = ((const f32x4*)A.coords)[m];
        a[0] = cc.x; a[1] = cc.y; a[2] = cc.z; g = cc.w != 0.f;
        const uint32_t ray = (uint32_t)(m / A.S);
        const float* R = A.rays + (int64_t)ray * 6;
        vd[0] = R[3]; vd[1] = R[4]; vd[2] = R[5];
      }
      const VMTaps t = vm_setup(a[0], a[1], a[2], A.F.res);
      const int C = A.n_comp;
      // features = basis_g (plane value x line value): the unit's [64 samples][3 C] products go through the slab a plane at a time and
      // meet basisT [g][column][32 features] on the matrix pipe; a sample's row of A is zero for the grid it does not belong to, so both
      // grids accumulate into the same tiles (the lane = sample form took 2 x 32 scalar weights and 32 selects per column and sample)
      f32x16 accf[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) accf[mt][r] = 0.f;
      const GenGridMask gm = gen_grid_mask(g, l31);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const PlaneTaps T = EGO_PLANE_TAPS_OF(A.F, C, g, i, t.ax);
        for (int c4 = 0; c4 < C; c4 += 4) {
          const f32x4 pv = tap4(T.p00, c4) * T.w00 + tap4(T.p01, c4) * T.w01 + tap4(T.p10, c4) * T.w10 + tap4(T.p11, c4) * T.w11;
          const f32x4 lv = tap4(T.l0, c4) * T.wl0 + tap4(T.l1, c4) * T.wl1;
          const f32x4 pr = pv * lv;
          if (DUMP && valid) *(f32x4*)(dump_v + m * A.ldv + i * C + c4) = pr;
#pragma unroll
          for (int e = 0; e < 4; ++e) SL(c4 + e, lane) = pr[e];
        }
        wave_sync_g();
        gen_pipelined<4, 2>((C + 1) / 2,
          [&](int it, float (&bq)[2]) {
            const int tt = 2 * it + kk, tc = tt < C ? tt : C - 1;
            const float* bw = gw + L.basis + (int64_t)(i * C + tc) * 32 + l31;
            bq[0] = gm.any_yin ? bw[0] : 0.f;
            bq[1] = gm.any_yang ? bw[(int64_t)3 * C * 32] : 0.f;
          },
          [&](int it, const float (&bq)[2]) {
            const int tt = 2 * it + kk;
            const bool ok = tt < C;
            const int tc = ok ? tt : C - 1;
            const float x0 = ok ? SL(tc, l31) : 0.f, x1 = ok ? SL(tc, 32 + l31) : 0.f;
            if (gm.any_yin) {
              accf[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(gm.yang0 ? 0.f : x0, bq[0], accf[0], 0, 0, 0);
              accf[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(gm.yang1 ? 0.f : x1, bq[0], accf[1], 0, 0, 0);
            }
            if (gm.any_yang) {
              accf[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(gm.yang0 ? x0 : 0.f, bq[1], accf[0], 0, 0, 0);
              accf[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(gm.yang1 ? x1 : 0.f, bq[1], accf[1], 0, 0, 0);
            }
          });
        wave_sync_g();
      }
      // the D layout (gen_d_sample; the column is the feature) back to lane = sample through the slab
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) SL(l31, gen_d_sample(0, mt, r, kk)) = accf[mt][r];
      wave_sync_g();
#pragma unroll
      for (int f = 0; f < 32; ++f)
        if (f < A.app_dim) feat[f] = SL(f, lane);
      wave_sync_g();
    }
    if (MODE == G_APP) {
      if (valid) {
#pragma unroll
        for (int f = 0; f < 32; ++f)
          if (f < A.app_dim) outp[m * A.app_dim + f] = feat[f];
      }
      continue;
    }
    if (A.head == EGO_HEAD_RGB) {   // RGBRender (tensorBase.py:37-39): the colour IS the (3-channel) appearance feature; no sigmoid, no clamp
      if (valid) {
        float* op = outp + m * 3;
        op[0] = feat[0]; op[1] = feat[1]; op[2] = feat[2];
      }
      continue;
    }
    // ---- row G: mlp_in = [features, viewdirs, PE(features), PE(viewdirs)] (tensorBase.py:68-75) -> Linear relu Linear relu Linear ----
    // Both hidden layers on the matrix pipe in fp32 (v_mfma_f32_32x32x2_f32: products and sums in fp32, as the reference's): the unit's 64
    // samples x HID hidden units are 2 x HID / 32 tiles of 16 accumulators; A = the staged inputs from the slab (lane = (sample l % 32,
    // k = l / 32)), B = two rows of W^T by coalesced VECTOR loads (lane = (k, hidden unit l % 32)).  The lane = sample form it replaces
    // fed every FMA an SGPR weight: 128 weights per input row through a 104-SGPR file, every row two or three dependent scalar-load ->
    // FMA phases with one wave per SIMD to hide them (5-10 % of the fp32 rate).
    constexpr int NT = HID / 32;
    f32x16 acc[2][NT];
    auto bias = [&](int64_t off) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float bv = gw[off + 32 * nt + l31];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mt][nt][r] = bv;
      }
    };
    // n staged inputs (slab rows off .. off + n - 1) times rows wrow0 + t * stride of the [rows][HID] matrix at `wbase`
    auto matmul = [&](int n, int off, int64_t wbase, int wrow0, int stride) {
      wave_sync_g();   // the slab rows were written by lane = sample
      gen_pipelined<2, NT>((n + 1) / 2,
        [&](int it, float (&bq)[NT]) {
          const int tt = 2 * it + kk, tc = tt < n ? tt : n - 1;
          const float* w = gw + wbase + (int64_t)(wrow0 + tc * stride) * HID + l31;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) bq[nt] = w[32 * nt];
        },
        [&](int it, const float (&bq)[NT]) {
          const int tt = 2 * it + kk;
          const bool ok = tt < n;
          const int tc = ok ? tt : n - 1;
          float av[2];
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) { const float x = SL(off + tc, 32 * mt + l31); av[mt] = ok ? x : 0.f; }
#pragma unroll
          for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt], bq[nt], acc[mt][nt], 0, 0, 0);
        });
      wave_sync_g();   // ... and will be overwritten by the next chunk
    };
    // relu of the accumulators -> slab [hidden][sample] (+ the row-major dump: a register's 32 lanes are 32 consecutive hidden units of
    // one sample - 128-byte stores): the D layout of gen_d_sample, the column is hidden unit 32 nt + l % 32
    const bool full = unit * 64 + 64 <= A.M;
    auto relu_out = [&](float* dump) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int smp = gen_d_sample(0, mt, r, kk), hu = 32 * nt + l31;
            const float hv = fmaxf(acc[mt][nt][r], 0.f);
            SL(hu, smp) = hv;
            if (DUMP) {
              const int64_t ms = unit * 64 + smp;
              if (full || ms < A.M) dump[ms * A.ldh + hu] = hv;   // (`full`, a scalar, spares 128 exec-mask branches: the stores then leave in one batch)
            }
          }
    };
    auto consume = [&](int n, int row0, int stride, int off = 0) {
      if (DUMP && valid)
        for (int tt = 0; tt < n; ++tt) dump_x[m * A.ldx + row0 + tt * stride] = SL(off + tt, lane);
      matmul(n, off, L.w1t, row0, stride);
    };
    bias(L.b1);
    const int D = A.app_dim;
    // chunk 1: the raw features and the view direction (rows 0 .. D + 2)
#pragma unroll
    for (int f = 0; f < 32; ++f)
      if (f < D) SL(f, lane) = feat[f];
    SL(D, lane) = vd[0]; SL(D + 1, lane) = vd[1]; SL(D + 2, lane) = vd[2];
    consume(D + 3, 0, 1);
    // PE(features): element-major, frequency-minor; all sines (rows base + f * fea_pe + q), then all cosines
    {
      const int base_s = D + 3, base_c = base_s + D * A.fea_pe;
      float fr = 1.f;
      for (int q = 0; q < A.fea_pe; ++q, fr *= 2.f) {
        // sine and cosine of one argument from ONE reduction (gen_sincos), the cosines parked in rows D .. 2 D - 1 of the slab (2 D <= 64 <= HID)
#pragma unroll
        for (int f = 0; f < 32; ++f)
          if (f < D) {
            float sv, cv;
            gen_sincos(__fmul_rn(feat[f], fr), sv, cv);
            SL(f, lane) = sv; SL(D + f, lane) = cv;
          }
        consume(D, base_s + q, A.fea_pe);
        consume(D, base_c + q, A.fea_pe, D);
      }
      const int vbase_s = base_c + D * A.fea_pe, vbase_c = vbase_s + 3 * A.view_pe;
      fr = 1.f;
      for (int q = 0; q < A.view_pe; ++q, fr *= 2.f) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          float sv, cv;
          gen_sincos(__fmul_rn(vd[d], fr), sv, cv);
          SL(d, lane) = sv; SL(3 + d, lane) = cv;
        }
        consume(3, vbase_s + q, A.view_pe);
        consume(3, vbase_c + q, A.view_pe, 3);
      }
    }
    relu_out(dump_h1);
    bias(L.b2);
    matmul(HID, 0, L.w2t, 0, 1);
    relu_out(dump_h2);
    wave_sync_g();
    const gen_cfloat* w3 = gp + L.w3;
    const gen_cfloat* b3 = gp + L.b3;
    float o[3] = {b3[0], b3[1], b3[2]};
    for (int j = 0; j < HID; ++j) {   // three outputs: lane = sample again, the weights as scalars
      const float hv = SL(j, lane);
      o[0] = fmaf(w3[j], hv, o[0]); o[1] = fmaf(w3[HID + j], hv, o[1]); o[2] = fmaf(w3[2 * HID + j], hv, o[2]);
    }
    if (valid) {
      float* op = outp + m * 3;
      op[0] = sigmoidf(o[0]); op[1] = sigmoidf(o[1]); op[2] = sigmoidf(o[2]);
    }
    wave_sync_g();   // the next unit stages into the slab
  }
}

}  // namespace

int check_generic_shape(const ego_scene* sc, const char* who, bool need_tables, bool need_mlp, bool need_packed) {
  if (!sc) return ego_fail(EGO_E_BADARG, "%s: null scene", who);
  const bool rgb_head = sc->head == EGO_HEAD_RGB;   // tensorBase.py:194-196: `assert self.app_dim == 3`; no MLP
  if (int e = check_head_shape(sc, who, EGO_E_UNSUPPORTED, !rgb_head, need_mlp)) return e;
  if (int e = check_generic_n_comp(sc->app.n_comp, who, "appearance ")) return e;
  if (sc->head != EGO_HEAD_MLP_FEA && !rgb_head) return ego_fail(EGO_E_BADARG, "%s: scene.head %d (EGO_HEAD_MLP_FEA or EGO_HEAD_RGB)", who, sc->head);
  if (rgb_head) {
    if (sc->app_dim != 3) return ego_fail(EGO_E_BADARG, "%s: the RGB head needs app_dim == 3 (got %d)", who, sc->app_dim);
    if (sc->mlp_in != 0 || sc->mlp_hidden != 0) return ego_fail(EGO_E_BADARG, "%s: the RGB head has no MLP (mlp_in / mlp_hidden must be 0)", who);
  }
  if (need_tables)
    if (int e = check_vm_field(sc->app, who, "appearance ", false, false)) return e;
  if (need_packed && !sc->packed) return ego_fail(EGO_E_BADARG, "%s: scene.packed is null (call ego_pack_mlp first)", who);
  return EGO_OK;
}

bool ego_shape_is_tuned(const ego_scene* sc) {
  return sc->head == EGO_HEAD_MLP_FEA && sc->app_dim == 27 && sc->app.n_comp == 48 && sc->mlp_in == 150 && sc->mlp_hidden == 128 && sc->view_pe == 2 &&
         sc->fea_pe == 2;
}

int64_t ego_generic_packed_floats(const ego_scene* sc) {
  return gen_layout(sc->mlp_in, sc->mlp_hidden, sc->app.n_comp).total;
}

int ego_generic_pack(const ego_scene* sc, float* out, void* stream) {
  if (int e = check_generic_shape(sc, "pack_mlp", false, true, false)) return e;
  const int64_t n = ego_generic_packed_floats(sc);
  const bool mlp = sc->head != EGO_HEAD_RGB;   // the RGB head's blob is [4 zeros | basisT]
  k_generic_pack<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(sc->mlp_w[0], sc->mlp_b[0], sc->mlp_w[1], sc->mlp_b[1], sc->mlp_w[2],
                                                                              mlp ? sc->mlp_b[2] : nullptr, sc->basis[0], sc->basis[1], sc->mlp_in, sc->mlp_hidden,
                                                                              sc->app.n_comp, sc->app_dim, out);
  return ego_launch_status("k_generic_pack");
}

// one wave per 64-sample unit, two waves per workgroup; the hidden width picks the instance (64, or 0 = the RGB head, which leaves before the MLP)
template <int MODE, bool DUMP = false>
static int launch_shade(const ego_scene* sc, const GenShadeArgs& a, void* stream) {
  const int64_t units = (a.M + 63) >> 6;
  const unsigned grid = (unsigned)((units + 1) / 2 < 2048 ? (units + 1) / 2 : 2048);
  if (sc->mlp_hidden != 128) k_shade_generic<64, MODE, DUMP><<<grid, 128, 0, (hipStream_t)stream>>>(a);
  else k_shade_generic<128, MODE, DUMP><<<grid, 128, 0, (hipStream_t)stream>>>(a);
  return ego_launch_status(DUMP ? "k_shade_generic<DUMP>" : "k_shade_generic");
}

static GenShadeArgs shade_args(const ego_scene* sc) {
  GenShadeArgs a{};
  a.F = make_field(sc->app);
  a.gp = sc->packed;
  a.app_dim = sc->app_dim; a.n_comp = sc->app.n_comp; a.in_c = sc->mlp_in; a.view_pe = sc->view_pe; a.fea_pe = sc->fea_pe; a.head = sc->head;
  return a;
}

int ego_generic_shade(const ego_scene* sc, const float* rays, const float* coords, int64_t N, int32_t S, float* rgb, const uint8_t* tile_active,
                      void* stream) {
  if (int e = check_generic_shape(sc, "shade", true, true)) return e;
  if (!coords) return ego_fail(EGO_E_BADARG, "shade: coords (from ego_march_density) is required for this model shape");
  GenShadeArgs a = shade_args(sc);
  a.rays = rays; a.coords = coords; a.out = rgb; a.tile_active = tile_active; a.M = N * (int64_t)S; a.S = S;
  return launch_shade<G_SHADE>(sc, a, stream);
}

int ego_generic_app_feature(const ego_scene* sc, const float* c7n, int64_t M, float* out, void* stream) {
  if (int e = check_generic_shape(sc, "app_feature", true, false)) return e;
  GenShadeArgs a = shade_args(sc);
  a.c7n = c7n; a.out = out; a.M = M; a.S = 1;
  return launch_shade<G_APP>(sc, a, stream);
}

int ego_generic_mlp_fea(const ego_scene* sc, const float* viewdirs, const float* feat, int64_t M, float* rgb, void* stream) {
  if (int e = check_generic_shape(sc, "mlp_fea", false, true)) return e;
  if (sc->head == EGO_HEAD_RGB) return ego_fail(EGO_E_UNSUPPORTED, "mlp_fea: the RGB head has no MLP (RGBRender returns the features)");
  GenShadeArgs a = shade_args(sc);
  a.feat = feat; a.dirs = viewdirs; a.out = rgb; a.M = M; a.S = 1;
  return launch_shade<G_MLP>(sc, a, stream);
}

// ---- training entry points for the other model shapes (declared in include/egonerf_hip.h) ---------------------------------------
extern "C" {

int ego_shade_train_generic(const ego_scene* sc, const float* rays, const float* coords, int64_t N, int32_t S, float* rgb, float* x, int32_t ldx,
                            float* h1, float* h2, int32_t ldh, float* v, int32_t ldv, void* stream) {
  EGO_TRACE("ego_shade_train_generic");
  EGO_REQUIRE(N >= 0 && S >= 1 && N * (int64_t)S < (1ll << 31), "shade_train_generic: bad size");
  if (N == 0) return EGO_OK;
  if (int e = check_generic_shape(sc, "shade_train_generic", true, true)) return e;
  const bool rgb_head = sc->head == EGO_HEAD_RGB;   // no MLP: x / h1 / h2 are not written and may be null
  EGO_REQUIRE(rays && coords && rgb && v && (rgb_head || (x && h1 && h2)), "shade_train_generic: null argument");
  EGO_REQUIRE(ldx >= sc->mlp_in && ldh >= sc->mlp_hidden && ldv >= 3 * sc->app.n_comp && (ldv & 3) == 0 && ((uintptr_t)v & 15) == 0,
              "shade_train_generic: leading dimensions too small (or v not 16-byte aligned / ldv not a multiple of 4)");
  GenShadeArgs a = shade_args(sc);
  a.rays = rays; a.coords = coords; a.out = rgb; a.M = N * (int64_t)S; a.S = S;
  a.dump_x = x; a.dump_h1 = h1; a.dump_h2 = h2; a.dump_v = v; a.ldx = ldx; a.ldh = ldh; a.ldv = ldv;
  return launch_shade<G_SHADE, true>(sc, a, stream);
}

}  // extern "C"
