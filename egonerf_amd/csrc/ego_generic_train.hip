// libegonerf_hip.so, part 7 (ego_generic.hip), training of the other model shapes: backward of rows F, G (k_shade_generic_bwd) and of
// the VM lookups (k_scatter_generic), plain fp32; the training forward is the dumping k_shade_generic of ego_generic.hip.  Tap addresses
// and weights: PlaneTaps (ego_device.h), as in the forward; the field and head checks: ego_host.h.
#include "ego_device.h"
#include "ego_host.h"
#include "ego_generic.h"
#include "ego_generic_dev.h"

namespace {

// The data-gradient chain of one sample: do = dL/d(pre-sigmoid) -> dh2 = relu'(h2) W3^T do -> dh1 = relu'(h1) W2^T dh2 -> dx = W1^T dh1
// -> feature gradients through the encodings (d sin(f w)/df = w cos(f w), taken from the dumped cosines) -> dv = B_g^T dfe.  The
// weight gradients are plain A^T B products over the row-major buffers written here and by the dumping forward (ego_weight_grad).
struct GenBwdArgs {
  const float* gp;
  const float* coords;  // [M][4]
  float* dc;            // in: dL/d rgb_sample [M][3]; out: dL/d(pre-sigmoid)
  const float* rgb;     // [M][3] the forward's colours
  const float* x;       // dumps of the forward
  const float* h1;
  const float* h2;
  float* dh2;           // out [M][HID]
  float* dh1;           // out [M][HID]
  float* dfe;           // out [M][64]: columns [32 g, 32 g + 32) of the sample's grid g, the other half zero
  float* dv;            // out [M][ldv]
  int64_t M;
  int32_t app_dim, n_comp, in_c, view_pe, fea_pe, ldx, ldh, ldv;
  int32_t head;
};

// The data-gradient chain on the matrix pipe (fp32 MFMA, as the forward): one wave = 64 samples, one wave per workgroup, slab rows
// [0, HID): the A operand of the running product ([k][sample]), [HID, HID + 32): one 32-column tile of dx, [HID + 32, HID + 64): the
// feature gradients being summed.  B operands from the natural-order copies in the blob (output index contiguous: coalesced loads); the
// relu masks read h2 / h1 and write dh2 / dh1 in the D layout, where a register's 32 lanes are 32 consecutive hidden units of one sample.
template <int HID>
__global__ __launch_bounds__(64) void k_shade_generic_bwd(GenBwdArgs A) {
  __shared__ float slab[HID + 64][64];
  const int lane = threadIdx.x & 63, l31 = lane & 31, kk = lane >> 5;
  float (*sl)[64] = slab;
  auto SL = [&](int row, int col) -> float& { return sl[row][col ^ (row & 31)]; };
  const GenLayout L = gen_layout(A.in_c, A.head == EGO_HEAD_RGB ? 0 : HID, A.n_comp);
  const int64_t n_units = (A.M + 63) >> 6;
  const int D = A.app_dim;
  const float* gw = A.gp;
  constexpr int NT = HID / 32;
  for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const int64_t m_raw = unit * 64 + lane;
    const bool valid = m_raw < A.M;
    const int64_t m = valid ? m_raw : A.M - 1;
    const int g = ((const f32x4*)A.coords)[m].w != 0.f;
    const int ncol = 3 * A.n_comp;
    if (A.head == EGO_HEAD_RGB) {   // colour = features: dfe = dL/d rgb_sample, then dv = B_g^T dfe (basisT [g][col][32])
      float dfe[3] = {A.dc[m * 3], A.dc[m * 3 + 1], A.dc[m * 3 + 2]};
      if (valid) {
#pragma unroll
        for (int f = 0; f < 32; ++f) {
          A.dfe[m * 64 + 32 * g + f] = f < 3 ? dfe[f] : 0.f;
          A.dfe[m * 64 + 32 * (1 - g) + f] = 0.f;
        }
      }
      for (int col = 0; col < ncol; ++col) {
        const float* b0 = A.gp + L.basis + (int64_t)col * 32;
        const float* b1 = b0 + (int64_t)ncol * 32;
        float s = 0.f;
#pragma unroll
        for (int f = 0; f < 3; ++f) s = fmaf(g ? b1[f] : b0[f], dfe[f], s);
        if (valid) A.dv[gen_dv_index(m, col, A.ldv)] = s;
      }
      continue;
    }
    // acc[mt][nt] (+)= slab rows [off, off + n) x rows of the [..][ld] matrix at wbase, columns col0 + 32 nt + l % 32 (zero beyond ncols)
    auto matmul = [&](f32x16 (&acc)[2][NT], int nts, int n, int off, int64_t wbase, int ld, int col0, int ncols) {
      wave_sync_g();
      gen_pipelined<2, NT>((n + 1) / 2,
        [&](int it, float (&bq)[NT]) {
          const int tt = 2 * it + kk, tc = tt < n ? tt : n - 1;
          const float* w = gw + wbase + (int64_t)tc * ld;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const int c = col0 + 32 * nt + l31;
            const float x = w[c < ncols ? c : ncols - 1];
            bq[nt] = (nt < nts && c < ncols) ? x : 0.f;
          }
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
            for (int nt = 0; nt < NT; ++nt)
              if (nt < nts) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt], bq[nt], acc[mt][nt], 0, 0, 0);
        });
      wave_sync_g();
    };
    const bool full = unit * 64 + 64 <= A.M;
    auto zero = [&](f32x16 (&acc)[2][NT]) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
    };
    // relu'(h) mask in the D layout, the masked gradient out (row-major [M][HID]) and into slab rows [0, HID) as the next A operand
    auto mask_out = [&](f32x16 (&acc)[2][NT], const float* h, float* out) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          // a tile's 16 loads first, then its 16 stores: `out` may alias `h` as far as the compiler knows, and load, store, load, store
          // in program order is one exposed round trip per element (6 of this kernel's 10 ms)
          const int hu = 32 * nt + l31;
          float hv[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t ms = gen_d_sample(unit * 64, mt, r, kk), mc = (full || ms < A.M) ? ms : A.M - 1;
            hv[r] = h[mc * A.ldh + hu];
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int smp = gen_d_sample(0, mt, r, kk);
            const int64_t ms = unit * 64 + smp;
            const float v = hv[r] > 0.f ? acc[mt][nt][r] : 0.f;      // threshold backward of torch.nn.ReLU
            if (full || ms < A.M) out[ms * HID + hu] = v;
            SL(hu, smp) = v;
          }
        }
    };
    float d_o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float y = A.rgb[m * 3 + c];
      d_o[c] = A.dc[m * 3 + c] * y * (1.f - y);       // sigmoid'
    }
    if (valid) { A.dc[m * 3] = d_o[0]; A.dc[m * 3 + 1] = d_o[1]; A.dc[m * 3 + 2] = d_o[2]; }
    SL(0, lane) = d_o[0]; SL(1, lane) = d_o[1]; SL(2, lane) = d_o[2];
    f32x16 acc[2][NT];
    zero(acc);
    matmul(acc, NT, 3, 0, L.w3, HID, 0, HID);                 // dh2 (before the mask) = d_o W3, W3 [3][HID]
    mask_out(acc, A.h2, A.dh2);
    zero(acc);
    matmul(acc, NT, HID, 0, L.w2n, HID, 0, HID);              // dh1 (before the mask) = dh2 W2, W2 [j][k]
    mask_out(acc, A.h1, A.dh1);
    // dx = dh1 W1 a 32-column tile at a time, each tile folded into the feature gradients through the encodings' derivatives
    // (d sin(f w) = w cos(f w) df, d cos(f w) = -w sin(f w) df, sines and cosines taken from the dumped x)
#pragma unroll
    for (int f = 0; f < 32; ++f) SL(HID + 32 + f, lane) = 0.f;
    const int base_s = D + 3, base_c = base_s + D * A.fea_pe, vbase_s = base_c + D * A.fea_pe;
    const float* xr = A.x + m * A.ldx;
    for (int c0 = 0; c0 < vbase_s; c0 += 32 * NT) {           // (the view-direction encodings behind vbase_s carry no gradient)
      zero(acc);
      const int nts = (vbase_s - c0 + 31) / 32 < NT ? (vbase_s - c0 + 31) / 32 : NT;
      matmul(acc, nts, HID, 0, L.w1n, A.in_c, c0, A.in_c);    // NT tiles per pass: two MFMAs per k-pair do not cover the loads' latency
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int b0 = c0 + 32 * nt;
        if (b0 >= vbase_s) break;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) SL(HID + l31, gen_d_sample(0, mt, r, kk)) = acc[mt][nt][r];
        wave_sync_g();
        const int b1 = b0 + 32 < vbase_s ? b0 + 32 : vbase_s;
        for (int t = b0; t < b1; ++t) {                        // lane = sample; t is uniform
          int f;
          float coef;
          if (t < D) { f = t; coef = 1.f; }
          else if (t < base_s) continue;                        // the view direction itself
          else if (t < base_c) { const int e = t - base_s, q = e % A.fea_pe; f = e / A.fea_pe; coef = ldexpf(xr[t + D * A.fea_pe], q); }
          else { const int e = t - base_c, q = e % A.fea_pe; f = e / A.fea_pe; coef = -ldexpf(xr[t - D * A.fea_pe], q); }
          SL(HID + 32 + f, lane) += coef * SL(HID + (t - b0), lane);
        }
        wave_sync_g();
      }
    }
    if (valid) {
#pragma unroll
      for (int f = 0; f < 32; ++f) {
        A.dfe[m * 64 + 32 * g + f] = SL(HID + 32 + f, lane);
        A.dfe[m * 64 + 32 * (1 - g) + f] = 0.f;
      }
    }
    // dv = dfe basis_g, basis [g][32][3 C]: a sample's row of A is zero for the grid it does not belong to
    const GenGridMask gm = gen_grid_mask(g, l31);
    wave_sync_g();
    for (int c0 = 0; c0 < ncol; c0 += 32 * NT) {
      zero(acc);
      gen_pipelined<2, 2 * NT>(16,
        [&](int it, float (&bq)[2 * NT]) {
          const float* bw = gw + L.basisn + (int64_t)(2 * it + kk) * ncol;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const int c = c0 + 32 * nt + l31;
            const bool okc = c < ncol;
            const int cc = okc ? c : ncol - 1;
            const float y0 = gm.any_yin ? bw[cc] : 0.f, y1 = gm.any_yang ? bw[(int64_t)32 * ncol + cc] : 0.f;
            bq[2 * nt] = okc ? y0 : 0.f; bq[2 * nt + 1] = okc ? y1 : 0.f;
          }
        },
        [&](int it, const float (&bq)[2 * NT]) {
          const int tt = 2 * it + kk;
          const float x0 = SL(HID + 32 + tt, l31), x1 = SL(HID + 32 + tt, 32 + l31);
          const float a00 = gm.yang0 ? 0.f : x0, a01 = gm.yang1 ? 0.f : x1, a10 = gm.yang0 ? x0 : 0.f, a11 = gm.yang1 ? x1 : 0.f;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            if (c0 + 32 * nt >= ncol) break;
            if (gm.any_yin) {
              acc[0][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a00, bq[2 * nt], acc[0][nt], 0, 0, 0);
              acc[1][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a01, bq[2 * nt], acc[1][nt], 0, 0, 0);
            }
            if (gm.any_yang) {
              acc[0][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a10, bq[2 * nt + 1], acc[0][nt], 0, 0, 0);
              acc[1][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a11, bq[2 * nt + 1], acc[1][nt], 0, 0, 0);
            }
          }
        });
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int c = c0 + 32 * nt + l31;
        if (c0 + 32 * nt >= ncol) break;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t ms = gen_d_sample(unit * 64, mt, r, kk);
            if (c < ncol && (full || ms < A.M)) A.dv[gen_dv_index(ms, c, A.ldv)] = acc[mt][nt][r];
          }
      }
    }
    wave_sync_g();   // the next unit stages into the slab
  }
}

// backward of the VM lookups for any component count (multiple of 4): thread = (sample, plane); float atomics per tap and channel
struct GenScatterArgs {
  DevField F;
  float* gplane[2][3];
  float* gline[2][3];
  const float* coords;   // [M][4]
  const float* d;        // ldd == 0: dfeat [M] (density: relu per plane, EgoNeRF.py:340,346); else dv [M][ldd], column = plane * C + channel
  int64_t M;
  int32_t C, ldd;
};

// A 16-lane group per (sample, plane), lane = channel (16 at a time): every gather and every atomic of a group is one 64-byte line, as in
// the tuned k_vm_scatter (ego_train.hip) but without its run merging.  (Rounds 2-5 had a THREAD per (sample, plane): 64 lanes = 64 texels
// = 64 lines per atomic instruction, 105 ms for the shipped tables at 8192 x 256 - 71 % of a training step of the other heads.)
__global__ __launch_bounds__(256) void k_scatter_generic(GenScatterArgs A) {
#pragma clang fp contract(fast)
  const int c16 = threadIdx.x & 15, C = A.C;
  const bool dens = A.ldd == 0;
  const int64_t n_items = A.M * 3, n_groups = (int64_t)gridDim.x * 16;
  for (int64_t item = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4; item < n_items; item += n_groups) {
    const int64_t m = item / 3;
    const int i = (int)(item - m * 3);
    float ds = 0.f;
    if (dens) {
      ds = A.d[m];
      if (ds == 0.f) continue;
    }
    const f32x4 cc = ((const f32x4*)A.coords)[m];
    const int g = cc.w != 0.f;
    const VMTaps t = vm_setup(cc.x, cc.y, cc.z, A.F.res);
    // (i is a run-time value here: the axis maps as expressions, ego_device.h)
    const PlaneTaps T = plane_taps(t.ax[VM_PLANE_X(i)], t.ax[VM_PLANE_Y(i)], t.ax[VM_LINE_AX(i)], A.F.res[VM_PLANE_X(i)],
                                   g ? A.F.plane[1][i] : A.F.plane[0][i], g ? A.F.line[1][i] : A.F.line[0][i], C);
    float* GP = g ? A.gplane[1][i] : A.gplane[0][i];
    float* GL = g ? A.gline[1][i] : A.gline[0][i];
    if (dens) {   // relu per plane (EgoNeRF.py:340,346): the gradient passes where this plane's sum over channels is positive
      float dot = 0.f;
      for (int c0 = 0; c0 < C; c0 += 16) {
        const int ch = c0 + c16;
        if (ch < C) {
          const float pv = T.P[T.o00 + ch] * T.w00 + T.P[T.o01 + ch] * T.w01 + T.P[T.o10 + ch] * T.w10 + T.P[T.o11 + ch] * T.w11;
          const float lv = T.L[T.ol0 + ch] * T.wl0 + T.L[T.ol1 + ch] * T.wl1;
          dot += pv * lv;
        }
      }
      dot = row_sum16(dot);
      if (!(dot > 0.f)) continue;
    }
    for (int c0 = 0; c0 < C; c0 += 16) {
      const int ch = c0 + c16;
      if (ch >= C) continue;
      const float pv = T.P[T.o00 + ch] * T.w00 + T.P[T.o01 + ch] * T.w01 + T.P[T.o10 + ch] * T.w10 + T.P[T.o11 + ch] * T.w11;
      const float lv = T.L[T.ol0 + ch] * T.wl0 + T.L[T.ol1 + ch] * T.wl1;
      const float di = dens ? ds : A.d[m * A.ldd + i * C + ch];
      const float gp = di * lv, gl = di * pv;
      if (gp != 0.f) {
        if (T.w00 != 0.f) unsafeAtomicAdd(GP + T.o00 + ch, gp * T.w00);
        if (T.w01 != 0.f) unsafeAtomicAdd(GP + T.o01 + ch, gp * T.w01);
        if (T.w10 != 0.f) unsafeAtomicAdd(GP + T.o10 + ch, gp * T.w10);
        if (T.w11 != 0.f) unsafeAtomicAdd(GP + T.o11 + ch, gp * T.w11);
      }
      if (gl != 0.f) {
        if (T.wl0 != 0.f) unsafeAtomicAdd(GL + T.ol0 + ch, gl * T.wl0);
        if (T.wl1 != 0.f) unsafeAtomicAdd(GL + T.ol1 + ch, gl * T.wl1);
      }
    }
  }
}

}  // namespace

// ---- training entry points for the other model shapes (declared in include/egonerf_hip.h) ---------------------------------------
extern "C" {

int ego_shade_backward_generic(const ego_scene* sc, const float* coords, float* dc, const float* rgb, const float* x, int32_t ldx, const float* h1,
                               const float* h2, int32_t ldh, float* dh2, float* dh1, float* dfe64, float* dv, int32_t ldv, int64_t N, int32_t S,
                               void* stream) {
  EGO_TRACE("ego_shade_backward_generic");
  EGO_REQUIRE(N >= 0 && S >= 1 && N * (int64_t)S < (1ll << 31), "shade_backward_generic: bad size");
  if (N == 0) return EGO_OK;
  if (int e = check_generic_shape(sc, "shade_backward_generic", false, true)) return e;
  EGO_REQUIRE(coords && dc && dfe64 && dv && (sc->head == EGO_HEAD_RGB || (rgb && x && h1 && h2 && dh2 && dh1)), "shade_backward_generic: null argument");
  EGO_REQUIRE(ldx >= sc->mlp_in && ldh >= sc->mlp_hidden && (ldv >= 3 * sc->app.n_comp || (ldv == 0 && sc->app.n_comp == 48)),
              "shade_backward_generic: leading dimensions too small (ldv == 0 = the blocked dv of the tuned scatters: 48 components only)");
  GenBwdArgs a{};
  a.gp = sc->packed; a.coords = coords; a.dc = dc; a.rgb = rgb; a.x = x; a.h1 = h1; a.h2 = h2; a.dh2 = dh2; a.dh1 = dh1; a.dfe = dfe64; a.dv = dv;
  a.M = N * (int64_t)S; a.app_dim = sc->app_dim; a.n_comp = sc->app.n_comp; a.in_c = sc->mlp_in; a.view_pe = sc->view_pe; a.fea_pe = sc->fea_pe;
  a.ldx = ldx; a.ldh = ldh; a.ldv = ldv; a.head = sc->head;
  const int64_t units = (a.M + 63) >> 6;
  const unsigned grid = (unsigned)(units < 4096 ? units : 4096);   // one wave per workgroup (its slab: 32 / 48 KB)
  if (sc->mlp_hidden != 128) k_shade_generic_bwd<64><<<grid, 64, 0, (hipStream_t)stream>>>(a);
  else k_shade_generic_bwd<128><<<grid, 64, 0, (hipStream_t)stream>>>(a);
  return ego_launch_status("k_shade_generic_bwd");
}

int ego_scatter_generic(const ego_vm_field* field, const ego_vm_grad* grad, const float* coords, const float* d, int32_t ldd, int64_t N, int32_t S,
                        void* stream) {
  EGO_TRACE("ego_scatter_generic");
  EGO_REQUIRE(field && grad && N >= 0 && S >= 1 && ldd >= 0, "scatter_generic: null argument or bad size");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(coords && d, "scatter_generic: null argument");
  const int C = field->n_comp;
  if (int e = check_vm_field(*field, "scatter_generic", "", false, true, false)) return e;   // (any resolution, as ever)
  EGO_REQUIRE(vm_tables_complete(*grad), "scatter_generic: null table");
  EGO_REQUIRE(ldd == 0 || (ldd >= 3 * C && (ldd & 3) == 0 && ((uintptr_t)d & 15) == 0), "scatter_generic: ldd must be 0 (density) or >= 3 C, a multiple of 4");
  GenScatterArgs a{};
  a.F = make_field(*field);
  for (int g = 0; g < 2; ++g)
    for (int i = 0; i < 3; ++i) { a.gplane[g][i] = grad->plane[g][i]; a.gline[g][i] = grad->line[g][i]; }
  a.coords = coords; a.d = d; a.M = N * (int64_t)S; a.C = C; a.ldd = ldd;
  const int64_t n = a.M * 3, blocks = (n + 15) / 16;   // 16 groups of 16 lanes per workgroup
  k_scatter_generic<<<(unsigned)(blocks < (1 << 20) ? (blocks > 0 ? blocks : 1) : (1 << 20)), 256, 0, (hipStream_t)stream>>>(a);
  return ego_launch_status("k_scatter_generic");
}

}  // extern "C"
