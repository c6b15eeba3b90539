// libegonerf_hip.so, part 9: backward of the separately callable stages (the reference's public stage methods), so that a loss built from
// them - the sparsity term of train.py:266-272, a custom render loop, a probe of the field - differentiates like the reference's autograd:
//
//   ego_density_feature_backward : F.grid_sample backward of compute_densityfeature / compute_coarse_densityfeature (EgoNeRF.py:291-347,
//                                  :232-289) plus the AvgPool2d / AvgPool1d backward of the coarse tables (EgoNeRF.py:124-133)
//   ego_app_feature_backward     : compute_appfeature (EgoNeRF.py:349-413): grid_sample backward + basis_mat_{yin,yang}.weight
//   ego_mlp_fea_backward         : MLPRender_Fea / MLPRender (tensorBase.py:54-78, :107-129)
//   ego_sh_render_backward       : SHRender (tensorBase.py:30-34, sh.py:87-112)
//   ego_feature2density_backward : TensorBase.feature2density (tensorBase.py:415-419)
//   ego_raw2alpha_backward       : raw2alpha (tensorBase.py:22-27)
//
// The table gradients reuse the training step's scatters: the sorted, bit-reproducible walk (csrc/ego_scatter_sorted.hip) where the
// tables have the shipped shape (16 density / 48 appearance components), ego_scatter_generic's float atomics otherwise.  Coordinates
// [M][7] are turned into the scatters' [M][4] (own grid's normalised r, theta, phi + grid flag) by a small adaptor; the forward's
// N x S samples become M x 1.  Weight gradients are ego_weight_grad_det products over row-major per-sample buffers.  Table sizes, axis
// maps and the tap description are ego_device.h's; the field / head / null-table checks ego_host.h's.
#include "ego_device.h"
#include "ego_host.h"
#include <algorithm>

namespace {

inline int64_t al256(int64_t b) { return (b + 255) & ~(int64_t)255; }
constexpr int LD = 160;        // row width of the weight-gradient B operands (ego_weight_grad_det's 5 column blocks)

// c7n [M][7] -> coords [M][4] = (r, theta, phi) of the sample's own grid + grid flag (EgoNeRF.py:292-296: yin iff the last column is 0)
__global__ void k_c7n_to_coords(const float* __restrict__ c7n, int64_t M, float* __restrict__ coords) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const float* p = c7n + m * 7;
  const int g = p[6] == 0.f ? 0 : 1;
  f32x4 c;
  c.x = p[3 * g]; c.y = p[3 * g + 1]; c.z = p[3 * g + 2]; c.w = (float)g;
  ((f32x4*)coords)[m] = c;
}

// AvgPool2d(2, 2) / AvgPool1d(2, 2) backward (floor mode: an odd last row / column gets nothing) of one channel-last table:
// full [H][W][C] = coarse [H/2][W/2][C] / 4 (planes), full [L][C] = coarse [L/2][C] / 2 (lines, W == 1); written, not accumulated
__global__ void k_avgpool_backward(const float* __restrict__ gc, int H, int W, int C, float* __restrict__ gf) {
  const int64_t n = (int64_t)H * W * C;
  const bool line = W == 1;
  const int Hc = H / 2, Wc = line ? 1 : W / 2;
  const float scale = line ? 0.5f : 0.25f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int64_t hw = i / C;
    const int w = (int)(hw % W), h = (int)(hw / W);
    const int hc = h >> 1, wc = line ? 0 : (w >> 1);
    float v = 0.f;
    if (hc < Hc && wc < Wc) v = __fmul_rn(gc[((int64_t)hc * Wc + wc) * C + c], scale);
    gf[i] = v;
  }
}

// Appearance backward, per sample (thread = sample): v = plane x line products of the own grid (the forward's gather arithmetic),
// dv = basis_g^T g, g64 = g in columns [32 g, 32 g + app_dim) (the other grid's half zero: g64^T v gives both basis gradients in one
// product).  v rows are LD wide with zero padding; dv is row-major [M][LD] or (blocked) the sorted walk's [tile][9][32][16] layout.
__global__ __launch_bounds__(256) void k_app_bwd_prep(DevField F, const float* __restrict__ basis_yin, const float* __restrict__ basis_yang,
                                                      const float* __restrict__ c7n, const float* __restrict__ g, int64_t M, int D, int C,
                                                      float* __restrict__ coords, float* __restrict__ v, float* __restrict__ g64,
                                                      float* __restrict__ dv, int blocked) {
  extern __shared__ float sb[];   // basis [2][D][3C]
  const int ncol = 3 * C;
  for (int i = threadIdx.x; i < 2 * D * ncol; i += blockDim.x) sb[i] = i < D * ncol ? basis_yin[i] : basis_yang[i - D * ncol];
  __syncthreads();
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) {   // the blocked dv's last tile: its padding rows are read when the walk takes max |dv|
    if (blocked && m < (M + 31) / 32 * 32)
      for (int col = 0; col < 144; ++col) dv[(m >> 5) * (32 * 144) + (int64_t)(col >> 4) * 512 + (m & 31) * 16 + (col & 15)] = 0.f;
    return;
  }
  const float* p = c7n + m * 7;
  const int gr = p[6] == 0.f ? 0 : 1;
  const float a0 = p[3 * gr], a1 = p[3 * gr + 1], a2 = p[3 * gr + 2];
  f32x4 cc;
  cc.x = a0; cc.y = a1; cc.z = a2; cc.w = (float)gr;
  ((f32x4*)coords)[m] = cc;
  float gv[32];
#pragma unroll
  for (int f = 0; f < 32; ++f) gv[f] = f < D ? g[m * D + f] : 0.f;
  float* g64r = g64 + m * 64;
  for (int f = 0; f < 64; ++f) g64r[f] = ((f >> 5) == gr && (f & 31) < D) ? gv[f & 31] : 0.f;
  const float* B = sb + gr * D * ncol;
  const VMTaps t = vm_setup(a0, a1, a2, F.res);
  float* vr = v + m * LD;
  for (int i = 0; i < 3; ++i) {
    const PlaneTaps T = EGO_PLANE_TAPS_OF(F, C, gr, i, t.ax);
    for (int c = 0; c < C; ++c) {
      const float pv = T.p00[c] * T.w00 + T.p01[c] * T.w01 + T.p10[c] * T.w10 + T.p11[c] * T.w11;
      const float lv = T.l0[c] * T.wl0 + T.l1[c] * T.wl1;
      const int col = i * C + c;
      vr[col] = pv * lv;
      float s = 0.f;
      for (int f = 0; f < D; ++f) s = fmaf(gv[f], B[f * ncol + col], s);
      const int64_t di = blocked ? (m >> 5) * (32 * 144) + (int64_t)(col >> 4) * 512 + (m & 31) * 16 + (col & 15) : m * LD + col;
      dv[di] = s;
    }
  }
  for (int col = ncol; col < LD; ++col) vr[col] = 0.f;
}

// MLPRender_Fea / MLPRender backward (tensorBase.py:54-78, :107-129) in plain fp32: a workgroup of 128 threads takes TS samples,
// rebuilds the MLP input x (features, viewdirs, PE(features), PE(viewdirs)), h1, h2 and the pre-sigmoid values from the fp32 weights,
// then runs the chain back: d(pre) = g sigmoid' , dh2 = relu'(h2) W3^T d(pre), dh1 = relu'(h1) W2^T dh2, dx = W1^T dh1, and dx through
// both positional encodings into d_feat / d_viewdirs.  x | 1, h1, h2 (LD-wide rows, zero padding), dh1, dh2 and d(pre) go to the
// workspace for the weight-gradient products.
struct MlpArgs {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  const float *dirs, *feat, *g;
  float *d_feat, *d_dirs;
  float *X, *H1, *H2, *DH1, *DH2, *DP;
  int64_t M;
  int D, in_c, hid, view_pe, fea_pe, ldx;
};

template <int TS>
__global__ __launch_bounds__(128) void k_mlp_bwd(MlpArgs A) {
  extern __shared__ float sm[];
  const int in_c = A.in_c, hid = A.hid, D = A.D;
  float* xs = sm;                        // [TS][in_c]
  float* dxs = xs + TS * in_c;           // [TS][in_c]
  float* h1s = dxs + TS * in_c;          // [TS][128]
  float* h2s = h1s + TS * 128;
  float* d2s = h2s + TS * 128;
  float* d1s = d2s + TS * 128;
  float* dps = d1s + TS * 128;           // [TS][4]
  const int tid = threadIdx.x;
  const int64_t m0 = (int64_t)blockIdx.x * TS;
  const int ns = (int)((A.M - m0) < TS ? (A.M - m0) : TS);
  const int fbs = D + 3, fbc = fbs + D * A.fea_pe, vbs = fbc + D * A.fea_pe, vbc = vbs + 3 * A.view_pe;
  // ---- x (tensorBase.py:68-75) ----
  for (int e = tid; e < TS * in_c; e += 128) {
    const int s = e / in_c, k = e % in_c;
    float val = 0.f;
    if (s < ns) {
      const int64_t m = m0 + s;
      if (k < D) val = A.feat[m * D + k];
      else if (k < fbs) val = A.dirs[m * 3 + (k - D)];
      else if (k < vbs) {
        const bool cosine = k >= fbc;
        const int j = k - (cosine ? fbc : fbs), f = j / A.fea_pe, q = j % A.fea_pe;
        const float arg = __fmul_rn(A.feat[m * D + f], (float)(1 << q));
        val = cosine ? cosf(arg) : sinf(arg);
      } else {
        const bool cosine = k >= vbc;
        const int j = k - (cosine ? vbc : vbs), d = j / A.view_pe, q = j % A.view_pe;
        const float arg = __fmul_rn(A.dirs[m * 3 + d], (float)(1 << q));
        val = cosine ? cosf(arg) : sinf(arg);
      }
    }
    xs[e] = val;
  }
  __syncthreads();
  for (int e = tid; e < TS * A.ldx; e += 128) {
    const int s = e / A.ldx, k = e % A.ldx;
    if (s < ns) A.X[(m0 + s) * A.ldx + k] = k < in_c ? xs[s * in_c + k] : 0.f;
  }
  // ---- h1 = relu(W1 x + b1), h2 = relu(W2 h1 + b2) ----
  const int j = tid;
  float acc[TS];
  if (j < hid) {
#pragma unroll
    for (int s = 0; s < TS; ++s) acc[s] = A.b1[j];
    const float* wr = A.w1 + (int64_t)j * in_c;
    for (int k = 0; k < in_c; ++k) {
      const float w = wr[k];
#pragma unroll
      for (int s = 0; s < TS; ++s) acc[s] = fmaf(w, xs[s * in_c + k], acc[s]);
    }
#pragma unroll
    for (int s = 0; s < TS; ++s) h1s[s * 128 + j] = fmaxf(acc[s], 0.f);
  }
  __syncthreads();
  if (j < hid) {
#pragma unroll
    for (int s = 0; s < TS; ++s) acc[s] = A.b2[j];
    const float* wr = A.w2 + (int64_t)j * hid;
    for (int k = 0; k < hid; ++k) {
      const float w = wr[k];
#pragma unroll
      for (int s = 0; s < TS; ++s) acc[s] = fmaf(w, h1s[s * 128 + k], acc[s]);
    }
#pragma unroll
    for (int s = 0; s < TS; ++s) h2s[s * 128 + j] = fmaxf(acc[s], 0.f);
  }
  __syncthreads();
  // ---- rgb = sigmoid(W3 h2 + b3): d(pre) = g y (1 - y) ----
  if (tid < TS * 3) {
    const int s = tid / 3, o = tid % 3;
    float pre = A.b3[o];
    for (int k = 0; k < hid; ++k) pre = fmaf(A.w3[o * hid + k], h2s[s * 128 + k], pre);
    const float y = 1.0f / (1.0f + expf(-pre));
    dps[s * 4 + o] = s < ns ? A.g[(m0 + s) * 3 + o] * ((1.0f - y) * y) : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < TS * LD; e += 128) {
    const int s = e / LD, k = e % LD;
    if (s < ns) {
      A.H1[(m0 + s) * LD + k] = k < hid ? h1s[s * 128 + k] : 0.f;
      A.H2[(m0 + s) * LD + k] = k < hid ? h2s[s * 128 + k] : 0.f;
    }
  }
  if (tid < TS * 3) {
    const int s = tid / 3, o = tid % 3;
    if (s < ns) A.DP[(m0 + s) * 3 + o] = dps[s * 4 + o];
  }
  // ---- dh2 = relu'(h2) W3^T d(pre); dh1 = relu'(h1) W2^T dh2 ----
  if (j < hid) {
#pragma unroll
    for (int s = 0; s < TS; ++s) {
      float d = 0.f;
      for (int o = 0; o < 3; ++o) d = fmaf(A.w3[o * hid + j], dps[s * 4 + o], d);
      d2s[s * 128 + j] = h2s[s * 128 + j] > 0.f ? d : 0.f;
    }
  }
  __syncthreads();
  if (j < hid) {
#pragma unroll
    for (int s = 0; s < TS; ++s) acc[s] = 0.f;
    for (int i = 0; i < hid; ++i) {
      const float w = A.w2[(int64_t)i * hid + j];
#pragma unroll
      for (int s = 0; s < TS; ++s) acc[s] = fmaf(w, d2s[s * 128 + i], acc[s]);
    }
#pragma unroll
    for (int s = 0; s < TS; ++s) d1s[s * 128 + j] = h1s[s * 128 + j] > 0.f ? acc[s] : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < TS * hid; e += 128) {
    const int s = e / hid, k = e % hid;
    if (s < ns) {
      A.DH2[(m0 + s) * hid + k] = d2s[s * 128 + k];
      A.DH1[(m0 + s) * hid + k] = d1s[s * 128 + k];
    }
  }
  // ---- dx = W1^T dh1 ----
  for (int k = tid; k < in_c; k += 128) {
    float a[TS];
#pragma unroll
    for (int s = 0; s < TS; ++s) a[s] = 0.f;
    for (int i = 0; i < hid; ++i) {
      const float w = A.w1[(int64_t)i * in_c + k];
#pragma unroll
      for (int s = 0; s < TS; ++s) a[s] = fmaf(w, d1s[s * 128 + i], a[s]);
    }
#pragma unroll
    for (int s = 0; s < TS; ++s) dxs[s * in_c + k] = a[s];
  }
  __syncthreads();
  // ---- through the encodings: d sin(2^q u) / du = 2^q cos(2^q u), d cos(2^q u) / du = -2^q sin(2^q u) ----
  for (int e = tid; e < TS * (D + 3); e += 128) {
    const int s = e / (D + 3), c = e % (D + 3);
    if (s >= ns) continue;
    const float* xr = xs + s * in_c;
    const float* dr = dxs + s * in_c;
    float d = dr[c];
    if (c < D) {
      for (int q = 0; q < A.fea_pe; ++q) {
        const int ks = fbs + c * A.fea_pe + q, kc = fbc + c * A.fea_pe + q;
        d = fmaf((float)(1 << q), dr[ks] * xr[kc] - dr[kc] * xr[ks], d);
      }
      if (A.d_feat) A.d_feat[(m0 + s) * D + c] = d;
    } else {
      const int dd = c - D;
      for (int q = 0; q < A.view_pe; ++q) {
        const int ks = vbs + dd * A.view_pe + q, kc = vbc + dd * A.view_pe + q;
        d = fmaf((float)(1 << q), dr[ks] * xr[kc] - dr[kc] * xr[ks], d);
      }
      if (A.d_dirs) A.d_dirs[(m0 + s) * 3 + dd] = d;
    }
  }
}

// SHRender backward (sh.py:87-112 degree 2, tensorBase.py:30-34): relu' from the recomputed output, d f[9c + k] = g_c Y_k, d dir = sum_c g_c
// sum_k f[9c + k] dY_k / d dir
__global__ void k_sh_render_bwd(const float* __restrict__ dirs, const float* __restrict__ feat, const float* __restrict__ g, int64_t M,
                                float* __restrict__ d_dirs, float* __restrict__ d_feat) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const float x = dirs[i * 3], y = dirs[i * 3 + 1], z = dirs[i * 3 + 2];
  const float xx = __fmul_rn(x, x), yy = __fmul_rn(y, y), zz = __fmul_rn(z, z);
  const float xy = __fmul_rn(x, y), yz = __fmul_rn(y, z), xz = __fmul_rn(x, z);
  const float C0 = 0.28209479177387814f, C1 = 0.4886025119029199f, C20 = 1.0925484305920792f, C21 = -1.0925484305920792f,
              C22 = 0.31539156525252005f, C23 = -1.0925484305920792f, C24 = 0.5462742152960396f;
  float Y[9];
  Y[0] = C0;
  Y[1] = __fmul_rn(-C1, y);
  Y[2] = __fmul_rn(C1, z);
  Y[3] = __fmul_rn(-C1, x);
  Y[4] = __fmul_rn(C20, xy);
  Y[5] = __fmul_rn(C21, yz);
  Y[6] = __fmul_rn(C22, __fsub_rn(__fsub_rn(__fmul_rn(2.0f, zz), xx), yy));
  Y[7] = __fmul_rn(C23, xz);
  Y[8] = __fmul_rn(C24, __fsub_rn(xx, yy));
  // dY_k / d(x, y, z)
  const float dYx[9] = {0.f, 0.f, 0.f, -C1, C20 * y, 0.f, -2.f * C22 * x, C23 * z, 2.f * C24 * x};
  const float dYy[9] = {0.f, -C1, 0.f, 0.f, C20 * x, C21 * z, -2.f * C22 * y, 0.f, -2.f * C24 * y};
  const float dYz[9] = {0.f, 0.f, C1, 0.f, 0.f, C21 * y, 4.f * C22 * z, C23 * x, 0.f};
  const float* f = feat + i * 27;
  float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) s = __fadd_rn(s, __fmul_rn(Y[k], f[9 * c + k]));
    const float gc = fmaxf(__fadd_rn(s, 0.5f), 0.f) > 0.f ? g[i * 3 + c] : 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      if (d_feat) d_feat[i * 27 + 9 * c + k] = gc * Y[k];
      gx = fmaf(gc * f[9 * c + k], dYx[k], gx);
      gy = fmaf(gc * f[9 * c + k], dYy[k], gy);
      gz = fmaf(gc * f[9 * c + k], dYz[k], gz);
    }
  }
  if (d_dirs) { d_dirs[i * 3] = gx; d_dirs[i * 3 + 1] = gy; d_dirs[i * 3 + 2] = gz; }
}

// feature2density backward: softplus(f + shift) as torch differentiates it (threshold 20: slope 1 above, z / (z + 1) with z = exp(x) below)
// or relu (slope 1 where the output is positive)
__global__ void k_feature2density_bwd(const float* __restrict__ feat, const float* __restrict__ g, int64_t M, int softplus, float shift,
                                      float* __restrict__ d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const float f = feat[i];
  float slope;
  if (softplus) {
    const float x = __fadd_rn(f, shift);
    const float z = expf(x);
    slope = x > 20.0f ? 1.0f : z / (z + 1.0f);
  } else {
    slope = relu_f(f) > 0.f ? 1.0f : 0.0f;
  }
  d[i] = g[i] * slope;
}

// raw2alpha backward, thread = ray.  a_j = 1 - alpha_j + 1e-10, T_i = prod_{j < i} a_j, weight_i = alpha_i T_i, bg = T_S.  The cumprod's
// backward as a reverse scan without division: R_i = sum_{k > i} g_w[k] alpha_k prod_{i < j < k} a_j + g_bg prod_{j > i} a_j satisfies
// R_{i-1} = g_w[i] alpha_i + a_i R_i, and dL/d alpha_i = g_alpha[i] + g_w[i] T_i - T_i R_i (exact where an a_j underflows to 0).  T_i is
// parked in d_sigma by a forward pass first.  alpha = 1 - exp(-sigma dist): d alpha = exp(-sigma dist) (dist d sigma + sigma d dist).
__global__ void k_raw2alpha_bwd(const float* __restrict__ sigma, const float* __restrict__ dist, const float* __restrict__ alpha,
                                const float* __restrict__ g_alpha, const float* __restrict__ g_w, const float* __restrict__ g_bg,
                                int64_t N, int S, float* __restrict__ d_sigma, float* __restrict__ d_dist) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= N) return;
  const int64_t o = r * S;
  float T = 1.f;
  for (int i = 0; i < S; ++i) {
    d_sigma[o + i] = T;
    T *= __fadd_rn(__fsub_rn(1.f, alpha[o + i]), 1e-10f);
  }
  float R = g_bg ? g_bg[r] : 0.f;
  for (int i = S - 1; i >= 0; --i) {
    const float Ti = d_sigma[o + i], a = alpha[o + i];
    const float gw = g_w ? g_w[o + i] : 0.f;
    const float da = (g_alpha ? g_alpha[o + i] : 0.f) + gw * Ti - Ti * R;
    R = fmaf(__fadd_rn(__fsub_rn(1.f, a), 1e-10f), R, gw * a);
    const float s = sigma[o + i], d = dist[o + i];
    const float e = expf(-(s * d));
    d_sigma[o + i] = da * d * e;
    d_dist[o + i] = da * s * e;
  }
}

int64_t table_floats(const ego_vm_field& f, int plane, int i) {
  return plane ? vm_plane_elems(f.res, f.n_comp, i) : vm_line_elems(f.res, f.n_comp, i);
}

int zero_grad(const ego_vm_field& f, const ego_vm_grad* g, hipStream_t st) {
  for (int gr = 0; gr < 2; ++gr)
    for (int i = 0; i < 3; ++i) {
      if (hipMemsetAsync(g->plane[gr][i], 0, (size_t)table_floats(f, 1, i) * 4, st) != hipSuccess ||
          hipMemsetAsync(g->line[gr][i], 0, (size_t)table_floats(f, 0, i) * 4, st) != hipSuccess)
        return ego_fail(EGO_E_BADARG, "stage backward: zero fill of a gradient table failed");
    }
  return EGO_OK;
}

// all tables, a component count of the any-shape envelope, resolutions >= 2 (the refusals are the callers': EGO_E_BADARG, their words)
bool field_complete(const ego_vm_field& f) { return vm_field_fault(f, false, true) == 0; }

// the sorted (bit-reproducible) walks serve the shipped table shapes
bool density_sorted(const ego_scene* sc, int64_t M, int32_t coarse) { return !coarse && sc->density.n_comp == 16 && M < (1ll << 31); }
bool app_sorted(const ego_scene* sc, int64_t M) { return sc->app.n_comp == 48 && (M + 31) / 32 * 32 * 144 < (1ll << 30); }

struct DensityWs { int64_t coords, sort, sort_bytes, coarse[12], total; };
DensityWs density_ws(const ego_scene* sc, int64_t M, int32_t coarse) {
  DensityWs w{};
  int64_t o = 0;
  w.coords = o; o += al256(M * 16);
  w.sort = o; w.sort_bytes = 0;
  if (density_sorted(sc, M, coarse)) { w.sort_bytes = ego_scatter_sorted_workspace_bytes(sc, M > 0 ? M : 1, 1); o += al256(w.sort_bytes); }
  for (int t = 0; t < 12; ++t) {
    w.coarse[t] = o;
    if (coarse) o += al256(table_floats(sc->density_coarse, t % 6 < 3, t % 3) * 4);
  }
  w.total = o;
  return w;
}

struct AppWs { int64_t coords, sort, sort_bytes, v, g64, dv, partial, total; };
AppWs app_ws(const ego_scene* sc, int64_t M) {
  AppWs w{};
  int64_t o = 0;
  const int64_t Mp = (M + 31) / 32 * 32;
  w.coords = o; o += al256(M * 16);
  w.sort = o; w.sort_bytes = 0;
  if (app_sorted(sc, M)) { w.sort_bytes = ego_scatter_sorted_workspace_bytes(sc, M > 0 ? M : 1, 1); o += al256(w.sort_bytes); }
  w.v = o; o += al256(M * LD * 4);
  w.g64 = o; o += al256(M * 64 * 4);
  w.dv = o; o += al256((app_sorted(sc, M) ? Mp * 144 : M * LD) * 4);
  w.partial = o; o += al256(ego_weight_grad_partial_floats() * 4);
  w.total = o;
  return w;
}

int mlp_ldx(const ego_scene* sc) { return (sc->mlp_in + 1 + LD - 1) / LD * LD; }
struct MlpWs { int64_t X, H1, H2, DH1, DH2, DP, partial, total; };
MlpWs mlp_ws(const ego_scene* sc, int64_t M) {
  MlpWs w{};
  int64_t o = 0;
  w.X = o; o += al256(M * mlp_ldx(sc) * 4);
  w.H1 = o; o += al256(M * LD * 4);
  w.H2 = o; o += al256(M * LD * 4);
  w.DH1 = o; o += al256(M * sc->mlp_hidden * 4);
  w.DH2 = o; o += al256(M * sc->mlp_hidden * 4);
  w.DP = o; o += al256(M * 3 * 4);
  w.partial = o; o += al256(ego_weight_grad_partial_floats() * 4);
  w.total = o;
  return w;
}

int check_density(const ego_scene* sc, int64_t M, int32_t coarse, const char* who) {
  if (!sc) return ego_fail(EGO_E_BADARG, "%s: null scene", who);
  if (M < 0 || M >= (1ll << 31)) return ego_fail(EGO_E_BADARG, "%s: bad size (0 <= M < 2^31)", who);
  if (!field_complete(sc->density) || (coarse && !field_complete(sc->density_coarse)))
    return ego_fail(EGO_E_BADARG, "%s: incomplete density field (tables, n_comp a multiple of 4 up to 48, res >= 2)", who);
  return EGO_OK;
}

int check_app(const ego_scene* sc, int64_t M, const char* who) {
  if (!sc) return ego_fail(EGO_E_BADARG, "%s: null scene", who);
  if (M < 0 || M >= (1ll << 31)) return ego_fail(EGO_E_BADARG, "%s: bad size (0 <= M < 2^31)", who);
  if (!field_complete(sc->app) || !sc->basis[0] || !sc->basis[1] || sc->app_dim < 1 || sc->app_dim > 32)
    return ego_fail(EGO_E_BADARG, "%s: incomplete appearance field / basis (app_dim 1..32)", who);
  return EGO_OK;
}

int check_mlp(const ego_scene* sc, int64_t M, const char* who) {
  if (!sc) return ego_fail(EGO_E_BADARG, "%s: null scene", who);
  if (M < 0 || M >= (1ll << 31)) return ego_fail(EGO_E_BADARG, "%s: bad size (0 <= M < 2^31)", who);
  if (sc->head != EGO_HEAD_MLP_FEA) return ego_fail(EGO_E_BADARG, "%s: the scene has no MLP head", who);
  if (int e = check_head_shape(sc, who, EGO_E_BADARG)) return e;
  for (int l = 0; l < 3; ++l)
    if (!sc->mlp_w[l] || !sc->mlp_b[l]) return ego_fail(EGO_E_BADARG, "%s: null MLP weight", who);
  return EGO_OK;
}

}  // namespace

extern "C" {

int64_t ego_density_feature_backward_workspace_bytes(const ego_scene* sc, int64_t M, int32_t coarse) {
  if (check_density(sc, M, coarse, "density_feature_backward_workspace_bytes")) return -1;
  return density_ws(sc, M, coarse).total;
}

int ego_density_feature_backward(const ego_scene* sc, const float* c7n, int64_t M, int32_t coarse, const float* g, const ego_vm_grad* gdensity,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  EGO_TRACE("ego_density_feature_backward");
  if (int e = check_density(sc, M, coarse, "density_feature_backward")) return e;
  EGO_REQUIRE(gdensity && vm_tables_complete(*gdensity), "density_feature_backward: null gradient table");
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) return zero_grad(sc->density, gdensity, st);
  EGO_REQUIRE(c7n && g && workspace && ((uintptr_t)workspace & 255) == 0, "density_feature_backward: null argument or workspace not 256-byte aligned");
  const DensityWs W = density_ws(sc, M, coarse);
  if (workspace_bytes < W.total)
    return ego_fail(EGO_E_BADARG, "density_feature_backward: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)W.total);
  char* base = (char*)workspace;
  float* coords = (float*)(base + W.coords);
  k_c7n_to_coords<<<nblk(M, 256), 256, 0, st>>>(c7n, M, coords);
  if (int e = ego_launch_status("k_c7n_to_coords")) return e;
  if (!coarse) {
    if (density_sorted(sc, M, coarse)) {
      if (int e = ego_scatter_sort(sc, coords, M, 1, base + W.sort, W.sort_bytes, stream)) return e;
      return ego_scatter_density_sorted(sc, gdensity, coords, g, M, 1, base + W.sort, W.sort_bytes, stream);
    }
    if (int e = zero_grad(sc->density, gdensity, st)) return e;
    return ego_scatter_generic(&sc->density, gdensity, coords, g, 0, M, 1, stream);
  }
  // coarse: the pooled tables' gradient first (scratch at the pooled resolution), then the pooling's backward into the full tables
  ego_vm_grad gc;
  for (int t = 0; t < 12; ++t) (t % 6 < 3 ? gc.plane : gc.line)[t / 6][t % 3] = (float*)(base + W.coarse[t]);
  if (int e = zero_grad(sc->density_coarse, &gc, st)) return e;
  if (int e = ego_scatter_generic(&sc->density_coarse, &gc, coords, g, 0, M, 1, stream)) return e;
  const ego_vm_field& F = sc->density;
  for (int t = 0; t < 12; ++t) {
    const bool plane = t % 6 < 3;
    const int gr = t / 6, i = t % 3;
    const int H = plane ? F.res[vm_plane_y(i)] : F.res[vm_line_ax(i)], Wd = plane ? F.res[vm_plane_x(i)] : 1;
    const int Hc = plane ? sc->density_coarse.res[vm_plane_y(i)] : sc->density_coarse.res[vm_line_ax(i)];
    const int Wc = plane ? sc->density_coarse.res[vm_plane_x(i)] : 1;
    EGO_REQUIRE(Hc == H / 2 && Wc == (plane ? Wd / 2 : 1), "density_feature_backward: density_coarse.res must be density.res / 2");
    const int64_t n = (int64_t)H * Wd * F.n_comp;
    float* dst = plane ? gdensity->plane[gr][i] : gdensity->line[gr][i];
    k_avgpool_backward<<<(unsigned)std::min<int64_t>((n + 255) / 256, 8192), 256, 0, st>>>(plane ? gc.plane[gr][i] : gc.line[gr][i], H, Wd,
                                                                                          F.n_comp, dst);
    if (int e = ego_launch_status("k_avgpool_backward")) return e;
  }
  return EGO_OK;
}

int64_t ego_app_feature_backward_workspace_bytes(const ego_scene* sc, int64_t M) {
  if (check_app(sc, M, "app_feature_backward_workspace_bytes")) return -1;
  return app_ws(sc, M).total;
}

int ego_app_feature_backward(const ego_scene* sc, const float* c7n, int64_t M, const float* g, const ego_vm_grad* gapp, float* gbasis, int32_t ldg,
                             void* workspace, int64_t workspace_bytes, void* stream) {
  EGO_TRACE("ego_app_feature_backward");
  if (int e = check_app(sc, M, "app_feature_backward")) return e;
  EGO_REQUIRE(gapp && vm_tables_complete(*gapp) && gbasis && ldg >= LD, "app_feature_backward: null gradient output or ldg < 160");
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) {
    if (hipMemsetAsync(gbasis, 0, (size_t)64 * ldg * 4, st) != hipSuccess) return ego_fail(EGO_E_BADARG, "app_feature_backward: zero fill failed");
    return zero_grad(sc->app, gapp, st);
  }
  EGO_REQUIRE(c7n && g && workspace && ((uintptr_t)workspace & 255) == 0, "app_feature_backward: null argument or workspace not 256-byte aligned");
  const AppWs W = app_ws(sc, M);
  if (workspace_bytes < W.total)
    return ego_fail(EGO_E_BADARG, "app_feature_backward: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)W.total);
  char* base = (char*)workspace;
  float *coords = (float*)(base + W.coords), *v = (float*)(base + W.v), *g64 = (float*)(base + W.g64), *dv = (float*)(base + W.dv);
  const bool sorted = app_sorted(sc, M);
  const int D = sc->app_dim, ncol = 3 * sc->app.n_comp;
  k_app_bwd_prep<<<nblk((M + 31) / 32 * 32, 256), 256, (size_t)2 * D * ncol * 4, st>>>(make_field(sc->app), sc->basis[0], sc->basis[1], c7n, g, M, D, sc->app.n_comp, coords, v,
                                                                       g64, dv, sorted ? 1 : 0);
  if (int e = ego_launch_status("k_app_bwd_prep")) return e;
  if (sorted) {
    if (int e = ego_scatter_sort(sc, coords, M, 1, base + W.sort, W.sort_bytes, stream)) return e;
    if (int e = ego_scatter_app_sorted(sc, gapp, coords, dv, nullptr, nullptr, nullptr, 0, M, 1, base + W.sort, W.sort_bytes, stream)) return e;
  } else {
    if (int e = zero_grad(sc->app, gapp, st)) return e;
    if (int e = ego_scatter_generic(&sc->app, gapp, coords, dv, LD, M, 1, stream)) return e;
  }
  // d(basis_g) = g_g^T v over the grid's samples: rows 32 g + slot of gbasis
  return ego_weight_grad_det(g64, 64, 64, 0, nullptr, v, LD, LD, 0, -1, M, gbasis, ldg, (float*)(base + W.partial), ego_weight_grad_partial_floats(),
                             stream);
}

int64_t ego_mlp_fea_backward_workspace_bytes(const ego_scene* sc, int64_t M) {
  if (check_mlp(sc, M, "mlp_fea_backward_workspace_bytes")) return -1;
  return mlp_ws(sc, M).total;
}

int ego_mlp_fea_backward(const ego_scene* sc, const float* viewdirs, const float* feat, int64_t M, const float* g_rgb, float* d_feat, float* d_viewdirs,
                         float* g1, int32_t ld1, float* g2, int32_t ld2, float* g3, int32_t ld3, void* workspace, int64_t workspace_bytes,
                         void* stream) {
  EGO_TRACE("ego_mlp_fea_backward");
  if (int e = check_mlp(sc, M, "mlp_fea_backward")) return e;
  const int hid = sc->mlp_hidden, ldx = mlp_ldx(sc);
  EGO_REQUIRE(g1 && g2 && g3 && ld1 >= ldx && ld2 >= LD && ld3 >= LD, "mlp_fea_backward: null weight-gradient output or leading dimension too small");
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) {
    if (hipMemsetAsync(g1, 0, (size_t)hid * ld1 * 4, st) != hipSuccess || hipMemsetAsync(g2, 0, (size_t)hid * ld2 * 4, st) != hipSuccess ||
        hipMemsetAsync(g3, 0, (size_t)32 * ld3 * 4, st) != hipSuccess)
      return ego_fail(EGO_E_BADARG, "mlp_fea_backward: zero fill failed");
    return EGO_OK;
  }
  EGO_REQUIRE(viewdirs && feat && g_rgb && workspace && ((uintptr_t)workspace & 255) == 0,
              "mlp_fea_backward: null argument or workspace not 256-byte aligned");
  const MlpWs W = mlp_ws(sc, M);
  if (workspace_bytes < W.total)
    return ego_fail(EGO_E_BADARG, "mlp_fea_backward: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)W.total);
  char* base = (char*)workspace;
  MlpArgs a;
  a.w1 = sc->mlp_w[0]; a.b1 = sc->mlp_b[0]; a.w2 = sc->mlp_w[1]; a.b2 = sc->mlp_b[1]; a.w3 = sc->mlp_w[2]; a.b3 = sc->mlp_b[2];
  a.dirs = viewdirs; a.feat = feat; a.g = g_rgb; a.d_feat = d_feat; a.d_dirs = d_viewdirs;
  a.X = (float*)(base + W.X); a.H1 = (float*)(base + W.H1); a.H2 = (float*)(base + W.H2);
  a.DH1 = (float*)(base + W.DH1); a.DH2 = (float*)(base + W.DH2); a.DP = (float*)(base + W.DP);
  a.M = M; a.D = sc->app_dim; a.in_c = sc->mlp_in; a.hid = hid; a.view_pe = sc->view_pe; a.fea_pe = sc->fea_pe; a.ldx = ldx;
  const size_t lds16 = ((size_t)2 * 16 * a.in_c + 4 * 16 * 128 + 16 * 4) * 4;
  if (lds16 <= 64 * 1024) {
    k_mlp_bwd<16><<<nblk(M, 16), 128, lds16, st>>>(a);
  } else {
    const size_t lds8 = ((size_t)2 * 8 * a.in_c + 4 * 8 * 128 + 8 * 4) * 4;
    k_mlp_bwd<8><<<nblk(M, 8), 128, lds8, st>>>(a);
  }
  if (int e = ego_launch_status("k_mlp_bwd")) return e;
  float* part = (float*)(base + W.partial);
  const int64_t pf = ego_weight_grad_partial_floats();
  // d(W3 | b3) = d(pre)^T [h2 | 1], d(W2 | b2) = dh2^T [h1 | 1], d(W1 | b1) = dh1^T [x | 1] in 160-column blocks
  if (int e = ego_weight_grad_det(a.DP, 3, 3, 0, nullptr, a.H2, LD, LD, 0, hid, M, g3, ld3, part, pf, stream)) return e;
  if (int e = ego_weight_grad_det(a.DH2, hid, hid, 0, nullptr, a.H1, LD, LD, 0, hid, M, g2, ld2, part, pf, stream)) return e;
  for (int c0 = 0; c0 < ldx; c0 += LD) {
    const int ones = (c0 <= sc->mlp_in && sc->mlp_in < c0 + LD) ? sc->mlp_in - c0 : -1;
    if (int e = ego_weight_grad_det(a.DH1, hid, hid, 0, nullptr, a.X + c0, ldx, LD, 0, ones, M, g1 + c0, ld1, part, pf, stream)) return e;
  }
  return EGO_OK;
}

int ego_sh_render_backward(const float* viewdirs, const float* features, int64_t M, const float* g_rgb, float* d_viewdirs, float* d_features,
                           void* stream) {
  EGO_TRACE("ego_sh_render_backward");
  EGO_REQUIRE(M >= 0, "sh_render_backward: M < 0");
  if (M == 0) return EGO_OK;
  EGO_REQUIRE(viewdirs && features && g_rgb && (d_viewdirs || d_features), "sh_render_backward: null argument");
  k_sh_render_bwd<<<nblk(M, 256), 256, 0, (hipStream_t)stream>>>(viewdirs, features, g_rgb, M, d_viewdirs, d_features);
  return ego_launch_status("k_sh_render_bwd");
}

int ego_feature2density_backward(const ego_scene* sc, const float* feat, int64_t M, const float* g, float* d_feat, void* stream) {
  EGO_TRACE("ego_feature2density_backward");
  EGO_REQUIRE(M >= 0, "feature2density_backward: M < 0");
  if (M == 0) return EGO_OK;
  EGO_REQUIRE(sc && feat && g && d_feat, "feature2density_backward: null argument");
  k_feature2density_bwd<<<nblk(M, 256), 256, 0, (hipStream_t)stream>>>(feat, g, M, sc->act_softplus, sc->density_shift, d_feat);
  return ego_launch_status("k_feature2density_bwd");
}

int ego_raw2alpha_backward(const float* sigma, const float* dist, const float* alpha, int64_t N, int32_t S, const float* g_alpha, const float* g_weight,
                           const float* g_bg, float* d_sigma, float* d_dist, void* stream) {
  EGO_TRACE("ego_raw2alpha_backward");
  EGO_REQUIRE(N >= 0 && S >= 1, "raw2alpha_backward: bad size");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(sigma && dist && alpha && d_sigma && d_dist, "raw2alpha_backward: null argument");
  k_raw2alpha_bwd<<<nblk(N, 64), 64, 0, (hipStream_t)stream>>>(sigma, dist, alpha, g_alpha, g_weight, g_bg, N, S, d_sigma, d_dist);
  return ego_launch_status("k_raw2alpha_bwd");
}

}  // extern "C"
