// Training-step table ops of the EgoNeRF path that sit next to the render (train.py:245-330): the TV / L1 / ortho
// regularisers with their gradients fused into the same pass, the ray-entropy loss, the distortion regulariser and the depth term (per
// ray, through alpha like the entropy), coarse-to-fine table resampling and a multi-tensor Adam.  All tables are channel-last ([H][W][C] fp32),
// all kernels are HBM-bound streaming passes.
#include <stddef.h>

#include "ego_device.h"
#include "ego_host.h"

namespace {

__device__ __forceinline__ double block_sum_256(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  return red[0];
}

// utils.py:155-171 (TVLoss) on one plane, value and gradient in one pass.  ah = scale*2/count_h, aw = scale*2/count_w.
__global__ __launch_bounds__(256) void k_tv_plane(const float* __restrict__ x, int C, int H, int W, float ah, float aw,
                                                  double* __restrict__ value, float* __restrict__ grad) {
  __shared__ double red[256];
  const int64_t n = (int64_t)H * W * C;
  const int64_t rowstride = (int64_t)W * C;
  double part = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t pix = i / C;
    const int xx = (int)(pix % W), yy = (int)(pix / W);
    const float v = x[i];
    const float dh = (yy + 1 < H) ? x[i + rowstride] - v : 0.f;
    const float dw = (xx + 1 < W) ? x[i + C] - v : 0.f;
    part += (double)(dh * dh * ah + dw * dw * aw);
    if (grad) {
      const float bh = (yy > 0) ? v - x[i - rowstride] : 0.f;
      const float bw = (xx > 0) ? v - x[i - C] : 0.f;
      grad[i] += 2.f * (ah * (bh - dh) + aw * (bw - dw));
    }
  }
  const double tot = block_sum_256(part, red);
  if (threadIdx.x == 0 && value) atomicAdd(value, tot);
}

// EgoNeRF.py:206-212 (density_L1) on one table: value += scale * mean|x|, grad += scale * sign(x) / n
__global__ __launch_bounds__(256) void k_l1(const float* __restrict__ x, int64_t n, float a, double* __restrict__ value,
                                            float* __restrict__ grad) {
  __shared__ double red[256];
  double part = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = x[i];
    part += (double)fabsf(v);
    if (grad) grad[i] += a * (float)((v > 0.f) - (v < 0.f));
  }
  const double tot = block_sum_256(part, red);
  if (threadIdx.x == 0 && value) atomicAdd(value, tot * (double)a);
}

// EgoNeRF.py:189-201 (vectorDiffs) on one line table L [n][C]: G = L^T L, value += scale * mean |offdiag G|,
// grad[k][i] += scale * 2 / (C (C-1)) * sum_{j != i} sign(G_ij) L[k][j].  One workgroup per table.
__global__ __launch_bounds__(256) void k_line_ortho(const float* __restrict__ L, int C, int n, float scale,
                                                    double* __restrict__ value, float* __restrict__ grad) {
  __shared__ float G[64 * 64];
  __shared__ double red[256];
  const int tid = threadIdx.x;
  for (int e = tid; e < C * C; e += 256) {
    const int i = e / C, j = e % C;
    float acc = 0.f;
    for (int k = 0; k < n; ++k) acc += L[k * C + i] * L[k * C + j];
    G[e] = acc;
  }
  __syncthreads();
  double part = 0.0;
  for (int e = tid; e < C * C; e += 256)
    if (e / C != e % C) part += (double)fabsf(G[e]);
  const float a = scale / (float)(C * (C - 1));
  const double tot = block_sum_256(part, red);
  if (tid == 0 && value) atomicAdd(value, tot * (double)a);
  if (!grad) return;
  for (int e = tid; e < n * C; e += 256) {
    const int k = e / C, i = e % C;
    float acc = 0.f;
    for (int j = 0; j < C; ++j) {
      const float g = G[i * C + j];
      const float s = (j == i) ? 0.f : (float)((g > 0.f) - (g < 0.f));
      acc += s * L[k * C + j];
    }
    grad[e] += 2.f * a * acc;
  }
}

// utils.py:175-183 (ray_entropy_loss), one wave per ray: value += H_ray / N, g_alpha = dH/dalpha / N
__global__ __launch_bounds__(256) void k_ray_entropy(const float* __restrict__ alpha, int64_t N, int S, int stride,
                                                     double* __restrict__ value, float* __restrict__ g_alpha) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= N) return;
  const float* a = alpha + ray * stride;
  float sum = 0.f;
  for (int s = lane; s < S; s += 64) sum += a[s];
  const float A = wave_sum(sum) + 1e-10f;
  const float inv_ln2 = 1.44269504088896340736f;
  float ent = 0.f, ph = 0.f;
  for (int s = lane; s < S; s += 64) {
    const float p = a[s] / A;
    const float lg = log2f(p + 1e-10f);
    ent -= p * lg;
    ph += p * -(lg + p / (p + 1e-10f) * inv_ln2);
  }
  ent = wave_sum(ent);
  ph = wave_sum(ph);
  const float invN = 1.f / (float)N;
  if (g_alpha)
    for (int s = lane; s < S; s += 64) {
      const float p = a[s] / A;
      const float h = -(log2f(p + 1e-10f) + p / (p + 1e-10f) * inv_ln2);
      g_alpha[ray * stride + s] = (h - ph) / A * invN;
    }
  if (lane == 0 && value) atomicAdd(value, (double)ent * (double)invN);
}

// ---- Distortion regulariser (Mip-NeRF 360's, in the point-sampled form used with voxel-grid NeRFs; not in the reference) ----
// One ray with samples z_0 <= ... <= z_{S-1}.  Sample i covers [z_i, z_{i+1}], z_S = z_{S-1} + (z_{S-1} - z_{S-2}): the render's own
// quadrature (dist = diff(z), last repeated, EgoNeRF.py:517-518).  The S + 1 ends go through a monotone map to s in [0, 1]:
//   linear     s = (z - near) / (far - near)
//   log        s = log(max(z, near) / near) / log(far / near)            (the exponential schedule has equal widths here)
//   disparity  s = (1 / near - 1 / max(z, near)) / (1 / near - 1 / far)
// m_i = (s_i + s_{i+1}) / 2, delta_i = s_{i+1} - s_i (ties in z give delta = 0), and with the render's weights (tensorBase.py:22-27)
// w_i = alpha_i T_i, T_i = prod_{j<i} (1 - alpha_j + 1e-10):
//   loss = (1 / N) sum_rays [ sum_i sum_j w_i w_j |m_i - m_j| + (1 / 3) sum_i w_i^2 delta_i ]
// z is a constant (the fine z is detached, EgoNeRF.py:534); alpha is the only differentiable input.
//
// O(S): m ascends, so with W_{<i} = sum_{j<i} w_j, WM_{<i} = sum_{j<i} w_j m_j (and the same sums over j > i)
//   double sum = 2 sum_i w_i (m_i W_{<i} - WM_{<i})
//   G_i = dL / dw_i = 2 [ m_i (W_{<i} - W_{>i}) - (WM_{<i} - WM_{>i}) ] + (2 / 3) w_i delta_i
//   R_{S-1} = 0, R_i = G_{i+1} alpha_{i+1} + (1 - alpha_{i+1} + 1e-10) R_{i+1}            (k_raw2alpha_bwd's recurrence: no division,
//   g_alpha_i = T_i (G_i - R_i) / N                                                         so alpha = 1 is harmless)
// The differences of the running sums cancel when a ray's mass sits in neighbouring samples, so W, WM, m and delta are carried in
// float64 (w m is the product of two float32 values, exact in float64); T, the map and the R recurrence stay float32.
//
// One wave per ray, 64 samples per pass (lane = sample), wave scans with a carry between the passes.  The forward sweep produces T,
// the running sums, their totals and the value; with a gradient it parks T_i in g_alpha[i].  The reverse sweep re-reads alpha, z
// (cache) and the parked T, forms the sums over j >= i by a reverse scan, G, and R by a reverse scan of the affine maps
// x -> (1 - alpha_i + 1e-10) x + G_i alpha_i, and overwrites g_alpha.  Every sum has a fixed order: the gradient is bit-reproducible.
struct DistMap {
  int space;
  float near_, scale;  // scale = 1 / (far - near), 1 / log(far / near), 1 / (1 / near - 1 / far): rounded once from float64
};

__device__ __forceinline__ float dist_map(float z, const DistMap& g) {
  if (g.space == EGO_DIST_LINEAR) return (z - g.near_) * g.scale;
  const float zc = fmaxf(z, g.near_);
  if (g.space == EGO_DIST_LOG) return logf(zc / g.near_) * g.scale;
  return (1.f / g.near_ - 1.f / zc) * g.scale;
}

struct DistSample {
  float a, f;       // alpha_i, 1 - alpha_i + 1e-10 (0 and 1 beyond the ray's end: the identities of every scan below)
  double m, delta;
};

__device__ __forceinline__ DistSample dist_sample(const float* __restrict__ a_row, const float* __restrict__ z_row, float z_end, int i, int S,
                                                  const DistMap& g) {
  DistSample o;
  o.a = i < S ? a_row[i] : 0.f;
  o.f = __fadd_rn(__fsub_rn(1.f, o.a), 1e-10f);
  const double s0 = (double)dist_map(i < S ? z_row[i] : z_end, g), s1 = (double)dist_map(i + 1 < S ? z_row[i + 1] : z_end, g);
  o.m = 0.5 * (s0 + s1);
  o.delta = s1 - s0;
  return o;
}

// wave64 inclusive sums in lane order (scan_add: over lanes <= lane, rscan_add: over lanes >= lane), float64
__device__ __forceinline__ double wave_scan_add(double v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

__device__ __forceinline__ double wave_rscan_add(double v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_down(v, d, 64);
    if (lane + d < 64) v += o;
  }
  return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// One 64-sample pass of the recurrence R_{i-1} = A_i R_i + B_i (A = 1 - alpha + 1e-10, B = G alpha; 1 and 0 beyond the ray's end), passes
// taken from the ray's end: -> R_i of this lane's sample; cR carries R at the pass's last sample in and R in front of its first one out.
__device__ __forceinline__ float recurrence_pass(float A, float B, float& cR, int lane) {
  // lane i: the map R_i -> R_{i-1}; after the scan the composition of the maps of lanes i .. 63
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float Ao = __shfl_down(A, d, 64), Bo = __shfl_down(B, d, 64);
    if (lane + d < 64) {
      B = fmaf(A, Bo, B);
      A *= Ao;
    }
  }
  const float R_before = fmaf(A, cR, B);   // R_{i-1}
  float R = __shfl_down(R_before, 1, 64);
  if (lane == 63) R = cR;
  cR = __shfl(R_before, 0, 64);
  return R;
}

// One ray by one wave (all 64 lanes run every scan) -> the ray's term of the value; with g_row, the ray's gradient row is written.
__device__ __forceinline__ double dist_ray(const float* __restrict__ a_row, const float* __restrict__ z_row, float* __restrict__ g_row, int64_t N,
                                           int S, int stride, const DistMap& map, int lane) {
  const float z_end = z_row[S - 1] + (z_row[S - 1] - z_row[S - 2]);
  const int passes = (S + 63) >> 6;

  float cT = 1.f;               // carries: T, W_{<i}, WM_{<i} at the pass's first sample
  double cW = 0.0, cWM = 0.0, part = 0.0;
  for (int p = 0; p < passes; ++p) {
    const int i = p * 64 + lane;
    const DistSample s = dist_sample(a_row, z_row, z_end, i, S, map);
    const float prod = wave_scan_mul(s.f, lane);
    float before = __shfl_up(prod, 1, 64);
    if (lane == 0) before = 1.f;
    const float T = cT * before;
    cT *= __shfl(prod, 63, 64);
    const double w = (double)(s.a * T), wm = w * s.m;
    const double W = cW + wave_scan_add(w, lane), WM = cWM + wave_scan_add(wm, lane);   // over j <= i
    part += 2.0 * w * (s.m * (W - w) - (WM - wm)) + w * w * s.delta / 3.0;
    cW = __shfl(W, 63, 64);
    cWM = __shfl(WM, 63, 64);
    if (g_row && i < S) g_row[i] = T;
  }
  // The ray's term, rounded to a multiple of 2^-51.  With z in [near, far] the mapped ends stay within [0, 2] (z_S <= 2 far) and
  // sum w <= 1, so a ray's term is at most s_S - s_0 <= 2 and so is the total: below 4, up to which every sum of such multiples - a
  // block's, and the adds into the zeroed `value` - is exact.  The result then does not depend on the order in which the blocks arrive
  // (value-only, joint and repeated calls return the same bits); the rounding costs at most N 2^-52 absolute.
  const double invN = 1.0 / (double)N;
  const double term = rint(wave_sum_f64(part) * invN * 0x1p51) * 0x1p-51;
  if (!g_row) return term;

  const double Wt = cW, WMt = cWM;
  double cGeW = 0.0, cGeWM = 0.0;   // carries: the sums over the samples behind the pass, and R at the pass's last sample
  float cR = 0.f;
  for (int p = passes - 1; p >= 0; --p) {
    const int i = p * 64 + lane;
    const DistSample s = dist_sample(a_row, z_row, z_end, i, S, map);
    const float T = i < S ? g_row[i] : 0.f;
    const double w = (double)(s.a * T), wm = w * s.m;
    const double geW = cGeW + wave_rscan_add(w, lane), geWM = cGeWM + wave_rscan_add(wm, lane);   // over j >= i
    const double G64 = 2.0 * (s.m * ((Wt - geW) - (geW - w)) - ((WMt - geWM) - (geWM - wm))) + (2.0 / 3.0) * w * s.delta;
    cGeW = __shfl(geW, 0, 64);
    cGeWM = __shfl(geWM, 0, 64);
    const float G = (float)G64;
    const float R = recurrence_pass(s.f, G * s.a, cR, lane);
    if (i < S) g_row[i] = T * (G - R) * (float)invN;
  }
  for (int c = S + lane; c < stride; c += 64) g_row[c] = 0.f;
  return term;
}

// Four rays per block.  The adds into `value` all hit one address and serialise (12.5 ns each, measured: what the entropy kernel's
// time consists of), so the block's four terms are summed first and added once.
__global__ __launch_bounds__(256) void k_ray_distortion(const float* __restrict__ alpha, int stride, const float* __restrict__ z, int64_t N,
                                                        int S, DistMap map, double* __restrict__ value, float* __restrict__ g_alpha) {
  __shared__ double terms[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * 4 + wave;
  double term = 0.0;
  if (ray < N)   // wave-uniform
    term = dist_ray(alpha + ray * stride, z + ray * S, g_alpha ? g_alpha + ray * stride : nullptr, N, S, stride, map, lane);
  if (!value) return;
  if (lane == 0) terms[wave] = term;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(value, (terms[0] + terms[1]) + (terms[2] + terms[3]));
}

// ---- Depth supervision (train.py:249-251, :275-283: a masked MSE between depth_map and a per-ray target, rays with target 0 left out) ----
// The reference computes depth_map under no_grad (EgoNeRF.py:595-598), so its term has no gradient; this is the term that loop means.
// The render's depth output stays non-differentiable: the loss enters through alpha, like the entropy and the distortion terms.  With
// the render's weights w_i = alpha_i T_i, T_i = prod_{j<i} f_j, f_j = 1 - alpha_j + 1e-10, the mapped distances q_i = s(z_i) and the
// mapped tail q_t = s(tail) (0 without one):
//   D       = sum_i w_i q_i + (1 - sum_i w_i) q_t                   (both sums in float64; w q is exact there)
//   G_i     = dD / dw_i = q_i - q_t
//   R_{S-1} = 0, R_i = G_{i+1} alpha_{i+1} + f_{i+1} R_{i+1}        (the distortion kernel's recurrence: no division)
//   dD / dalpha_i = T_i (G_i - R_i)
// A ray is valid iff its target is finite and > 0; V = the number of valid rays, r = D - s(target):
//   l2: loss = (1 / V) sum_valid r^2,  g_alpha_i = (2 r / V) dD / dalpha_i        l1: |r| and sign(r) (0 at r = 0) in their places
// An invalid ray adds nothing and its gradient row is 0; with V = 0 the value and every gradient element are 0.
//
// Three launches, no host synchronisation: k_depth_count leaves V in the workspace; k_ray_depth_loss (one wave per ray, four rays per
// block, 64 samples per pass like k_ray_distortion) writes pred = D, the ray's r^2 or |r| into the workspace and the gradient row:
// the forward sweep keeps per-lane float64 partial sums over the passes and parks T_i in g_alpha[i], the reverse sweep runs the affine
// scan for R and overwrites it; k_depth_reduce sums the rays' terms in a fixed order and divides by V.  r^2 reaches far^2, so the
// distortion kernel's rounding to multiples of 2^-51 (sums below 4) does not carry over: the order is fixed instead, and value-only,
// gradient-only, joint and repeated calls return the same bits.
__device__ __forceinline__ float depth_map(float z, const DistMap& g) { return g.space == EGO_DIST_METRIC ? z : dist_map(z, g); }

__device__ __forceinline__ bool depth_valid(float t) { return t > 0.f && t < INFINITY; }   // false for NaN

struct DepthWorkspace {
  unsigned long long valid;   // V
  unsigned long long pad;
  double term[1];             // [N]: r^2 or |r| of a valid ray, 0 of an invalid one
};

__global__ __launch_bounds__(1024) void k_depth_count(const float* __restrict__ target, int64_t N, DepthWorkspace* __restrict__ ws) {
  __shared__ unsigned long long total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  unsigned long long c = 0;
  for (int64_t i = threadIdx.x; i < N; i += 1024) c += depth_valid(target[i]) ? 1u : 0u;
  atomicAdd(&total, c);   // integers: any order gives the same sum
  __syncthreads();
  if (threadIdx.x == 0) ws->valid = total;
}

__global__ __launch_bounds__(256) void k_ray_depth_loss(const float* __restrict__ alpha, int stride, const float* __restrict__ z,
                                                        const float* __restrict__ target, const float* __restrict__ tail, int64_t N, int S,
                                                        DistMap map, int kind, DepthWorkspace* __restrict__ ws, float* __restrict__ g_alpha,
                                                        float* __restrict__ pred) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= N) return;   // wave-uniform
  const float* a_row = alpha + ray * stride;
  const float* z_row = z + ray * S;
  float* g_row = g_alpha ? g_alpha + ray * stride : nullptr;
  const float q_t = tail ? depth_map(tail[ray], map) : 0.f;
  const float tgt = target ? target[ray] : 0.f;
  const bool valid = depth_valid(tgt);
  const bool want_row = g_row && valid;   // an invalid ray's row is zeros: T need not be parked
  const int passes = (S + 63) >> 6;

  float cT = 1.f;   // carry: T at the pass's first sample
  double sw = 0.0, swq = 0.0;   // this lane's share of sum w, sum w q
  for (int p = 0; p < passes; ++p) {
    const int i = p * 64 + lane;
    const float a = i < S ? a_row[i] : 0.f;
    const float f = __fadd_rn(__fsub_rn(1.f, a), 1e-10f);
    const float q = i < S ? depth_map(z_row[i], map) : 0.f;
    const float prod = wave_scan_mul(f, lane);
    float before = __shfl_up(prod, 1, 64);
    if (lane == 0) before = 1.f;
    const float T = cT * before;
    cT *= __shfl(prod, 63, 64);
    const double w = (double)(a * T);
    sw += w;
    swq += w * (double)q;
    if (want_row && i < S) g_row[i] = T;
  }
  const double D = wave_sum_f64(swq) + (1.0 - wave_sum_f64(sw)) * (double)q_t;
  if (pred && lane == 0) pred[ray] = (float)D;
  if (!ws) return;   // pred only

  const double r = valid ? D - (double)depth_map(tgt, map) : 0.0;
  if (lane == 0) ws->term[ray] = kind == EGO_DEPTH_L2 ? r * r : fabs(r);
  if (!g_row) return;
  // d loss / d D; V >= 1 where a ray is valid
  const float scale = !valid ? 0.f : (float)((kind == EGO_DEPTH_L2 ? 2.0 * r : (double)((r > 0.0) - (r < 0.0))) / (double)ws->valid);
  if (scale == 0.f) {   // invalid, or r = 0: exactly 0
    for (int c = lane; c < stride; c += 64) g_row[c] = 0.f;
    return;
  }
  float cR = 0.f;   // carry: R at the pass's last sample
  for (int p = passes - 1; p >= 0; --p) {
    const int i = p * 64 + lane;
    const bool in = i < S;
    const float a = in ? a_row[i] : 0.f;
    const float f = __fadd_rn(__fsub_rn(1.f, a), 1e-10f);
    const float G = in ? depth_map(z_row[i], map) - q_t : 0.f;
    const float T = in ? g_row[i] : 0.f;
    const float R = recurrence_pass(f, G * a, cR, lane);
    if (in) g_row[i] = T * (G - R) * scale;
  }
  for (int c = S + lane; c < stride; c += 64) g_row[c] = 0.f;
}

// value += (1 / V) sum_rays term, the rays in a fixed order: thread t takes rays t, t + 256, ..., then block_sum_256's tree
__global__ __launch_bounds__(256) void k_depth_reduce(const DepthWorkspace* __restrict__ ws, int64_t N, double* __restrict__ value) {
  __shared__ double red[256];
  double part = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += 256) part += ws->term[i];
  const double tot = block_sum_256(part, red);
  if (threadIdx.x == 0 && ws->valid > 0) *value += tot / (double)ws->valid;
}

// coordinates.py:27-39 / :226-266: bilinear (align_corners, zero padding) resample of a channel-last table at per-axis
// normalised coordinates xs [W2], ys [H2]
__global__ void k_resample_table(const float* __restrict__ src, int C, int H, int W, const float* __restrict__ xs,
                                 const float* __restrict__ ys, int H2, int W2, float* __restrict__ dst) {
#pragma clang fp contract(fast)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)H2 * W2 * C) return;
  const int c = (int)(i % C);
  const int64_t pix = i / C;
  const int x2 = (int)(pix % W2), y2 = (int)(pix / W2);
  const Lin1 X = lin_setup(xs[x2], W), Y = lin_setup(ys[y2], H);
  const float* r0 = src + ((int64_t)Y.i0 * W) * C + c;
  const float* r1 = src + ((int64_t)Y.i1 * W) * C + c;
  dst[i] = (r0[(int64_t)X.i0 * C] * X.w0 + r0[(int64_t)X.i1 * C] * X.w1) * Y.w0 +
           (r1[(int64_t)X.i0 * C] * X.w0 + r1[(int64_t)X.i1 * C] * X.w1) * Y.w1;
}

// torch.optim.Adam (train.py:182, betas (0.9, 0.99)) over up to ADAM_MAX tensors per launch; 1024 elements per block
constexpr int ADAM_MAX = 40;
struct AdamBatch {
  float* p[ADAM_MAX];
  const float* g[ADAM_MAX];
  float* m[ADAM_MAX];
  float* v[ADAM_MAX];
  int64_t n[ADAM_MAX];
  int32_t chunk0[ADAM_MAX + 1];  // first block of each tensor
  float step_size[ADAM_MAX];     // lr / (1 - beta1^t)
  int32_t count;
  float beta1, beta2, eps, bc2_sqrt;
  const double* clock;           // optional device clock (ego_adam_step_graph): [2] = lr scale / (1 - beta1^t), [3] = sqrt(1 - beta2^t)
};

// The step count and the learning-rate scale live on the device, so that a captured hipGraph of the training step advances them
// by itself: clock = {t, lr scale, lr scale / (1 - beta1^t), sqrt(1 - beta2^t)}.  One thread, double precision like the host path.
__global__ void k_adam_clock(double* clock, double beta1, double beta2, double lr_factor) {
  const double t = clock[0] + 1.0;
  clock[0] = t;
  clock[2] = clock[1] / (1.0 - pow(beta1, t));
  clock[3] = sqrt(1.0 - pow(beta2, t));
  clock[1] *= lr_factor;   // train.py:328-329: the decay follows the step
}

__global__ __launch_bounds__(256) void k_adam(AdamBatch B) {
  int t = 0;
  while (t + 1 < B.count && (int)blockIdx.x >= B.chunk0[t + 1]) ++t;
  const int64_t base = (int64_t)(blockIdx.x - B.chunk0[t]) * 1024;
  float* __restrict__ p = B.p[t];
  const float* __restrict__ g = B.g[t];
  float* __restrict__ m = B.m[t];
  float* __restrict__ v = B.v[t];
  const int64_t n = B.n[t];
  const float ss = B.clock ? (float)((double)B.step_size[t] * B.clock[2]) : B.step_size[t];
  const float bc2_sqrt = B.clock ? (float)B.clock[3] : B.bc2_sqrt;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    if (i >= n) break;
    const float gi = g[i];
    const float mi = m[i] + (gi - m[i]) * (1.f - B.beta1);           // exp_avg.lerp_(grad, 1 - beta1)
    const float vi = v[i] * B.beta2 + (1.f - B.beta2) * gi * gi;     // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + B.eps;
    p[i] = p[i] - ss * (mi / denom);
  }
}

inline unsigned stream_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

extern "C" {

int ego_tv_plane(const float* table, int32_t C, int32_t H, int32_t W, float scale, double* value, float* grad, void* stream) {
  EGO_TRACE("ego_tv_plane");
  EGO_REQUIRE(C >= 1 && H >= 2 && W >= 2, "tv_plane: bad size");
  EGO_REQUIRE(table && (value || grad), "tv_plane: null argument");
  const float ah = scale * 2.f / ((float)C * (float)(H - 1) * (float)W);
  const float aw = scale * 2.f / ((float)C * (float)H * (float)(W - 1));
  k_tv_plane<<<stream_blocks((int64_t)C * H * W), 256, 0, (hipStream_t)stream>>>(table, C, H, W, ah, aw, value, grad);
  return ego_launch_status("k_tv_plane");
}

int ego_l1_table(const float* table, int64_t n, float scale, double* value, float* grad, void* stream) {
  EGO_TRACE("ego_l1_table");
  EGO_REQUIRE(n >= 1, "l1_table: bad size");
  EGO_REQUIRE(table && (value || grad), "l1_table: null argument");
  k_l1<<<stream_blocks(n), 256, 0, (hipStream_t)stream>>>(table, n, scale / (float)n, value, grad);
  return ego_launch_status("k_l1");
}

int ego_line_ortho(const float* line, int32_t C, int32_t n, float scale, double* value, float* grad, void* stream) {
  EGO_TRACE("ego_line_ortho");
  EGO_REQUIRE(C >= 2 && C <= 64 && n >= 1, "line_ortho: bad size (2 <= n_comp <= 64)");
  EGO_REQUIRE(line && (value || grad), "line_ortho: null argument");
  k_line_ortho<<<1, 256, 0, (hipStream_t)stream>>>(line, C, n, scale, value, grad);
  return ego_launch_status("k_line_ortho");
}

int ego_ray_entropy(const float* alpha, int64_t N, int32_t S, int32_t stride, double* value, float* g_alpha, void* stream) {
  EGO_TRACE("ego_ray_entropy");
  EGO_REQUIRE(N >= 0 && S >= 1 && stride >= S, "ray_entropy: bad size");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(alpha && (value || g_alpha), "ray_entropy: null argument");
  k_ray_entropy<<<(unsigned)((N + 3) / 4), 256, 0, (hipStream_t)stream>>>(alpha, N, S, stride, value, g_alpha);
  return ego_launch_status("k_ray_entropy");
}

int ego_ray_distortion(const float* alpha, int32_t alpha_stride, const float* z, int64_t N, int32_t S, float near_, float far_, int32_t space,
                       double* value, float* g_alpha, void* stream) {
  EGO_TRACE("ego_ray_distortion");
  EGO_REQUIRE(N >= 0 && (N + 3) / 4 <= INT32_MAX && S >= 2 && alpha_stride >= S, "ray_distortion: bad size (S >= 2, alpha_stride >= S)");
  EGO_REQUIRE(space == EGO_DIST_LINEAR || space == EGO_DIST_LOG || space == EGO_DIST_DISPARITY, "ray_distortion: unknown space");
  EGO_REQUIRE(far_ > near_ && far_ < INFINITY && near_ > -INFINITY, "ray_distortion: needs finite near < far");
  EGO_REQUIRE(space == EGO_DIST_LINEAR || near_ > 0.f, "ray_distortion: the log and disparity spaces need near > 0");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(alpha && z && (value || g_alpha), "ray_distortion: null argument");
  const double n = (double)near_, f = (double)far_;
  const double span = space == EGO_DIST_LINEAR ? f - n : space == EGO_DIST_LOG ? log(f / n) : 1.0 / n - 1.0 / f;
  const DistMap map{space, near_, (float)(1.0 / span)};
  k_ray_distortion<<<(unsigned)((N + 3) / 4), 256, 0, (hipStream_t)stream>>>(alpha, alpha_stride, z, N, S, map, value, g_alpha);
  return ego_launch_status("k_ray_distortion");
}

int64_t ego_ray_depth_loss_workspace_bytes(int64_t N) { return N < 0 ? -1 : (int64_t)offsetof(DepthWorkspace, term) + N * (int64_t)sizeof(double); }

int ego_ray_depth_loss(const float* alpha, int32_t alpha_stride, const float* z, const float* target, const float* tail, int64_t N, int32_t S,
                       float near_, float far_, int32_t space, int32_t kind, void* workspace, double* value, float* g_alpha, float* pred,
                       void* stream) {
  EGO_TRACE("ego_ray_depth_loss");
  EGO_REQUIRE(N >= 0 && (N + 3) / 4 <= INT32_MAX && S >= 2 && (alpha_stride == S || alpha_stride == S + 1),
              "ray_depth_loss: bad size (S >= 2, alpha_stride = S or S + 1)");
  EGO_REQUIRE(space == EGO_DIST_METRIC || space == EGO_DIST_LOG || space == EGO_DIST_DISPARITY,
              "ray_depth_loss: unknown space (metric, log or disparity)");
  EGO_REQUIRE(kind == EGO_DEPTH_L2 || kind == EGO_DEPTH_L1, "ray_depth_loss: unknown kind (l2 or l1)");
  EGO_REQUIRE(space == EGO_DIST_METRIC || (far_ > near_ && far_ < INFINITY && near_ > 0.f),
              "ray_depth_loss: the log and disparity spaces need finite 0 < near < far");
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(alpha && z && (value || g_alpha || pred), "ray_depth_loss: null argument");
  const bool loss = value || g_alpha;
  EGO_REQUIRE(!loss || (target && workspace), "ray_depth_loss: a value or a gradient needs target and workspace (null)");
  EGO_REQUIRE(((uintptr_t)workspace & 7) == 0, "ray_depth_loss: the workspace must be 8-byte aligned");
  DistMap map{space, 1.f, 1.f};
  if (space != EGO_DIST_METRIC) {
    const double n = (double)near_, f = (double)far_;
    map = DistMap{space, near_, (float)(1.0 / (space == EGO_DIST_LOG ? log(f / n) : 1.0 / n - 1.0 / f))};
  }
  DepthWorkspace* ws = loss ? (DepthWorkspace*)workspace : nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (ws) {
    k_depth_count<<<1, 1024, 0, st>>>(target, N, ws);
    if (int e = ego_launch_status("k_depth_count")) return e;
  }
  k_ray_depth_loss<<<(unsigned)((N + 3) / 4), 256, 0, st>>>(alpha, alpha_stride, z, target, tail, N, S, map, kind, ws, g_alpha, pred);
  if (int e = ego_launch_status("k_ray_depth_loss")) return e;
  if (value) {
    k_depth_reduce<<<1, 256, 0, st>>>(ws, N, value);
    return ego_launch_status("k_depth_reduce");
  }
  return EGO_OK;
}

int ego_resample_table(const float* src, int32_t C, int32_t H, int32_t W, const float* xs, const float* ys, int32_t H2, int32_t W2,
                       float* dst, void* stream) {
  EGO_TRACE("ego_resample_table");
  EGO_REQUIRE(C >= 1 && H >= 1 && W >= 1 && H2 >= 1 && W2 >= 1, "resample_table: bad size");
  EGO_REQUIRE(src && xs && ys && dst, "resample_table: null argument");
  const int64_t n = (int64_t)H2 * W2 * C;
  k_resample_table<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(src, C, H, W, xs, ys, H2, W2, dst);
  return ego_launch_status("k_resample_table");
}

static int adam_launch(const ego_adam_tensor* tensors, int32_t count, float beta1, float beta2, float eps, double bc1, double bc2,
                       const double* clock, void* stream) {
  for (int first = 0; first < count; first += ADAM_MAX) {
    AdamBatch b{};
    b.count = count - first < ADAM_MAX ? count - first : ADAM_MAX;
    b.beta1 = beta1; b.beta2 = beta2; b.eps = eps; b.bc2_sqrt = (float)sqrt(bc2); b.clock = clock;
    int blocks = 0;
    for (int i = 0; i < b.count; ++i) {
      const ego_adam_tensor& t = tensors[first + i];
      EGO_REQUIRE(t.param && t.grad && t.exp_avg && t.exp_avg_sq && t.n >= 0, "adam_step: null tensor / negative size");
      b.p[i] = t.param; b.g[i] = t.grad; b.m[i] = t.exp_avg; b.v[i] = t.exp_avg_sq; b.n[i] = t.n;
      b.step_size[i] = (float)((double)t.lr / bc1);
      b.chunk0[i] = blocks;
      blocks += (int)((t.n + 1023) / 1024);
    }
    b.chunk0[b.count] = blocks;
    if (blocks == 0) continue;
    k_adam<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(b);
    if (int e = ego_launch_status("k_adam")) return e;
  }
  return EGO_OK;
}

int ego_adam_step(const ego_adam_tensor* tensors, int32_t count, float beta1, float beta2, float eps, int32_t step, void* stream) {
  EGO_TRACE("ego_adam_step");
  EGO_REQUIRE(count >= 0 && step >= 1, "adam_step: bad count / step (steps count from 1)");
  if (count == 0) return EGO_OK;
  EGO_REQUIRE(tensors, "adam_step: null argument");
  return adam_launch(tensors, count, beta1, beta2, eps, 1.0 - pow((double)beta1, (double)step), 1.0 - pow((double)beta2, (double)step), nullptr, stream);
}

int ego_adam_step_graph(const ego_adam_tensor* tensors, int32_t count, float beta1, float beta2, float eps, double lr_factor, double* clock,
                        void* stream) {
  EGO_TRACE("ego_adam_step_graph");
  EGO_REQUIRE(count >= 0 && lr_factor > 0.0, "adam_step_graph: bad count / lr_factor");
  if (count == 0) return EGO_OK;
  EGO_REQUIRE(tensors && clock, "adam_step_graph: null argument");
  k_adam_clock<<<1, 1, 0, (hipStream_t)stream>>>(clock, (double)beta1, (double)beta2, lr_factor);
  if (int e = ego_launch_status("k_adam_clock")) return e;
  return adam_launch(tensors, count, beta1, beta2, eps, 1.0, 0.0, clock, stream);
}

}  // extern "C"
