// The structural term on patch batches (include/egonerf_hip.h: ego_patch_ssim): 1 - mean SSIM over the 'valid' Gaussian windows of P
// patches of ph x pw pixels, rows p ph pw + a pw + b of rgb / target [.][3] (ego_ray_batch_sample_patches' layout), with the gradient with
// respect to rgb.  The reference has no counterpart: its rgb_ssim (utils.py:104-152) is an evaluation metric on whole images without a
// gradient, and its samplers draw independent pixels.
//
//   g = ego_ssim_taps (utils.py:117-121, the metric's window).  Per patch p, channel c and window origin (i, j), 0 <= i <= ph - fs,
//   0 <= j <= pw - fs, with weights g_a g_b over x = rgb, y = target:  mux, muy, Exx, Eyy, Exy;  sxx = Exx - mux^2, syy = Eyy - muy^2,
//   sxy = Exy - mux muy;  A1 = 2 mux muy + C1, B1 = mux^2 + muy^2 + C1, A2 = 2 sxy + C2, B2 = sxx + syy + C2, S = A1 A2 / (B1 B2).
//   The metric's rounding guards (the clamps of sxx, syy and sxy, the float32 squares) are left out: a loss must be smooth.
//   A window is valid iff every pixel under it has a finite weight > 0 (weight NULL: 1) and three finite target channels; M = the number
//   of valid (patch, window) pairs;  value = 1 - (1 / 3M) sum S over valid windows and channels.
//   dS/dExx = -S / B2, dS/dExy = 2 A1 / (B1 B2), dmu = (A2 / B2)(2 muy B1 - 2 mux A1) / B1^2 + 2 mux S / B2 - 2 muy A1 / (B1 B2);
//   g_rgb[pixel] = -(1 / 3M) sum over the valid windows covering it of g_a g_b (dmu + 2 x dS/dExx + y dS/dExy)
//
// All sums and products are float64 over the float32 inputs, and every sum has a fixed order:
//   k_patch_ssim_count  block p: the patch's pixel validity to LDS, its valid windows counted; the count goes to the workspace.
//   k_patch_ssim        block p: M = the counts added by every block alike (integers).  Per channel: x and y of the patch to LDS; the five
//                       row-filtered moments to LDS (rows, then columns, as k_rgb_ssim takes them); each thread's windows -> S and the
//                       three coefficient fields (dmu, dS/dExx, dS/dExy; 0 on an invalid window), which replace the row moments in LDS;
//                       then, per field, the transposed filter - over the window columns into LDS, over the window rows into the
//                       pixel's register, taps in ascending window order - and the pixel's gradient, rounded once.  The patch's sum of S:
//                       per thread in (channel, window) order, then block_sum_256's tree, to the workspace.
//   k_patch_ssim_finish one block adds the patch sums, thread t taking patches t, t + 256, ..., then the same tree, and writes the value.
// No atomics; value-only, gradient-only, joint and repeated calls return the same bits.
#include <stddef.h>

#include "ego_device.h"
#include "ego_host.h"

namespace {

constexpr int kMaxFs = 15, kMaxSide = 32, kMaxPix = kMaxSide * kMaxSide, kSlots = kMaxPix / 256;

struct PatchSsimArgs {
  const float* rgb;
  const float* target;
  const float* weight;   // or NULL: 1
  int64_t P;
  int32_t ph, pw, fs;
  double filt[kMaxFs];
  double c1, c2;
};

template <class T>
__device__ __forceinline__ T block_sum_256(T v, T* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  const T tot = red[0];
  __syncthreads();   // red is used again
  return tot;
}

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < INFINITY; }   // false for NaN

// pv[e] = pixel e of patch p is valid; wv[w] = every pixel under window w is; -> this thread's share of the patch's valid windows.
// Ends with a barrier: pv and wv can be read by every thread.
__device__ __forceinline__ int patch_validity(const PatchSsimArgs& a, int64_t p, uint8_t* pv, uint8_t* wv) {
  const int npx = a.ph * a.pw, ho = a.ph - a.fs + 1, wo = a.pw - a.fs + 1;
  for (int e = threadIdx.x; e < npx; e += 256) {
    const int64_t n = p * npx + e;
    const float w = a.weight ? a.weight[n] : 1.f;
    const float t0 = a.target[n * 3], t1 = a.target[n * 3 + 1], t2 = a.target[n * 3 + 2];
    pv[e] = (w > 0.f && w < INFINITY && finite_f(t0) && finite_f(t1) && finite_f(t2)) ? 1 : 0;
  }
  __syncthreads();
  int count = 0;
  for (int w = threadIdx.x; w < ho * wo; w += 256) {
    const int i = w / wo, j = w - i * wo;
    int ok = 1;
    for (int dy = 0; dy < a.fs; ++dy)
      for (int dx = 0; dx < a.fs; ++dx) ok &= pv[(i + dy) * a.pw + j + dx];
    wv[w] = (uint8_t)ok;
    count += ok;
  }
  __syncthreads();
  return count;
}

__global__ __launch_bounds__(256) void k_patch_ssim_count(PatchSsimArgs a, int64_t* __restrict__ counts) {
  __shared__ uint8_t pv[kMaxPix], wv[kMaxPix];
  __shared__ int64_t red[256];
  const int64_t m = block_sum_256<int64_t>(patch_validity(a, blockIdx.x, pv, wv), red);
  if (threadIdx.x == 0) counts[blockIdx.x] = m;
}

// the batch's M from the per-patch counts, by every thread of a 256-thread block (integers: the same whatever the order)
__device__ __forceinline__ int64_t total_count(const int64_t* __restrict__ counts, int64_t P, int64_t* red) {
  int64_t m = 0;
  for (int64_t b = threadIdx.x; b < P; b += 256) m += counts[b];
  return block_sum_256<int64_t>(m, red);
}

__global__ __launch_bounds__(256) void k_patch_ssim(PatchSsimArgs a, const int64_t* __restrict__ counts, double* __restrict__ sums,
                                                    float* __restrict__ g_rgb) {
  __shared__ float xs[kMaxPix], ys[kMaxPix];
  __shared__ uint8_t pv[kMaxPix], wv[kMaxPix];
  __shared__ double U[5 * kMaxPix];   // the five row-filtered moment fields [ph][wo]; then three coefficient fields [ho][wo] and tmp [ho][pw]
  __shared__ double red[256];
  const int64_t p = blockIdx.x;
  const int ph = a.ph, pw = a.pw, fs = a.fs, npx = ph * pw, ho = ph - fs + 1, wo = pw - fs + 1, nw = ho * wo;
  const int64_t M = total_count(counts, a.P, (int64_t*)red);
  patch_validity(a, p, pv, wv);
  double* const coef = U;                 // [3][nw]
  double* const tmp = U + 3 * kMaxPix;    // [ho][pw]
  // the pixels of this thread that some valid window covers: the others' gradient is exactly 0 whatever their x and y hold
  unsigned covered = 0;
  if (g_rgb) {
    for (int k = 0; k < kSlots; ++k) {
      const int e = threadIdx.x + 256 * k;
      if (e >= npx) break;
      const int r = e / pw, c = e - r * pw;
      const int i0 = r - fs + 1 > 0 ? r - fs + 1 : 0, i1 = r < ho - 1 ? r : ho - 1;
      const int j0 = c - fs + 1 > 0 ? c - fs + 1 : 0, j1 = c < wo - 1 ? c : wo - 1;
      int any = 0;
      for (int i = i0; i <= i1; ++i)
        for (int j = j0; j <= j1; ++j) any |= wv[i * wo + j];
      covered |= (unsigned)any << k;
    }
  }
  const double inv3M = M > 0 ? 1.0 / (3.0 * (double)M) : 0.0;
  double part = 0.0;
  for (int ch = 0; ch < 3; ++ch) {
    for (int e = threadIdx.x; e < npx; e += 256) {
      xs[e] = a.rgb[(p * npx + e) * 3 + ch];
      ys[e] = a.target[(p * npx + e) * 3 + ch];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < ph * wo; e += 256) {   // rows: (pixel row py, window column j)
      const int py = e / wo, j = e - py * wo;
      double r0 = 0, r1 = 0, r00 = 0, r11 = 0, r01 = 0;
      for (int dx = 0; dx < fs; ++dx) {
        const double x = (double)xs[py * pw + j + dx], y = (double)ys[py * pw + j + dx];
        const double w = a.filt[dx];
        r0 += w * x; r1 += w * y;
        r00 += w * (x * x); r11 += w * (y * y); r01 += w * (x * y);
      }
      U[e] = r0; U[kMaxPix + e] = r1; U[2 * kMaxPix + e] = r00; U[3 * kMaxPix + e] = r11; U[4 * kMaxPix + e] = r01;
    }
    __syncthreads();
    double cf[kSlots][3];
    for (int k = 0; k < kSlots; ++k) {   // columns: this thread's windows
      const int w = threadIdx.x + 256 * k;
      cf[k][0] = cf[k][1] = cf[k][2] = 0.0;
      if (w >= nw || !wv[w]) continue;   // an invalid window adds nothing and hands nothing back
      const int i = w / wo, j = w - i * wo;
      double mux = 0, muy = 0, exx = 0, eyy = 0, exy = 0;
      for (int dy = 0; dy < fs; ++dy) {
        const double g = a.filt[dy];
        const int o = (i + dy) * wo + j;
        mux += g * U[o]; muy += g * U[kMaxPix + o];
        exx += g * U[2 * kMaxPix + o]; eyy += g * U[3 * kMaxPix + o]; exy += g * U[4 * kMaxPix + o];
      }
      const double sxx = exx - mux * mux, syy = eyy - muy * muy, sxy = exy - mux * muy;
      const double A1 = 2.0 * (mux * muy) + a.c1, B1 = mux * mux + muy * muy + a.c1;
      const double A2 = 2.0 * sxy + a.c2, B2 = sxx + syy + a.c2;
      const double S = (A1 * A2) / (B1 * B2);
      part += S;
      const double dExx = -S / B2, dExy = 2.0 * A1 / (B1 * B2);
      cf[k][0] = (A2 / B2) * (2.0 * muy * B1 - 2.0 * mux * A1) / (B1 * B1) + 2.0 * mux * S / B2 - 2.0 * muy * A1 / (B1 * B2);
      cf[k][1] = dExx;
      cf[k][2] = dExy;
    }
    if (g_rgb) {   // block-uniform
      __syncthreads();   // every window has read its row moments: the coefficient fields take their place
      for (int k = 0; k < kSlots; ++k) {
        const int w = threadIdx.x + 256 * k;
        if (w >= nw) break;
        coef[w] = cf[k][0]; coef[kMaxPix + w] = cf[k][1]; coef[2 * kMaxPix + w] = cf[k][2];
      }
      __syncthreads();
      double F[kSlots][3];
      for (int f = 0; f < 3; ++f) {
        for (int e = threadIdx.x; e < ho * pw; e += 256) {   // transposed filter over the window columns: (window row i, pixel column c)
          const int i = e / pw, c = e - i * pw;
          const int j0 = c - fs + 1 > 0 ? c - fs + 1 : 0, j1 = c < wo - 1 ? c : wo - 1;
          double t = 0.0;
          for (int j = j0; j <= j1; ++j) t += a.filt[c - j] * coef[f * kMaxPix + i * wo + j];
          tmp[e] = t;
        }
        __syncthreads();
        for (int k = 0; k < kSlots; ++k) {   // ... and over the window rows, for this thread's pixels
          const int e = threadIdx.x + 256 * k;
          if (e >= npx) break;
          const int r = e / pw, c = e - r * pw;
          const int i0 = r - fs + 1 > 0 ? r - fs + 1 : 0, i1 = r < ho - 1 ? r : ho - 1;
          double t = 0.0;
          for (int i = i0; i <= i1; ++i) t += a.filt[r - i] * tmp[i * pw + c];
          F[k][f] = t;
        }
        __syncthreads();   // tmp is written again
      }
      for (int k = 0; k < kSlots; ++k) {
        const int e = threadIdx.x + 256 * k;
        if (e >= npx) break;
        float g = 0.f;
        if ((covered >> k) & 1u) {
          const double x = (double)xs[e], y = (double)ys[e];
          g = (float)(-((F[k][0] + 2.0 * x * F[k][1]) + y * F[k][2]) * inv3M);
        }
        g_rgb[(p * npx + e) * 3 + ch] = g;
      }
    }
    __syncthreads();   // the next channel overwrites xs, ys and U
  }
  part = block_sum_256<double>(part, red);
  if (threadIdx.x == 0) sums[p] = part;
}

__global__ __launch_bounds__(256) void k_patch_ssim_finish(const int64_t* __restrict__ counts, const double* __restrict__ sums, int64_t P,
                                                           double* __restrict__ value) {
  __shared__ double red[256];
  const int64_t M = total_count(counts, P, (int64_t*)red);
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < P; b += 256) s += sums[b];
  s = block_sum_256<double>(s, red);
  if (threadIdx.x == 0) *value = M > 0 ? 1.0 - s / (3.0 * (double)M) : 0.0;
}

}  // namespace

extern "C" {

int64_t ego_patch_ssim_workspace_bytes(int64_t P, int32_t ph, int32_t pw) {
  if (P < 0 || ph < 1 || pw < 1 || ph > kMaxSide || pw > kMaxSide) return -1;
  return P * (int64_t)(sizeof(int64_t) + sizeof(double));   // per patch: its valid-window count and its sum of S
}

int ego_patch_ssim(const float* rgb, const float* target, const float* weight, int64_t P, int32_t ph, int32_t pw, int32_t filter_size,
                   double filter_sigma, double max_val, double k1, double k2, void* workspace, double* value, float* g_rgb, void* stream) {
  EGO_TRACE("ego_patch_ssim");
  EGO_REQUIRE(P >= 0, "patch_ssim: P < 0");
  EGO_REQUIRE(filter_size >= 1 && filter_size <= kMaxFs, "patch_ssim: filter_size must be 1..15");
  EGO_REQUIRE(ph >= filter_size && pw >= filter_size && ph <= kMaxSide && pw <= kMaxSide,
              "patch_ssim: a patch must cover the filter and be at most 32 x 32 (filter_size <= ph, pw <= 32)");
  EGO_REQUIRE(filter_sigma > 0.0 && filter_sigma < INFINITY, "patch_ssim: filter_sigma must be finite and > 0");
  EGO_REQUIRE(value || g_rgb, "patch_ssim: no output asked for (value and g_rgb are both null)");
  EGO_REQUIRE(P < ((int64_t)1 << 31), "patch_ssim: P must stay below 2^31 (one block per patch)");
  if (P == 0) return EGO_OK;
  EGO_REQUIRE(rgb && target, "patch_ssim: null rgb or target");
  EGO_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "patch_ssim: the workspace must be given and 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  PatchSsimArgs a{};
  a.rgb = rgb; a.target = target; a.weight = weight; a.P = P; a.ph = ph; a.pw = pw; a.fs = filter_size;
  ego_ssim_taps(filter_size, filter_sigma, a.filt);
  a.c1 = (k1 * max_val) * (k1 * max_val);
  a.c2 = (k2 * max_val) * (k2 * max_val);
  int64_t* counts = (int64_t*)workspace;
  double* sums = (double*)(counts + P);
  k_patch_ssim_count<<<(unsigned)P, 256, 0, st>>>(a, counts);
  if (int e = ego_launch_status("k_patch_ssim_count")) return e;
  k_patch_ssim<<<(unsigned)P, 256, 0, st>>>(a, counts, sums, g_rgb);
  if (int e = ego_launch_status("k_patch_ssim")) return e;
  if (value) {
    k_patch_ssim_finish<<<1, 256, 0, st>>>(counts, sums, P, value);
    return ego_launch_status("k_patch_ssim_finish");
  }
  return EGO_OK;
}

}  // extern "C"
