// The photometric term for real captures (include/egonerf_hip.h: ego_photo_loss, ego_photo_fit): train.py:261's
// `torch.mean((rgb_map - rgb_train) ** 2)` with what hand-held 360 video needs next to it - a per-image affine colour map (exposure and
// white balance drift from frame to frame), a per-ray weight (the photographer, the tripod and the stitching seam must not be explained)
// and robust kinds (people walk through the footage) - plus the closed-form least-squares fit of that colour map, which evaluation
// against held-out images needs and which is the same per-image reduction.
//
//   c'_nc = gain[k][c] rgb_nc + bias[k][c], k = image[n];   r_nc = c'_nc - target_nc
//   valid(n): weight finite and > 0, the three target channels finite, 0 <= image[n] < K;   W = sum_valid w_n
//   value = (1 / 3W) sum_valid w_n sum_c rho(r_nc)
//   g_rgb_nc = w_n rho'(r_nc) gain[k][c] / 3W;   d value / d gain[k][c] = sum_{n in k} w_n rho'(r_nc) rgb_nc / 3W, bias: without rgb_nc
//
// Three channels per ray and a few thousand rays: every kernel here is latency-bound, so the per-element arithmetic is float64 like the
// sums (an output is then the float64 result rounded once).  Every sum has a fixed order:
//   k_photo_partial   block b sums w and w rho over rays b 256 + t, (b + nb) 256 + t, ... per thread, then block_sum_256's tree, and
//                     leaves the pair in the workspace; nb <= 1024 blocks
//   photo_total       thread t adds partials t, t + 256, ..., then the same tree: every block that needs W computes these same bits
//   k_photo_rays      its first blocks, thread per ray: the gradient row.  Its other blocks own one (image, slice of the batch) each: a
//                     block scans the slice's image indices 256 at a time, thread t adds the terms of rays t, t + 256, ... that belong
//                     to its image in ray order, a butterfly joins the lanes and thread 0..5 the four waves, and the six sums go to
//                     the workspace.  A slice is 2048 rays (longer beyond 64 slices), so every block is eight short rounds whatever N
//                     and K are; the index reads are N K in all - the scan scales as N K / (256 x the blocks in flight), not N + K -
//                     and it needs no sorting and no atomics.
//   k_photo_finish    block 0 adds the value; the other threads own one element of g_affine each and add its slices in slice order.
// so value-only, gradient-only, joint and repeated calls return the same bits.  ego_photo_fit is the image scan with the five moments
// per channel in the accumulators, one block per image over the whole batch (an evaluation-time call: one launch, no workspace).
#include <stddef.h>

#include "ego_device.h"
#include "ego_host.h"

namespace {

constexpr int kMaxPartialBlocks = 1024;
constexpr int kSliceRays = 2048, kMaxSlices = 64;

struct PhotoArgs {
  const float* rgb;
  const float* target;
  const float* weight;     // or NULL: 1
  const int32_t* image;    // or NULL
  const float* affine;     // [K][3][2] (gain, bias), or NULL: identity
  int64_t N;
  int32_t K, kind;
  double param;
};

struct PhotoWorkspace {
  double W, S;             // W = sum_valid w; S = sum_valid w sum_c rho
};

__device__ __forceinline__ double block_sum_256(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  const double tot = red[0];
  __syncthreads();   // red is used again
  return tot;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < INFINITY; }   // false for NaN

// the ray's weight, 0 for an invalid ray; `k` = its image (0 without image indices)
__device__ __forceinline__ double photo_weight(const float* __restrict__ target, const float* __restrict__ weight,
                                               const int32_t* __restrict__ image, int32_t K, int64_t n, int& k) {
  k = 0;
  if (image) {
    k = image[n];
    if (k < 0 || k >= K) return 0.0;
  }
  const float w = weight ? weight[n] : 1.f;   // all four loads before the first test: one latency, not two
  const float t0 = target[n * 3], t1 = target[n * 3 + 1], t2 = target[n * 3 + 2];
  if (!(w > 0.f && w < INFINITY)) return 0.0;
  if (!(finite_f(t0) && finite_f(t1) && finite_f(t2))) return 0.0;
  return (double)w;
}

__device__ __forceinline__ double photo_residual(const PhotoArgs& a, int64_t n, int k, int c, double& gain) {
  gain = 1.0;
  double v = (double)a.rgb[n * 3 + c];
  if (a.affine) {
    gain = (double)a.affine[(k * 3 + c) * 2];
    v = gain * v + (double)a.affine[(k * 3 + c) * 2 + 1];
  }
  return v - (double)a.target[n * 3 + c];
}

__device__ __forceinline__ double photo_rho(int kind, double p, double r) {
  switch (kind) {
    case EGO_PHOTO_L2: return r * r;
    case EGO_PHOTO_L1: return fabs(r);
    case EGO_PHOTO_HUBER: return fabs(r) <= p ? 0.5 * r * r : p * (fabs(r) - 0.5 * p);
    default: return sqrt(r * r + p * p) - p;
  }
}

__device__ __forceinline__ double photo_drho(int kind, double p, double r) {
  const double sign = (double)((r > 0.0) - (r < 0.0));   // 0 at r = 0
  switch (kind) {
    case EGO_PHOTO_L2: return 2.0 * r;
    case EGO_PHOTO_L1: return sign;
    case EGO_PHOTO_HUBER: return fabs(r) <= p ? r : p * sign;
    default: return r / sqrt(r * r + p * p);
  }
}

__global__ __launch_bounds__(256) void k_photo_partial(PhotoArgs a, PhotoWorkspace* __restrict__ ws) {
  __shared__ double red[256];
  double W = 0.0, S = 0.0;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < a.N; n += (int64_t)gridDim.x * 256) {
    int k;
    const double w = photo_weight(a.target, a.weight, a.image, a.K, n, k);
    if (w == 0.0) continue;
    double gain, rho = 0.0;
    for (int c = 0; c < 3; ++c) rho += photo_rho(a.kind, a.param, photo_residual(a, n, k, c, gain));
    W += w;
    S += w * rho;
  }
  W = block_sum_256(W, red);
  S = block_sum_256(S, red);
  if (threadIdx.x == 0) {
    ws[blockIdx.x].W = W;
    ws[blockIdx.x].S = S;
  }
}

// the batch's W (and S) from the nb partials, by every thread of a 256-thread block
__device__ __forceinline__ double photo_total(const PhotoWorkspace* __restrict__ ws, int nb, double* red, double* S_out) {
  double W = 0.0, S = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) {
    W += ws[b].W;
    S += ws[b].S;
  }
  W = block_sum_256(W, red);
  if (S_out) *S_out = block_sum_256(S, red);
  return W;
}

// d value / d (gain, bias) times 3W of image `img` over rays [n0, n1): six sums, thread t taking rays n0 + t, n0 + t + 256, ...
__device__ __forceinline__ void photo_image_sums(const PhotoArgs& a, int img, int64_t n0, int64_t n1, double acc[6]) {
  for (int j = 0; j < 6; ++j) acc[j] = 0.0;
  for (int64_t n = n0 + threadIdx.x; n < n1; n += 256) {
    if (a.image[n] != img) continue;
    int k;
    const double w = photo_weight(a.target, a.weight, a.image, a.K, n, k);
    const float c0 = a.rgb[n * 3], c1 = a.rgb[n * 3 + 1], c2 = a.rgb[n * 3 + 2];   // loaded with the weight and the target
    if (w == 0.0) continue;
    const float rgb[3] = {c0, c1, c2};
    for (int c = 0; c < 3; ++c) {
      double gain;
      const double d = w * photo_drho(a.kind, a.param, photo_residual(a, n, img, c, gain));
      acc[c * 2] += d * (double)rgb[c];
      acc[c * 2 + 1] += d;
    }
  }
}

// the block's total of per-thread sums v[0..n): lanes by a butterfly, then thread j adds the four waves' j-th sums in wave order
template <int NV>
__device__ __forceinline__ void block_sums(double v[NV], double (*red)[NV]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = 0; j < NV; ++j) {
    const double t = wave_sum_f64(v[j]);
    if (lane == 0) red[wave][j] = t;
  }
  __syncthreads();
  if (threadIdx.x < NV) red[0][threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  __syncthreads();
}

struct SlicePlan {
  int P;            // slices per image
  int64_t len;      // rays per slice, a multiple of 256
};

// blocks [0, grad_blocks): thread per ray, the gradient row.  Block grad_blocks + img * P + p: the six sums of image img over slice p.
__global__ __launch_bounds__(256) void k_photo_rays(PhotoArgs a, const PhotoWorkspace* __restrict__ ws, int nb, float* __restrict__ g_rgb,
                                                    unsigned grad_blocks, SlicePlan plan, double* __restrict__ slices) {
  if (blockIdx.x >= grad_blocks) {   // block-uniform
    __shared__ double red[4][6];
    const unsigned s = blockIdx.x - grad_blocks;
    const int img = (int)(s / (unsigned)plan.P), p = (int)(s % (unsigned)plan.P);
    const int64_t n0 = (int64_t)p * plan.len, n1 = n0 + plan.len < a.N ? n0 + plan.len : a.N;
    double acc[6];
    photo_image_sums(a, img, n0, n1, acc);
    block_sums<6>(acc, red);
    if (threadIdx.x < 6) slices[(int64_t)s * 6 + threadIdx.x] = red[0][threadIdx.x];
    return;
  }
  __shared__ double red[256];
  const double W = photo_total(ws, nb, red, nullptr);
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= a.N) return;
  int k;
  const double w = photo_weight(a.target, a.weight, a.image, a.K, n, k);
  for (int c = 0; c < 3; ++c) {
    float g = 0.f;   // an invalid ray, or W = 0 (then no ray is valid): exactly 0
    if (w != 0.0) {
      double gain;
      const double r = photo_residual(a, n, k, c, gain);
      g = (float)(w * photo_drho(a.kind, a.param, r) * gain / (3.0 * W));
    }
    g_rgb[n * 3 + c] = g;
  }
}

// block 0: the value; thread e of the other blocks: element e of g_affine [K][3][2], its slices added in slice order
__global__ __launch_bounds__(256) void k_photo_finish(PhotoArgs a, const PhotoWorkspace* __restrict__ ws, int nb, double* __restrict__ value,
                                                      float* __restrict__ g_affine, SlicePlan plan, const double* __restrict__ slices) {
  __shared__ double red[256];
  double S;
  const double W = photo_total(ws, nb, red, &S);
  if (blockIdx.x == 0) {
    if (value && threadIdx.x == 0 && W > 0.0) *value += S / (3.0 * W);
    return;
  }
  const int64_t e = ((int64_t)blockIdx.x - 1) * 256 + threadIdx.x;
  if (e >= (int64_t)a.K * 6) return;
  const int64_t img = e / 6;
  const int j = (int)(e % 6);
  double tot = 0.0;
  for (int p = 0; p < plan.P; ++p) tot += slices[(img * plan.P + p) * 6 + j];
  // an image without a valid ray has tot = +0, and with W = 0 no ray is valid: exactly 0 either way
  g_affine[e] = W > 0.0 ? (float)(tot / (3.0 * W)) : 0.f;
}

// One block per image: the moments W_k, sum w c, sum w t, sum w c^2, sum w c t of the image's valid rays, then the 2 x 2 solve.
__global__ __launch_bounds__(256) void k_photo_fit(PhotoArgs a, float* __restrict__ affine, double* __restrict__ Wk) {
  __shared__ double red[4][13];
  const int img = (int)blockIdx.x;
  double m[13] = {};   // W, then (sum w c, sum w t, sum w c^2, sum w c t) per channel
  for (int64_t n = threadIdx.x; n < a.N; n += 256) {
    if (a.image && a.image[n] != img) continue;
    int k;
    const double w = photo_weight(a.target, a.weight, a.image, a.K, n, k);
    const float c0 = a.rgb[n * 3], c1 = a.rgb[n * 3 + 1], c2 = a.rgb[n * 3 + 2];
    if (w == 0.0) continue;
    const float rgb[3] = {c0, c1, c2};
    m[0] += w;
    for (int c = 0; c < 3; ++c) {
      const double x = (double)rgb[c], t = (double)a.target[n * 3 + c];
      m[1 + c * 4] += w * x;
      m[2 + c * 4] += w * t;
      m[3 + c * 4] += w * (x * x);
      m[4 + c * 4] += w * (x * t);
    }
  }
  block_sums<13>(m, red);
  const double W = red[0][0];
  if (Wk && threadIdx.x == 0) Wk[img] = W;
  if (threadIdx.x >= 3) return;
  const int c = threadIdx.x;
  const double Sx = red[0][1 + c * 4], St = red[0][2 + c * 4], Sxx = red[0][3 + c * 4], Sxt = red[0][4 + c * 4];
  double gain = 1.0, bias = 0.0;
  if (W > 0.0) {
    const double det = W * Sxx - Sx * Sx;
    if (det <= 1e-9 * (W * Sxx)) {   // all colours equal (the definition of degenerate, not a tolerance): only the bias is determined
      bias = St / W - Sx / W;
    } else {
      gain = (W * Sxt - Sx * St) / det;
      bias = (St - gain * Sx) / W;
    }
  }
  affine[((int64_t)img * 3 + c) * 2] = (float)gain;
  affine[((int64_t)img * 3 + c) * 2 + 1] = (float)bias;
}

int partial_blocks(int64_t N) {
  const int64_t nb = (N + 255) / 256;
  return (int)(nb < 1 ? 1 : nb > kMaxPartialBlocks ? kMaxPartialBlocks : nb);
}

SlicePlan slice_plan(int64_t N) {
  SlicePlan pl;
  int64_t P = (N + kSliceRays - 1) / kSliceRays;
  P = P < 1 ? 1 : P > kMaxSlices ? kMaxSlices : P;
  pl.P = (int)P;
  pl.len = ((N + P - 1) / P + 255) / 256 * 256;
  if (pl.len < 256) pl.len = 256;
  return pl;
}

}  // namespace

extern "C" {

int64_t ego_photo_loss_workspace_bytes(int64_t N, int32_t K) {
  if (N < 0) return -1;   // the partials, then six float64 sums per image and slice
  return (int64_t)sizeof(PhotoWorkspace) * partial_blocks(N) + (K > 0 ? (int64_t)K * slice_plan(N).P * 6 * (int64_t)sizeof(double) : 0);
}

int ego_photo_loss(const float* rgb, const float* target, const float* weight, const int32_t* image, const float* affine, int64_t N, int32_t K,
                   int32_t kind, float param, void* workspace, double* value, float* g_rgb, float* g_affine, void* stream) {
  EGO_TRACE("ego_photo_loss");
  EGO_REQUIRE(kind == EGO_PHOTO_L2 || kind == EGO_PHOTO_L1 || kind == EGO_PHOTO_HUBER || kind == EGO_PHOTO_CHARBONNIER,
              "photo_loss: unknown kind (l2, l1, huber or charbonnier)");
  if (kind == EGO_PHOTO_HUBER || kind == EGO_PHOTO_CHARBONNIER)
    EGO_REQUIRE(param > 0.f && param < INFINITY, "photo_loss: huber and charbonnier need a finite param > 0 (delta, epsilon)");
  EGO_REQUIRE(N >= 0, "photo_loss: N < 0");
  EGO_REQUIRE(rgb && target, "photo_loss: null rgb or target");
  EGO_REQUIRE(value || g_rgb || g_affine, "photo_loss: no output asked for (value, g_rgb, g_affine are all null)");
  EGO_REQUIRE(!affine || image, "photo_loss: affine needs image (the image index of every ray)");
  EGO_REQUIRE(!g_affine || image, "photo_loss: g_affine needs image (the image index of every ray)");
  EGO_REQUIRE(!(affine || g_affine) || K >= 1, "photo_loss: K < 1 with affine or g_affine");
  EGO_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "photo_loss: the workspace must be given and 8-byte aligned");
  if (N == 0) return EGO_OK;
  hipStream_t st = (hipStream_t)stream;
  PhotoArgs a{rgb, target, weight, image, affine, N, K, kind, (double)param};
  PhotoWorkspace* ws = (PhotoWorkspace*)workspace;
  const int nb = partial_blocks(N);
  k_photo_partial<<<nb, 256, 0, st>>>(a, ws);
  if (int e = ego_launch_status("k_photo_partial")) return e;
  const SlicePlan plan = slice_plan(N);
  double* slices = (double*)(ws + nb);
  const int64_t grad_blocks = g_rgb ? (N + 255) / 256 : 0, scan_blocks = g_affine ? (int64_t)K * plan.P : 0;
  EGO_REQUIRE(grad_blocks + scan_blocks < ((int64_t)1 << 31), "photo_loss: N / 256 + K x slices must stay below 2^31 blocks");
  if (grad_blocks + scan_blocks > 0) {
    k_photo_rays<<<(unsigned)(grad_blocks + scan_blocks), 256, 0, st>>>(a, ws, nb, g_rgb, (unsigned)grad_blocks, plan, slices);
    if (int e = ego_launch_status("k_photo_rays")) return e;
  }
  if (value || g_affine) {
    k_photo_finish<<<1 + (g_affine ? nblk((int64_t)K * 6, 256) : 0), 256, 0, st>>>(a, ws, nb, value, g_affine, plan, slices);
    return ego_launch_status("k_photo_finish");
  }
  return EGO_OK;
}

int ego_photo_fit(const float* rgb, const float* target, const float* weight, const int32_t* image, int64_t N, int32_t K, float* affine,
                  double* Wk, void* stream) {
  EGO_TRACE("ego_photo_fit");
  EGO_REQUIRE(N >= 0, "photo_fit: N < 0");
  EGO_REQUIRE(K >= 1, "photo_fit: K < 1");
  EGO_REQUIRE(image || K == 1, "photo_fit: without image indices there is one image (K = 1)");
  EGO_REQUIRE(affine, "photo_fit: null affine");
  EGO_REQUIRE(N == 0 || (rgb && target), "photo_fit: null rgb or target");
  PhotoArgs a{rgb, target, weight, image, nullptr, N, K, EGO_PHOTO_L2, 0.0};
  k_photo_fit<<<(unsigned)K, 256, 0, (hipStream_t)stream>>>(a, affine, Wk);   // N == 0: every image gets (1, 0)
  return ego_launch_status("k_photo_fit");
}

}  // extern "C"
