// Device-resident training batches (include/egonerf_hip.h: ego_ray_bank, ego_ray_batch_gather, ego_ray_batch_sample): the
// `ids = sampler.nextids(); allrays[ids], allrgbs[ids]` of train.py:247-248 as one launch that reads K poses and K 8-bit images
// instead of the materialised [K H W][6] / [K H W][3] float arrays, with the indices drawn on the device from a counter-based
// generator, so that a captured training iteration needs no input from the host.
//
// Thread per ray over a few thousand elements: latency-bound, a few microseconds; nothing here wants LDS or the matrix pipe.
#include "ego_device.h"
#include "ego_host.h"

namespace {

struct BankArgs {
  const float* poses;
  const uint32_t* images;   // one RGBA pixel per word, R in the low byte
  int32_t K, H, W, r0, n_rows, c0, n_cols, normalize;
  int64_t per_img, total;   // n_rows * n_cols, K * per_img
};

// ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter c[4], key k[2] -> c[4] ----
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// round function of the Feistel network: murmur3's 32-bit finaliser of (half + key)
__device__ __forceinline__ uint32_t feistel_f(uint32_t r, uint32_t key) {
  uint32_t x = r + key;
  x ^= x >> 16; x *= 0x85EBCA6Bu;
  x ^= x >> 13; x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// keyed bijection of [0, total): six balanced Feistel rounds over 2 * half bits, then cycle-walking - a value that lands in
// [total, 4^half) is enciphered again; the walk follows the cycle of a permutation that starts inside [0, total), so it returns there
__device__ __forceinline__ uint64_t feistel_permute(uint64_t p, uint64_t total, int half, const uint32_t key[6]) {
  const uint32_t mask = (uint32_t)(((uint64_t)1 << half) - 1);
  uint64_t v = p;
  do {
    uint32_t L = (uint32_t)(v >> half) & mask, R = (uint32_t)v & mask;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const uint32_t t = L ^ (feistel_f(R, key[r]) & mask);
      L = R; R = t;
    }
    v = ((uint64_t)L << half) | R;
  } while (v >= total);
  return v;
}

// one row of all_rays / all_rgbs (dataLoader/dataset_omniblender.py:71-84) from the pose and the 8-bit pixel
__device__ __forceinline__ void gather_row(const BankArgs& b, int64_t id, int64_t i, float* __restrict__ rays, float* __restrict__ rgb) {
  if (id < 0 || id >= b.total) {   // outside the caller's contract: touch no memory of the bank, mark the row
    const float nan = __int_as_float(0x7fc00000);
    if (rays) for (int k = 0; k < 6; ++k) rays[i * 6 + k] = nan;
    if (rgb) for (int k = 0; k < 3; ++k) rgb[i * 3 + k] = nan;
    return;
  }
  const int img = (int)(id / b.per_img);
  const int64_t rem = id - (int64_t)img * b.per_img;
  const int row = b.r0 + (int)(rem / b.n_cols), col = b.c0 + (int)(rem % b.n_cols);
  if (rays) {
    float o[6];
    erp_ray(b.H, b.W, row, col, b.poses + (int64_t)img * 12, b.normalize, o);
#pragma unroll
    for (int k = 0; k < 6; ++k) rays[i * 6 + k] = o[k];
  }
  if (rgb) {
    const uint32_t px = b.images[((int64_t)img * b.H + row) * b.W + col];
    // ToTensor: u8 / 255 (a true division), then img[:, :3] * a + (1 - a), every operation rounded on its own
    const float a = __fdiv_rn((float)(px >> 24), 255.f);
    const float one_minus_a = __fsub_rn(1.f, a);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float t = __fdiv_rn((float)((px >> (8 * k)) & 0xffu), 255.f);
      rgb[i * 3 + k] = __fadd_rn(__fmul_rn(t, a), one_minus_a);
    }
  }
}

__global__ __launch_bounds__(256) void k_ray_batch_gather(BankArgs b, const int64_t* __restrict__ idx, int64_t B, float* __restrict__ rays,
                                                          float* __restrict__ rgb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  gather_row(b, idx[i], i, rays, rgb);
}

__global__ __launch_bounds__(256) void k_ray_batch_sample(BankArgs b, int mode, uint32_t seed_lo, uint32_t seed_hi,
                                                          const int64_t* __restrict__ counter, const float* __restrict__ row_cdf, int64_t B,
                                                          int64_t batches_per_epoch, int half_bits, int64_t* __restrict__ idx,
                                                          float* __restrict__ rays, float* __restrict__ rgb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const uint64_t c = (uint64_t)*counter;
  int64_t id;
  if (mode == EGO_BATCH_SIMPLE) {
    const uint64_t epoch = c / (uint64_t)batches_per_epoch, in_epoch = c % (uint64_t)batches_per_epoch;
    uint32_t key[8];
#pragma unroll
    for (int j = 0; j < 2; ++j) {   // round keys = Philox(seed; epoch, block j): the same for every lane of the epoch
      uint32_t x[4] = {(uint32_t)epoch, (uint32_t)(epoch >> 32), (uint32_t)j, 0x46656973u};
      philox4x32_10(x, seed_lo, seed_hi);
#pragma unroll
      for (int k = 0; k < 4; ++k) key[4 * j + k] = x[k];
    }
    id = (int64_t)feistel_permute(in_epoch * (uint64_t)B + (uint64_t)i, (uint64_t)b.total, half_bits, key);
  } else {
    uint32_t x[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)c, (uint32_t)(c >> 32)};
    philox4x32_10(x, seed_lo, seed_hi);
    // uniform integers by the high half of a 32 x 32-bit product (bias <= n / 2^32)
    const int img = (int)(((uint64_t)x[0] * (uint32_t)b.K) >> 32);
    const int col = (int)(((uint64_t)x[1] * (uint32_t)b.n_cols) >> 32);
    const float u = (float)(x[2] >> 8) * 5.9604644775390625e-8f;   // 24 bits: exact in float32, in [0, 1)
    int lo = 0, hi = b.n_rows - 1;   // first entry > u; the last entry counts as 1 whatever it holds
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (row_cdf[mid] > u) hi = mid; else lo = mid + 1;
    }
    id = (int64_t)img * b.per_img + (int64_t)lo * b.n_cols + col;
  }
  idx[i] = id;
  if (rays || rgb) gather_row(b, id, i, rays, rgb);
}

// key tweaks of the patch mode's two Philox streams (xor into the low key word): EGO_BATCH_THETA keys with the seed itself and the same
// counter words, so the tweak is what keeps the three streams apart
constexpr uint32_t kPatchKeyTweak = 0x50415443u, kPatchRandomKeyTweak = 0x52414E44u;   // "PATC", "RAND"

struct PatchPlan {
  int64_t n_patch_rows;      // P * ph * pw
  int32_t ph, pw, stride;
  int32_t row_origins;       // n_rows - (ph - 1) * stride
  int32_t col_origins;       // n_cols when the panorama wraps, else n_cols - (pw - 1) * stride
  int32_t wrap;
};

// rows [0, P ph pw): row p ph pw + a pw + b = pixel (row0_p + a stride, col0_p + b stride) of image img_p, the origin drawn once per patch
// (every thread of a patch computes the same three integers); the rows behind them: independent uniform pixels
__global__ __launch_bounds__(256) void k_ray_batch_sample_patches(BankArgs b, PatchPlan pl, uint32_t seed_lo, uint32_t seed_hi,
                                                                  const int64_t* __restrict__ counter, int64_t B, int64_t* __restrict__ idx,
                                                                  float* __restrict__ rays, float* __restrict__ rgb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const uint64_t c = (uint64_t)*counter;
  int img, row, col;
  if (i < pl.n_patch_rows) {
    const int64_t per = (int64_t)pl.ph * pl.pw;
    const uint64_t p = (uint64_t)(i / per);
    const int64_t e = i - (int64_t)p * per;
    const int pa = (int)(e / pl.pw), pb = (int)(e - (int64_t)pa * pl.pw);
    uint32_t x[4] = {(uint32_t)p, (uint32_t)(p >> 32), (uint32_t)c, (uint32_t)(c >> 32)};
    philox4x32_10(x, seed_lo ^ kPatchKeyTweak, seed_hi);
    img = (int)(((uint64_t)x[0] * (uint32_t)b.K) >> 32);
    row = (int)(((uint64_t)x[1] * (uint32_t)pl.row_origins) >> 32) + pa * pl.stride;
    col = (int)(((uint64_t)x[2] * (uint32_t)pl.col_origins) >> 32) + pb * pl.stride;
    if (pl.wrap) col %= b.n_cols;   // the panorama's seam: column n_cols is column 0
  } else {
    const uint64_t r = (uint64_t)(i - pl.n_patch_rows);
    uint32_t x[4] = {(uint32_t)r, (uint32_t)(r >> 32), (uint32_t)c, (uint32_t)(c >> 32)};
    philox4x32_10(x, seed_lo ^ kPatchRandomKeyTweak, seed_hi);
    img = (int)(((uint64_t)x[0] * (uint32_t)b.K) >> 32);
    col = (int)(((uint64_t)x[1] * (uint32_t)b.n_cols) >> 32);
    row = (int)(((uint64_t)x[2] * (uint32_t)b.n_rows) >> 32);
  }
  const int64_t id = (int64_t)img * b.per_img + (int64_t)row * b.n_cols + col;
  idx[i] = id;
  if (rays || rgb) gather_row(b, id, i, rays, rgb);
}

// the depth target of one row of all_rays: the pixel gather_row reads the colour of, from a [K][H][W] float32 / float16 array
__global__ __launch_bounds__(256) void k_ray_batch_gather_depth(BankArgs b, const void* __restrict__ depth, int is_half,
                                                                const int64_t* __restrict__ idx, int64_t B, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const int64_t id = idx[i];
  if (id < 0 || id >= b.total) {   // outside the caller's contract: touch no memory of the bank, mark the row
    out[i] = __int_as_float(0x7fc00000);
    return;
  }
  const int img = (int)(id / b.per_img);
  const int64_t rem = id - (int64_t)img * b.per_img;
  const int row = b.r0 + (int)(rem / b.n_cols), col = b.c0 + (int)(rem % b.n_cols);
  const int64_t px = ((int64_t)img * b.H + row) * b.W + col;
  out[i] = is_half ? (float)((const _Float16*)depth)[px] : ((const float*)depth)[px];
}

// the mask weight of one row of all_rays: the pixel gather_row reads the colour of, from a [K][H][W] uint8 array, 255 -> 1
__global__ __launch_bounds__(256) void k_ray_batch_gather_mask(BankArgs b, const uint8_t* __restrict__ mask, const int64_t* __restrict__ idx,
                                                               int64_t B, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const int64_t id = idx[i];
  if (id < 0 || id >= b.total) {   // outside the caller's contract: touch no memory of the bank, mark the row
    out[i] = __int_as_float(0x7fc00000);
    return;
  }
  const int img = (int)(id / b.per_img);
  const int64_t rem = id - (int64_t)img * b.per_img;
  const int row = b.r0 + (int)(rem / b.n_cols), col = b.c0 + (int)(rem % b.n_cols);
  out[i] = __fdiv_rn((float)mask[((int64_t)img * b.H + row) * b.W + col], 255.f);
}

// shared argument checks; `what` names the entry point in the message
int check_bank(const ego_ray_bank* bank, bool need_images, const char* what, BankArgs* out) {
  if (!bank) return ego_fail(EGO_E_BADARG, "%s: null bank", what);
  if (!bank->poses) return ego_fail(EGO_E_BADARG, "%s: null poses", what);
  if (need_images && !bank->images) return ego_fail(EGO_E_BADARG, "%s: colours asked for but the bank has no images (null)", what);
  if (bank->K < 1) return ego_fail(EGO_E_BADARG, "%s: K < 1", what);
  if (bank->H < 1 || bank->W < 1 || bank->r0 < 0 || bank->c0 < 0 || bank->n_rows < 1 || bank->n_cols < 1 ||
      (int64_t)bank->r0 + bank->n_rows > bank->H || (int64_t)bank->c0 + bank->n_cols > bank->W)
    return ego_fail(EGO_E_BADARG, "%s: bad image window (rows [%d, +%d) of %d, columns [%d, +%d) of %d)", what, bank->r0, bank->n_rows,
                    bank->H, bank->c0, bank->n_cols, bank->W);
  if (((uintptr_t)bank->images & 3) != 0) return ego_fail(EGO_E_BADARG, "%s: images must be 4-byte aligned", what);
  out->poses = bank->poses;
  out->images = (const uint32_t*)bank->images;
  out->K = bank->K; out->H = bank->H; out->W = bank->W;
  out->r0 = bank->r0; out->n_rows = bank->n_rows; out->c0 = bank->c0; out->n_cols = bank->n_cols;
  out->normalize = bank->normalize;
  out->per_img = (int64_t)bank->n_rows * bank->n_cols;
  out->total = out->per_img * bank->K;
  return EGO_OK;
}

}  // namespace

extern "C" {

int ego_ray_batch_gather(const ego_ray_bank* bank, const int64_t* idx, int64_t B, float* rays, float* rgb, void* stream) {
  EGO_TRACE("ego_ray_batch_gather");
  BankArgs b;
  if (const int e = check_bank(bank, rgb != nullptr, "ray_batch_gather", &b)) return e;
  EGO_REQUIRE(B >= 0, "ray_batch_gather: B < 0");
  if (B == 0) return EGO_OK;
  EGO_REQUIRE(idx, "ray_batch_gather: null idx");
  EGO_REQUIRE(rays || rgb, "ray_batch_gather: null outputs (rays and rgb)");
  k_ray_batch_gather<<<nblk(B, 256), 256, 0, (hipStream_t)stream>>>(b, idx, B, rays, rgb);
  return ego_launch_status("k_ray_batch_gather");
}

int ego_ray_batch_gather_depth(const ego_ray_bank* bank, const void* depth, int32_t is_half, const int64_t* idx, int64_t B, float* out,
                               void* stream) {
  EGO_TRACE("ego_ray_batch_gather_depth");
  BankArgs b;
  if (const int e = check_bank(bank, false, "ray_batch_gather_depth", &b)) return e;
  EGO_REQUIRE(B >= 0, "ray_batch_gather_depth: B < 0");
  if (B == 0) return EGO_OK;
  EGO_REQUIRE(depth && idx && out, "ray_batch_gather_depth: null depth, idx or out");
  EGO_REQUIRE(((uintptr_t)depth & (is_half ? 1 : 3)) == 0, "ray_batch_gather_depth: depth must be aligned to its element size");
  k_ray_batch_gather_depth<<<nblk(B, 256), 256, 0, (hipStream_t)stream>>>(b, depth, is_half, idx, B, out);
  return ego_launch_status("k_ray_batch_gather_depth");
}

int ego_ray_batch_gather_mask(const ego_ray_bank* bank, const uint8_t* mask, const int64_t* idx, int64_t B, float* out, void* stream) {
  EGO_TRACE("ego_ray_batch_gather_mask");
  BankArgs b;
  if (const int e = check_bank(bank, false, "ray_batch_gather_mask", &b)) return e;
  EGO_REQUIRE(B >= 0, "ray_batch_gather_mask: B < 0");
  if (B == 0) return EGO_OK;
  EGO_REQUIRE(mask && idx && out, "ray_batch_gather_mask: null mask, idx or out");
  k_ray_batch_gather_mask<<<nblk(B, 256), 256, 0, (hipStream_t)stream>>>(b, mask, idx, B, out);
  return ego_launch_status("k_ray_batch_gather_mask");
}

int ego_ray_batch_sample(const ego_ray_bank* bank, int32_t mode, uint64_t seed, const int64_t* counter, const float* row_cdf, int64_t B,
                         int64_t* idx, float* rays, float* rgb, void* stream) {
  EGO_TRACE("ego_ray_batch_sample");
  BankArgs b;
  if (const int e = check_bank(bank, rgb != nullptr, "ray_batch_sample", &b)) return e;
  EGO_REQUIRE(mode == EGO_BATCH_SIMPLE || mode == EGO_BATCH_THETA, "ray_batch_sample: unknown mode");
  EGO_REQUIRE(B >= 0, "ray_batch_sample: B < 0");
  EGO_REQUIRE(mode != EGO_BATCH_THETA || row_cdf, "ray_batch_sample: theta_importance needs row_cdf (null)");
  EGO_REQUIRE(mode != EGO_BATCH_SIMPLE || (B <= b.total / 2), "ray_batch_sample: simple needs total >= 2 B (two batches per permutation)");
  EGO_REQUIRE(b.total < ((int64_t)1 << 62), "ray_batch_sample: total must stay below 2^62");
  if (B == 0) return EGO_OK;
  EGO_REQUIRE(counter && idx, "ray_batch_sample: null counter or idx");
  int half = 1;   // smallest even number of bits 2 * half with 4^half >= total
  while (half < 31 && ((int64_t)1 << (2 * half)) < b.total) ++half;
  const int64_t per_epoch = mode == EGO_BATCH_SIMPLE ? b.total / B : 1;
  k_ray_batch_sample<<<nblk(B, 256), 256, 0, (hipStream_t)stream>>>(b, mode, (uint32_t)seed, (uint32_t)(seed >> 32), counter, row_cdf, B,
                                                                   per_epoch, half, idx, rays, rgb);
  return ego_launch_status("k_ray_batch_sample");
}

int ego_ray_batch_sample_patches(const ego_ray_bank* bank, uint64_t seed, const int64_t* counter, int64_t P, int32_t ph, int32_t pw,
                                 int32_t stride, int64_t n_random, int64_t* idx, float* rays, float* rgb, void* stream) {
  EGO_TRACE("ego_ray_batch_sample_patches");
  BankArgs b;
  if (const int e = check_bank(bank, rgb != nullptr, "ray_batch_sample_patches", &b)) return e;
  EGO_REQUIRE(P >= 0 && n_random >= 0, "ray_batch_sample_patches: P < 0 or n_random < 0");
  EGO_REQUIRE(ph >= 1 && pw >= 1 && stride >= 1, "ray_batch_sample_patches: ph, pw and stride must be >= 1");
  const int64_t ext_rows = (int64_t)(ph - 1) * stride + 1, ext_cols = (int64_t)(pw - 1) * stride + 1;
  if (ext_rows > b.n_rows || ext_cols > b.n_cols)
    return ego_fail(EGO_E_BADARG, "ray_batch_sample_patches: a patch of %lld x %lld pixels ((ph - 1) stride + 1, (pw - 1) stride + 1) does not "
                                  "fit the bank's window of %d x %d", (long long)ext_rows, (long long)ext_cols, b.n_rows, b.n_cols);
  EGO_REQUIRE(P <= (((int64_t)1 << 62) - n_random) / ((int64_t)ph * pw), "ray_batch_sample_patches: P ph pw + n_random must stay below 2^62");
  const int64_t n_patch_rows = P * ph * pw, B = n_patch_rows + n_random;
  if (B == 0) return EGO_OK;
  EGO_REQUIRE(counter && idx, "ray_batch_sample_patches: null counter or idx");
  EGO_REQUIRE((B + 255) / 256 < ((int64_t)1 << 31), "ray_batch_sample_patches: B / 256 must stay below 2^31 blocks");
  PatchPlan pl;
  pl.n_patch_rows = n_patch_rows;
  pl.ph = ph; pl.pw = pw; pl.stride = stride;
  pl.wrap = b.c0 == 0 && b.n_cols == b.W;
  pl.row_origins = (int32_t)(b.n_rows - (ext_rows - 1));
  pl.col_origins = pl.wrap ? b.n_cols : (int32_t)(b.n_cols - (ext_cols - 1));
  k_ray_batch_sample_patches<<<nblk(B, 256), 256, 0, (hipStream_t)stream>>>(b, pl, (uint32_t)seed, (uint32_t)(seed >> 32), counter, B, idx, rays,
                                                                           rgb);
  return ego_launch_status("k_ray_batch_sample_patches");
}

}  // extern "C"
