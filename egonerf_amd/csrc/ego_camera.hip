// Camera paths on the device (include/egonerf_hip.h: ego_camera_rays, ego_finish_frame): the two ends of the reference's
// evaluation_path (renderer.py:199-255).  ego_camera_rays generates the rays of a window of pixels of an equirectangular or pinhole
// camera from a pose that lives in device memory, so a captured frame follows a pose that is overwritten between replays;
// ego_finish_frame turns a chunk's float32 colour and depth into the 8-bit images the reference writes (clamp, * 255, truncate;
// depth -> 8-bit index -> palette), straight into device memory or mapped pinned host memory.  ego_camera_rays_ex adds the eyes of an
// omnidirectional-stereo panorama and s x s sub-pixel samples, ego_resolve_frame averages such samples before it quantises.
//
// Both kernels are one thread per pixel (per four pixels for the bytes) over at most a few million elements: bound by their stores,
// a few microseconds per chunk next to a render of about a millisecond; nothing here wants LDS or the matrix pipe.
#include "ego_device.h"
#include "ego_host.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct CamArgs {
  int32_t model, H, W, normalize;
  float fx, fy, cx, cy;
};

// One ray of pixel (row, col) of camera `c`: the body of k_camera_rays and k_camera_rays_ex, so a sub-pixel sample has the bits of the
// corresponding pixel of the fine camera.
__device__ __forceinline__ void camera_ray(const CamArgs& c, const float* __restrict__ pose, int row, int col, float* o) {
  if (c.model == EGO_CAM_ERP) {
    erp_ray(c.H, c.W, row, col, pose, c.normalize, o);   // ego_device.h: the body ego_erp_rays runs
  } else {
    // get_ray_directions / get_ray_directions_blender (dataLoader/ray_utils.py:43-82): grid + 0.5, (i - cx) / fx, (j - cy) / fy, 1 -
    // every operation rounded on its own, true divisions - then get_rays (:85-113): d = R dir, o = t, no normalisation
    const float x = __fdiv_rn(__fsub_rn((float)col + 0.5f, c.cx), c.fx);
    float y = __fdiv_rn(__fsub_rn((float)row + 0.5f, c.cy), c.fy), z = 1.f;
    if (c.model == EGO_CAM_PINHOLE_BLENDER) { y = -y; z = -1.f; }
    o[0] = pose[3]; o[1] = pose[7]; o[2] = pose[11];
#pragma unroll
    for (int r = 0; r < 3; ++r)
      o[3 + r] = __fadd_rn(__fadd_rn(__fmul_rn(x, pose[4 * r]), __fmul_rn(y, pose[4 * r + 1])), __fmul_rn(z, pose[4 * r + 2]));
  }
}

__device__ __forceinline__ void store_ray(float* __restrict__ rays, int64_t i, const float* o) {
  f32x2* out = (f32x2*)(rays + i * 6);   // 24 bytes per row: 8-byte aligned whenever `rays` is (checked by the entry point)
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = f32x2{o[2 * k], o[2 * k + 1]};
}

__global__ __launch_bounds__(256) void k_camera_rays(CamArgs c, const float* __restrict__ pose, int64_t first, int64_t count,
                                                     float* __restrict__ rays) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int64_t p = first + i;
  const int row = (int)(p / c.W), col = (int)(p - (int64_t)row * c.W);
  float o[6];
  camera_ray(c, pose, row, col, o);
  store_ray(rays, i, o);
}

// Eyes and sub-pixel samples.  One thread per RAY: ray i = q ss^2 + a ss + b is fine pixel (row ss + a, col ss + b) of output pixel
// first + q = row (W / ss) + col, so the ss^2 samples of an output pixel are contiguous and a wave's stores stay one contiguous run.
// eye_sign = -1 / 0 / +1 (left / centre / right): the origin moves to +-half_ipd (cos phi, 0, -sin phi) in camera space - forward x
// up of the horizontal viewing direction (-sin phi, 0, -cos phi) - with phi formed as erp_ray forms it; the direction is untouched.
__global__ __launch_bounds__(256) void k_camera_rays_ex(CamArgs c, const float* __restrict__ pose, int64_t first, int64_t n_rays, int32_t ss,
                                                        float eye_sign, float half_ipd, float* __restrict__ rays) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rays) return;
  const int s2 = ss * ss, Wo = c.W / ss;
  const int64_t q = i / s2;
  const int sub = (int)(i - q * s2), a = sub / ss, b = sub - a * ss;
  const int64_t p = first + q;
  const int orow = (int)(p / Wo), ocol = (int)(p - (int64_t)orow * Wo);
  const int row = orow * ss + a, col = ocol * ss + b;
  float o[6];
  camera_ray(c, pose, row, col, o);
  if (eye_sign != 0.f && half_ipd != 0.f) {   // (only with EGO_CAM_ERP: the entry point refuses the rest)
    const float phi = __fmul_rn(__fsub_rn(1.f, __fdiv_rn(__fmul_rn(2.f, (float)col + 0.5f), (float)c.W)), 3.14159265358979323846f);
    const float e = __fmul_rn(eye_sign, half_ipd);
    const float ex = __fmul_rn(e, cosf(phi)), ez = -__fmul_rn(e, sinf(phi));   // camera space: (ex, 0, ez)
#pragma unroll
    for (int r = 0; r < 3; ++r)   // o = R o_cam + t, the zero y term left out: (ex R_r0 + ez R_r2) + t_r
      o[r] = __fadd_rn(__fadd_rn(__fmul_rn(ex, pose[4 * r]), __fmul_rn(ez, pose[4 * r + 2])), pose[4 * r + 3]);
  }
  store_ray(rays, i, o);
}

struct FinishArgs {
  const float* rgb;       // [count][3]
  const float* depth;     // [count]
  int64_t first, count;
  int32_t W, side_by_side;
  float mi, den;
  const uint8_t* palette; // [256][3] or null
  uint8_t* rgb8;          // frame base: [n][3], or [H][2W][3] side by side
  uint8_t* depth8;        // frame base: [n][3] with a palette, [n] without; unused side by side
};

// (rgb.clamp(0, 1) * 255).astype('uint8') of renderer.py:227, :233: float32 multiply, truncation
__device__ __forceinline__ uint32_t quantise_colour(float v) {
  const float c = fminf(fmaxf(v, 0.f), 1.f);   // fmaxf(NaN, 0) = 0: a NaN colour, undefined in the reference's cast, becomes 0
  return (uint32_t)(int)__fmul_rn(c, 255.f);
}

// visualize_depth_numpy (utils.py:14-25): (255 * ((nan_to_num(depth) - mi) / den)).astype(uint8), saturated to [0, 255] where the
// reference's cast is undefined
__device__ __forceinline__ uint32_t depth_index(float d, float mi, float den) {
  float x = (d != d) ? 0.f : d;                                   // np.nan_to_num: NaN -> 0, +-inf -> +-FLT_MAX
  x = fminf(fmaxf(x, -3.402823466e+38f), 3.402823466e+38f);
  const float v = __fmul_rn(255.f, __fdiv_rn(__fsub_rn(x, mi), den));
  if (!(v >= 0.f)) return 0u;
  return v >= 255.f ? 255u : (uint32_t)(int)v;
}

// 12 bytes (four pixels of three channels) to `dst`: three whole words where `dst` is 4-byte aligned, bytes otherwise
__device__ __forceinline__ void store12(uint8_t* dst, const uint32_t b[12]) {
  if (((uintptr_t)dst & 3) == 0) {
#pragma unroll
    for (int w = 0; w < 3; ++w)
      ((uint32_t*)dst)[w] = b[4 * w] | (b[4 * w + 1] << 8) | (b[4 * w + 2] << 16) | (b[4 * w + 3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) dst[k] = (uint8_t)b[k];
  }
}

// One thread per group of four pixels [4 g, 4 g + 4) of the FRAME (not of the chunk), so a group's 12 output bytes start on a word of
// an aligned image wherever the chunk begins; a group cut by the chunk's ends or by the end of an image row (side by side: the two
// halves of an output row are not contiguous) is written pixel by pixel.
__global__ __launch_bounds__(256) void k_finish_frame(FinishArgs a) {
  const int64_t g = a.first / 4 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t p0 = g * 4, end = a.first + a.count;
  if (p0 >= end) return;
  const int64_t lo = p0 < a.first ? a.first : p0, hi = p0 + 4 > end ? end : p0 + 4;
  uint32_t c8[12], d8[12], idx[4];
  for (int64_t p = lo; p < hi; ++p) {
    const int k = (int)(p - p0);
    const int64_t s = p - a.first;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c8[3 * k + ch] = quantise_colour(a.rgb[s * 3 + ch]);
    idx[k] = depth_index(a.depth[s], a.mi, a.den);
    if (a.palette) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) d8[3 * k + ch] = a.palette[idx[k] * 3 + ch];
    }
  }
  const bool full = lo == p0 && hi == p0 + 4;
  if (a.side_by_side) {
    const int64_t row = p0 / a.W;
    const int col = (int)(p0 - row * a.W);
    uint8_t* left = a.rgb8 + (row * 2 * a.W + col) * 3;
    if (full && col + 4 <= a.W) {
      store12(left, c8);
      store12(left + (int64_t)a.W * 3, d8);
    } else {
      for (int64_t p = lo; p < hi; ++p) {
        const int k = (int)(p - p0);
        const int64_t r = p / a.W;
        uint8_t* l = a.rgb8 + (r * 2 * a.W + (p - r * a.W)) * 3;
        for (int ch = 0; ch < 3; ++ch) { l[ch] = (uint8_t)c8[3 * k + ch]; l[(int64_t)a.W * 3 + ch] = (uint8_t)d8[3 * k + ch]; }
      }
    }
    return;
  }
  if (full) {
    store12(a.rgb8 + p0 * 3, c8);
    if (a.palette) store12(a.depth8 + p0 * 3, d8);
    else if (((uintptr_t)a.depth8 & 3) == 0) ((uint32_t*)a.depth8)[g] = idx[0] | (idx[1] << 8) | (idx[2] << 16) | (idx[3] << 24);
    else for (int k = 0; k < 4; ++k) a.depth8[p0 + k] = (uint8_t)idx[k];
    return;
  }
  for (int64_t p = lo; p < hi; ++p) {
    const int k = (int)(p - p0);
    for (int ch = 0; ch < 3; ++ch) a.rgb8[p * 3 + ch] = (uint8_t)c8[3 * k + ch];
    if (a.palette) for (int ch = 0; ch < 3; ++ch) a.depth8[p * 3 + ch] = (uint8_t)d8[3 * k + ch];
    else a.depth8[p] = (uint8_t)idx[k];
  }
}

// Resolve and finish: ss x ss samples per output pixel -> the bytes k_finish_frame writes for their average.  ONE THREAD PER OUTPUT
// PIXEL of the frame (thread t of the launch is pixel (first / 4) * 4 + t, so the four lanes of an aligned lane quad hold one group of
// four frame pixels); a thread reads its ss^2 contiguous samples - 12 ss^2 bytes next to its neighbours' - sums clamp(rgb, 0, 1) and
// nan_to_num(depth) in sample order, divides by float(ss^2) and quantises as k_finish_frame does.  The quad then trades its packed
// bytes through cross-lane shuffles and lanes 0..2 store one whole word each of the group's 12 bytes (lane 0 the four index bytes)
// wherever k_finish_frame stores words; elsewhere every lane stores its own bytes.  No lane leaves before the shuffles.
struct ResolveArgs {
  FinishArgs f;   // f.rgb [count ss^2][3], f.depth [count ss^2]
  float n;      // float(ss^2), the divisor
};

// the 12 bytes v0 | v1 << 24 | v2 << 48 | v3 << 72 of four packed pixels (3 bytes each): word w of three
__device__ __forceinline__ uint32_t quad_word(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, int w) {
  return w == 0 ? (v0 | (v1 << 24)) : w == 1 ? ((v1 >> 8) | (v2 << 16)) : ((v2 >> 16) | (v3 << 8));
}

template <int SS>
__global__ __launch_bounds__(256) void k_resolve_frame(ResolveArgs r) {
  const FinishArgs& a = r.f;
  constexpr int S2 = SS * SS;
  const int64_t p = a.first / 4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x, end = a.first + a.count;
  const int64_t p0 = p & ~(int64_t)3;
  const int k = (int)(p - p0);
  const bool live = p >= a.first && p < end;
  uint32_t c = 0, d = 0, idx = 0;   // this pixel's colour bytes, depth colour bytes (packed b0 | b1 << 8 | b2 << 16) and depth index
  if (live) {
    const float* rgb = a.rgb + (p - a.first) * (3 * S2);
    const float* dep = a.depth + (p - a.first) * S2;
    float sum[3], ds;
#pragma unroll
    for (int s = 0; s < S2; ++s) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float v = fminf(fmaxf(rgb[3 * s + ch], 0.f), 1.f);   // fmaxf(NaN, 0) = 0, as quantise_colour
        sum[ch] = s == 0 ? v : __fadd_rn(sum[ch], v);
      }
      float x = dep[s];
      x = (x != x) ? 0.f : fminf(fmaxf(x, -3.402823466e+38f), 3.402823466e+38f);   // np.nan_to_num per sample
      ds = s == 0 ? x : __fadd_rn(ds, x);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c |= quantise_colour(__fdiv_rn(sum[ch], r.n)) << (8 * ch);
    idx = depth_index(__fdiv_rn(ds, r.n), a.mi, a.den);
    if (a.palette) d = a.palette[idx * 3] | ((uint32_t)a.palette[idx * 3 + 1] << 8) | ((uint32_t)a.palette[idx * 3 + 2] << 16);
  }
  uint32_t cq[4], dq[4], iq[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {   // lane j of this quad (width 4: lanes of other quads are never read)
    cq[j] = (uint32_t)__shfl((int)c, j, 4);
    dq[j] = (uint32_t)__shfl((int)d, j, 4);
    iq[j] = (uint32_t)__shfl((int)idx, j, 4);
  }
  if (!live) return;
  bool full = p0 >= a.first && p0 + 4 <= end;   // the same in the four lanes of a quad
  uint8_t *dst_c, *dst_d;                       // this PIXEL's three colour bytes / depth bytes
  if (a.side_by_side) {
    const int64_t row = p0 / a.W;
    const int col0 = (int)(p0 - row * a.W);
    full = full && col0 + 4 <= a.W;
    const int64_t rr = p / a.W;
    dst_c = a.rgb8 + (rr * 2 * a.W + (p - rr * a.W)) * 3;
    dst_d = dst_c + (int64_t)a.W * 3;
  } else {
    dst_c = a.rgb8 + p * 3;
    dst_d = a.palette ? a.depth8 + p * 3 : a.depth8 + p;
  }
  const bool three = a.side_by_side || a.palette;   // the depth product has three channels
  // a full group's 12 bytes begin at this pixel's address minus 3 k: the word test of store12, on the group's address
  if (full && (((uintptr_t)dst_c - 3 * k) & 3) == 0) {
    if (k < 3) ((uint32_t*)(dst_c - 3 * k))[k] = quad_word(cq[0], cq[1], cq[2], cq[3], k);
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) dst_c[ch] = (uint8_t)(c >> (8 * ch));
  }
  if (three) {
    if (full && (((uintptr_t)dst_d - 3 * k) & 3) == 0) {
      if (k < 3) ((uint32_t*)(dst_d - 3 * k))[k] = quad_word(dq[0], dq[1], dq[2], dq[3], k);
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) dst_d[ch] = (uint8_t)(d >> (8 * ch));
    }
  } else if (full && ((uintptr_t)a.depth8 & 3) == 0) {
    if (k == 0) ((uint32_t*)a.depth8)[p0 / 4] = iq[0] | (iq[1] << 8) | (iq[2] << 16) | (iq[3] << 24);
  } else {
    *dst_d = (uint8_t)idx;
  }
}

}  // namespace

extern "C" {

int ego_camera_rays(int32_t model, int32_t H, int32_t W, float fx, float fy, float cx, float cy, int32_t normalize, const float* c2w,
                    int64_t first, int64_t count, float* rays, void* stream) {
  EGO_TRACE("ego_camera_rays");
  EGO_REQUIRE(model == EGO_CAM_ERP || model == EGO_CAM_PINHOLE || model == EGO_CAM_PINHOLE_BLENDER, "camera_rays: unknown camera model");
  EGO_REQUIRE(H >= 1 && W >= 1, "camera_rays: H or W < 1");
  EGO_REQUIRE(first >= 0 && count >= 0 && first <= (int64_t)H * W && count <= (int64_t)H * W - first,
              "camera_rays: pixel window [first, first + count) outside the image");
  if (model != EGO_CAM_ERP) {
    EGO_REQUIRE(fx == fx && fy == fy && fx != 0.f && fy != 0.f && fabsf(fx) <= 3.402823466e+38f && fabsf(fy) <= 3.402823466e+38f,
                "camera_rays: a pinhole camera needs a finite, non-zero focal length (fx, fy)");
    EGO_REQUIRE(cx == cx && cy == cy, "camera_rays: NaN principal point");
  }
  if (count == 0) return EGO_OK;
  EGO_REQUIRE(c2w && rays, "camera_rays: null argument");
  EGO_REQUIRE(((uintptr_t)rays & 7) == 0 && ((uintptr_t)c2w & 3) == 0, "camera_rays: rays must be 8-byte, c2w 4-byte aligned");
  const CamArgs c{model, H, W, normalize, fx, fy, cx, cy};
  k_camera_rays<<<nblk(count, 256), 256, 0, (hipStream_t)stream>>>(c, c2w, first, count, rays);
  return ego_launch_status("k_camera_rays");
}

int ego_camera_rays_ex(int32_t model, int32_t H, int32_t W, float fx, float fy, float cx, float cy, int32_t normalize, const float* c2w,
                       int64_t first, int64_t count, int32_t eye, float half_ipd, int32_t ss, float* rays, void* stream) {
  EGO_TRACE("ego_camera_rays_ex");
  EGO_REQUIRE(model == EGO_CAM_ERP || model == EGO_CAM_PINHOLE || model == EGO_CAM_PINHOLE_BLENDER, "camera_rays_ex: unknown camera model");
  EGO_REQUIRE(H >= 1 && W >= 1, "camera_rays_ex: H or W < 1");
  EGO_REQUIRE(ss >= 1 && ss <= 4, "camera_rays_ex: ss outside 1..4");
  EGO_REQUIRE(H % ss == 0 && W % ss == 0, "camera_rays_ex: H and W (the fine camera's) must be multiples of ss");
  EGO_REQUIRE(eye == EGO_EYE_CENTRE || eye == EGO_EYE_LEFT || eye == EGO_EYE_RIGHT, "camera_rays_ex: unknown eye");
  EGO_REQUIRE(eye == EGO_EYE_CENTRE || model == EGO_CAM_ERP, "camera_rays_ex: a left or right eye needs the equirectangular camera");
  EGO_REQUIRE(half_ipd >= 0.f && half_ipd <= 3.402823466e+38f, "camera_rays_ex: half_ipd must be a finite number >= 0");
  const int64_t n_out = (int64_t)(H / ss) * (W / ss);
  EGO_REQUIRE(first >= 0 && count >= 0 && first <= n_out && count <= n_out - first,
              "camera_rays_ex: pixel window [first, first + count) outside the (H / ss) x (W / ss) frame");
  if (model != EGO_CAM_ERP) {
    EGO_REQUIRE(fx == fx && fy == fy && fx != 0.f && fy != 0.f && fabsf(fx) <= 3.402823466e+38f && fabsf(fy) <= 3.402823466e+38f,
                "camera_rays_ex: a pinhole camera needs a finite, non-zero focal length (fx, fy)");
    EGO_REQUIRE(cx == cx && cy == cy, "camera_rays_ex: NaN principal point");
  }
  if (count == 0) return EGO_OK;
  EGO_REQUIRE(c2w && rays, "camera_rays_ex: null argument");
  EGO_REQUIRE(((uintptr_t)rays & 7) == 0 && ((uintptr_t)c2w & 3) == 0, "camera_rays_ex: rays must be 8-byte, c2w 4-byte aligned");
  const CamArgs c{model, H, W, normalize, fx, fy, cx, cy};
  const int64_t n_rays = count * ss * ss;
  const float sign = eye == EGO_EYE_LEFT ? -1.f : eye == EGO_EYE_RIGHT ? 1.f : 0.f;
  k_camera_rays_ex<<<nblk(n_rays, 256), 256, 0, (hipStream_t)stream>>>(c, c2w, first, n_rays, ss, sign, half_ipd, rays);
  return ego_launch_status("k_camera_rays_ex");
}

int ego_finish_frame(const float* rgb, const float* depth, int64_t first, int64_t count, int32_t H, int32_t W, float mi, float den,
                     const uint8_t* palette, int32_t side_by_side, uint8_t* rgb8, uint8_t* depth8, void* stream) {
  EGO_TRACE("ego_finish_frame");
  EGO_REQUIRE(H >= 1 && W >= 1, "finish_frame: H or W < 1");
  EGO_REQUIRE(first >= 0 && count >= 0 && first <= (int64_t)H * W && count <= (int64_t)H * W - first,
              "finish_frame: pixel window [first, first + count) outside the image");
  EGO_REQUIRE(mi == mi && den == den && den != 0.f, "finish_frame: mi / den must be numbers, den non-zero");
  EGO_REQUIRE(!side_by_side || palette, "finish_frame: the side-by-side layout needs a palette (three-channel depth)");
  if (count == 0) return EGO_OK;
  EGO_REQUIRE(rgb && depth && rgb8 && (side_by_side || depth8), "finish_frame: null argument");
  FinishArgs a;
  a.rgb = rgb; a.depth = depth; a.first = first; a.count = count; a.W = W; a.side_by_side = side_by_side ? 1 : 0;
  a.mi = mi; a.den = den; a.palette = palette; a.rgb8 = rgb8; a.depth8 = depth8;
  const int64_t groups = (first + count + 3) / 4 - first / 4;
  k_finish_frame<<<nblk(groups, 256), 256, 0, (hipStream_t)stream>>>(a);
  return ego_launch_status("k_finish_frame");
}

int ego_resolve_frame(const float* rgb, const float* depth, int64_t first, int64_t count, int32_t H, int32_t W, int32_t ss, float mi,
                      float den, const uint8_t* palette, int32_t side_by_side, uint8_t* rgb8, uint8_t* depth8, void* stream) {
  EGO_TRACE("ego_resolve_frame");
  EGO_REQUIRE(H >= 1 && W >= 1, "resolve_frame: H or W < 1");
  EGO_REQUIRE(ss >= 1 && ss <= 4, "resolve_frame: ss outside 1..4");
  EGO_REQUIRE(first >= 0 && count >= 0 && first <= (int64_t)H * W && count <= (int64_t)H * W - first,
              "resolve_frame: pixel window [first, first + count) outside the image");
  EGO_REQUIRE(mi == mi && den == den && den != 0.f, "resolve_frame: mi / den must be numbers, den non-zero");
  EGO_REQUIRE(!side_by_side || palette, "resolve_frame: the side-by-side layout needs a palette (three-channel depth)");
  if (count == 0) return EGO_OK;
  EGO_REQUIRE(rgb && depth && rgb8 && (side_by_side || depth8), "resolve_frame: null argument");
  ResolveArgs r;
  FinishArgs& a = r.f;
  a.rgb = rgb; a.depth = depth; a.first = first; a.count = count; a.W = W; a.side_by_side = side_by_side ? 1 : 0;
  a.mi = mi; a.den = den; a.palette = palette; a.rgb8 = rgb8; a.depth8 = depth8;
  r.n = (float)(ss * ss);
  const unsigned blocks = nblk(first + count - first / 4 * 4, 256);   // one thread per pixel from the window's first group on
  hipStream_t st = (hipStream_t)stream;
  switch (ss) {
    case 1: k_resolve_frame<1><<<blocks, 256, 0, st>>>(r); break;
    case 2: k_resolve_frame<2><<<blocks, 256, 0, st>>>(r); break;
    case 3: k_resolve_frame<3><<<blocks, 256, 0, st>>>(r); break;
    default: k_resolve_frame<4><<<blocks, 256, 0, st>>>(r); break;
  }
  return ego_launch_status("k_resolve_frame");
}

}  // extern "C"
