// libegonerf_hip.so: inverse-CDF resampling + sort (row I of SURVEY 8a), one workgroup or one wave per ray.  gfx950 only.
// dataLoader/ray_utils.py:156-187 and models/EgoNeRF.py:532-542
//
// Two kernels, one body: every step below is written once and walks its items as (first index, stride) - (thread, 256) in the
// workgroup kernel, (lane, 64) in the wave kernel - with the kernel's own barrier handed in where a step synchronises.  So the two
// evaluate the same arithmetic in the same order by construction.  The kernels keep their LDS layout, the grouping of the
// normaliser's sum and what they do with an unsorted run.
#include "ego_device.h"
#include "ego_host.h"

#define PDF_MAX 2048            // Sc + n_fine of the workgroup kernel
constexpr int PDFW_MAX = 256;   // Sc and n_fine of the wave kernel

// cdf[0] = 0, cdf[i + 1] = cumsum(value(i)) over the nw = Sc - 2 pdf entries (w[1 + i] + 1e-5) / sum, by ONE wave: 64-wide scan with carry.
// sum(w + 1e-5) and the cdf are accumulated in double and rounded to float per element, like ATen's CPU
// sum/cumsum (acc_type<float> = double): the inverse CDF is discontinuous at u == 1 when the last bin is
// thinner than 1e-5, so the rounding of cdf[-1] is observable
template <class Value>
__device__ __forceinline__ void pdf_cdf_scan(float* cdf, int nw, int lane, Value value) {
  double carry = 0.0;
  for (int s0 = 0; s0 < nw; s0 += 64) {
    const int i = s0 + lane;
    double v = (i < nw) ? (double)value(i) : 0.0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double o = __shfl_up(v, d, 64);
      if (lane >= d) v += o;
    }
    if (i < nw) cdf[i + 1] = (float)(carry + v);
    carry += __shfl(v, 63, 64);
  }
  if (lane == 0) cdf[0] = 0.f;
}

// u of fine sample j: the caller's, or torch.linspace(0, 1, n) in float32: symmetric evaluation from both ends
__device__ __forceinline__ float pdf_u(const float* __restrict__ u_in, int64_t ray, int j, int n_fine) {
  if (u_in) return u_in[ray * n_fine + j];
  const float step = __fdiv_rn(1.f, (float)(n_fine - 1));
  return (n_fine == 1) ? 0.f : (j < n_fine / 2 ? __fmul_rn(step, (float)j) : __fsub_rn(1.f, __fmul_rn(step, (float)(n_fine - 1 - j))));
}

// the inverse CDF at u over the nb = Sc - 1 bins whose edges are the midpoints of zr
__device__ __forceinline__ float pdf_invert(const float* cdf, const float* __restrict__ zr, int nb, float u) {
  int lo = 0, hi = nb;  // searchsorted right over cdf[0..nb-1]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (!(cdf[mid] > u)) lo = mid + 1; else hi = mid;
  }
  const int below = max(lo - 1, 0), above = min(lo, nb - 1);
  const float c0 = cdf[below], c1 = cdf[above];
  const float b0 = 0.5f * __fadd_rn(zr[below + 1], zr[below]);
  const float b1 = 0.5f * __fadd_rn(zr[above + 1], zr[above]);
  float den = __fsub_rn(c1, c0);
  if (den < 1e-5f) den = 1.f;
  const float t = __fdiv_rn(__fsub_rn(u, c0), den);
  return __fadd_rn(b0, __fmul_rn(t, __fsub_rn(b1, b0)));
}

// keys = [coarse run zr[0..Sc) if use_coarse | fine run: the n_fine inverse-CDF samples], the fine run also to z_new
__device__ __forceinline__ void pdf_fill_keys(float* keys, const float* cdf, const float* __restrict__ zr, const float* __restrict__ u_in,
                                              int64_t ray, int Sc, int n_fine, int use_coarse, float* __restrict__ z_new_out, int first, int stride) {
  for (int j = first; j < n_fine; j += stride) {
    const float zs = pdf_invert(cdf, zr, Sc - 1, pdf_u(u_in, ray, j, n_fine));
    keys[(use_coarse ? Sc : 0) + j] = zs;
    if (z_new_out) z_new_out[ray * n_fine + j] = zs;
  }
  if (use_coarse)
    for (int i = first; i < Sc; i += stride) keys[i] = zr[i];
}

// does the run keys[base .. base + n) have an inversion (among the pairs this thread looks at)
__device__ __forceinline__ bool pdf_inverted(const float* keys, int base, int n, int first, int stride) {
  bool inv = false;
  for (int j = first; j + 1 < n; j += stride) inv |= keys[base + j] > keys[base + j + 1];
  return inv;
}

// In eval mode u is a linspace, so the fine samples come out non-decreasing, and the coarse schedule always is: the sort is then
// a merge of two sorted runs — every key finds its output slot with one binary search in the other run (stable: coarse keys
// before equal fine ones) — instead of 36 barrier-separated bitonic stages.  Sortedness is checked by the callers, not assumed
// (training draws random u; rounding may invert neighbours by an ulp).
// keys = two sorted runs (or the fine run alone) -> the ray's row of z_out; outk: n_out floats of scratch
template <class Sync>
__device__ __forceinline__ void pdf_merge_out(const float* keys, float* outk, int Sc, int n_fine, int use_coarse, float* __restrict__ z_out,
                                              int64_t ray, int first, int stride, Sync sync) {
  const int n_out = use_coarse ? Sc + n_fine : n_fine;
  if (!use_coarse) {
    for (int i = first; i < n_out; i += stride) z_out[ray * n_out + i] = keys[i];
    return;
  }
  for (int i = first; i < Sc; i += stride) {
    const float v = keys[i];
    int lo = 0, hi = n_fine;  // number of fine keys < v
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[Sc + mid] < v) lo = mid + 1; else hi = mid; }
    outk[i + lo] = v;
  }
  for (int j = first; j < n_fine; j += stride) {
    const float v = keys[Sc + j];
    int lo = 0, hi = Sc;      // number of coarse keys <= v
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] <= v) lo = mid + 1; else hi = mid; }
    outk[j + lo] = v;
  }
  sync();
  for (int i = first; i < n_out; i += stride) z_out[ray * n_out + i] = outk[i];
}

__device__ __forceinline__ int pdf_pow2(int n) {
  int P = 1;
  while (P < n) P <<= 1;
  return P;
}

// bitonic network over buf[0..P), P a power of two (the callers pad with +inf); the callers have synchronised the keys in
template <class Sync>
__device__ __forceinline__ void pdf_bitonic(float* buf, int P, int first, int stride, Sync sync) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = first; i < P; i += stride) {
        const int l = i ^ j;
        if (l > i) {
          const float a = buf[i], b = buf[l];
          const bool up = (i & k) == 0;
          if ((a > b) == up) { buf[i] = b; buf[l] = a; }
        }
      }
      sync();
    }
}

// One workgroup (256 threads) per ray, Sc + n_fine <= PDF_MAX.  Any inversion sends ALL keys through the bitonic network.
__global__ __launch_bounds__(256) void k_sample_pdf_merge(const float* __restrict__ z, const float* __restrict__ weight,
                                                          const float* __restrict__ u_in, int Sc, int n_fine,
                                                          int use_coarse, float* __restrict__ z_out,
                                                          float* __restrict__ z_new_out) {
  __shared__ float cdf[PDF_MAX];   // [Sc-1] entries: 0, cumsum(pdf)
  __shared__ float keys[PDF_MAX];  // sort buffer
  __shared__ double red[256];
  const int64_t ray = blockIdx.x;
  const int tid = threadIdx.x;
  const float* zr = z + ray * Sc;
  const float* wr = weight + ray * Sc;
  const int nw = Sc - 2;
  const int n_out = use_coarse ? Sc + n_fine : n_fine;
  const auto sync = [] { __syncthreads(); };
  double part = 0.0;
  for (int i = tid; i < nw; i += 256) part += (double)__fadd_rn(wr[1 + i], 1e-5f);
  red[tid] = part;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  const float total = (float)red[0];
  for (int i = tid; i < nw; i += 256) keys[i] = __fdiv_rn(__fadd_rn(wr[1 + i], 1e-5f), total);
  __syncthreads();
  if (tid < 64) pdf_cdf_scan(cdf, nw, tid, [&](int i) { return keys[i]; });
  __syncthreads();
  pdf_fill_keys(keys, cdf, zr, u_in, ray, Sc, n_fine, use_coarse, z_new_out, tid, 256);
  __syncthreads();
  bool inv = pdf_inverted(keys, use_coarse ? Sc : 0, n_fine, tid, 256);
  if (use_coarse) inv |= pdf_inverted(keys, 0, Sc, tid, 256);
  if (!__syncthreads_or(inv)) {
    pdf_merge_out(keys, cdf /* no longer needed */, Sc, n_fine, use_coarse, z_out, ray, tid, 256, sync);
    return;
  }
  // bitonic sort of n_out keys padded to a power of two with +inf
  const int P = pdf_pow2(n_out);
  for (int i = n_out + tid; i < P; i += 256) keys[i] = __int_as_float(0x7f800000);
  __syncthreads();
  pdf_bitonic(keys, P, tid, 256, sync);
  for (int i = tid; i < n_out; i += 256) z_out[ray * n_out + i] = keys[i];
}

// One WAVE per ray (four rays per workgroup) for Sc, n_fine <= PDFW_MAX - every shipped configuration (128 + 128): no workgroup
// barriers (the workgroup form has ~15 on its path and leaves half of its 256 threads without an item at Sc = 128), four times as
// many rays in flight per CU.  What differs from the workgroup kernel: the grouping of the double-precision sum of the pdf
// normaliser (per-lane partials + butterfly instead of 256 partials + tree): it is rounded to float once, so the two agree unless
// the double sum lands within 2^-29 ulp of a float rounding boundary.  And when the fine samples come out unsorted (random u in
// training) only THEY are sorted (bitonic in LDS, wave-synchronous) and then merged with the coarse run; equal keys are equal
// values, so the result is the sort's.
__global__ __launch_bounds__(256) void k_sample_pdf_merge_w(const float* __restrict__ z, const float* __restrict__ weight,
                                                            const float* __restrict__ u_in, int64_t N, int Sc, int n_fine,
                                                            int use_coarse, float* __restrict__ z_out,
                                                            float* __restrict__ z_new_out) {
  __shared__ float s_cdf[4][PDFW_MAX];
  __shared__ float s_keys[4][2 * PDFW_MAX];
  __shared__ float s_out[4][2 * PDFW_MAX];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * 4 + wv;
  if (ray >= N) return;
  float* cdf = s_cdf[wv];
  float* keys = s_keys[wv];
  float* outk = s_out[wv];
  const float* zr = z + ray * Sc;
  const float* wr = weight + ray * Sc;
  const int nw = Sc - 2;
  const int n_out = use_coarse ? Sc + n_fine : n_fine;
  const int base_f = use_coarse ? Sc : 0;
  const auto sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  double part = 0.0;
  for (int i = lane; i < nw; i += 64) part += (double)__fadd_rn(wr[1 + i], 1e-5f);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
  const float total = (float)part;
  pdf_cdf_scan(cdf, nw, lane, [&](int i) { return __fdiv_rn(__fadd_rn(wr[1 + i], 1e-5f), total); });
  sync();
  pdf_fill_keys(keys, cdf, zr, u_in, ray, Sc, n_fine, use_coarse, z_new_out, lane, 64);
  sync();
  const bool any_f = __ballot(pdf_inverted(keys, base_f, n_fine, lane, 64)) != 0ull;
  const bool any_c = __ballot(use_coarse && pdf_inverted(keys, 0, Sc, lane, 64)) != 0ull;
  // sort a run of n keys at keys[base ..) in place: bitonic network over the next power of two (padding +inf lives in outk)
  const auto sort_run = [&](int base, int n) {
    const int P = pdf_pow2(n);   // <= 2 * PDFW_MAX
    for (int i = lane; i < P; i += 64) outk[i] = i < n ? keys[base + i] : __int_as_float(0x7f800000);
    sync();
    pdf_bitonic(outk, P, lane, 64, sync);
    for (int i = lane; i < n; i += 64) keys[base + i] = outk[i];
    sync();
  };
  if (any_c) {            // never seen (the coarse schedule is monotone); kept for safety: sort everything
    sort_run(0, n_out);
    for (int i = lane; i < n_out; i += 64) z_out[ray * n_out + i] = keys[i];
    return;
  }
  if (any_f) sort_run(base_f, n_fine);
  pdf_merge_out(keys, outk, Sc, n_fine, use_coarse, z_out, ray, lane, 64, sync);
}

extern "C" {

int ego_sample_pdf_merge(const float* z, const float* weight, const float* u, int64_t N, int32_t Sc, int32_t n_fine,
                         int32_t use_coarse, float* z_out, float* z_new_out, void* stream) {
  EGO_TRACE("ego_sample_pdf_merge");
  EGO_REQUIRE(z && weight && z_out && N >= 0, "sample_pdf_merge: null argument");
  EGO_REQUIRE(Sc >= 3 && n_fine >= 1 && Sc + n_fine <= PDF_MAX, "sample_pdf_merge: need 3 <= Sc, Sc + n_fine <= 2048");
  if (N == 0) return EGO_OK;
  if (Sc <= PDFW_MAX && n_fine <= PDFW_MAX)   // every shipped configuration: one wave per ray
    k_sample_pdf_merge_w<<<(unsigned)((N + 3) / 4), 256, 0, (hipStream_t)stream>>>(z, weight, u, N, Sc, n_fine, use_coarse, z_out, z_new_out);
  else
    k_sample_pdf_merge<<<(unsigned)N, 256, 0, (hipStream_t)stream>>>(z, weight, u, Sc, n_fine, use_coarse, z_out, z_new_out);
  return ego_launch_status("k_sample_pdf_merge");
}

}  // extern "C"
