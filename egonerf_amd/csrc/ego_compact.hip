// Live-sample list for ego_render_forward's compact path (models/tensorBase.py:480-487: app_mask = weight > rayMarch_weight_thres, the
// appearance lookup and the MLP then run on coords_sampled[app_mask] only).  Three launches on the caller's stream, no atomics, no host
// synchronisation, no allocation:
//   k_live_count    one wave per ray: ballot + popcount over the ray's [S] weights -> count[ray]; a block's 64 rays -> part[block]
//   k_live_scan     one workgroup: exclusive scan of part[] in place, total -> *n_live
//   k_live_scatter  one wave per ray again: block-local exclusive scan of count[], then ballot + mbcnt place every live sample
// The list comes out in (ray, sample) order, which is the order the tile path walks the same samples in.
#include "ego_device.h"
#include "ego_host.h"

namespace {

constexpr int LIVE_RPB = 64;            // rays per 256-thread workgroup of the count / scatter kernels (16 per wave)
constexpr int LIVE_SCAN_T = 1024;       // threads of the scan workgroup

__device__ __forceinline__ int wave_live_bits(const float* __restrict__ w, int64_t row, int32_t S, int s0, int lane, float above,
                                              unsigned long long& bits) {
  const int s = s0 + lane;
  const bool live = s < S && w[row + s] > above;
  bits = __ballot(live);
  return live;
}

__global__ __launch_bounds__(256) void k_live_count(const float* __restrict__ w, int64_t N, int32_t S, float above, int32_t* __restrict__ count,
                                                    int32_t* __restrict__ part) {
  __shared__ int32_t wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t mine = 0;   // this wave's total over its rays (wave-uniform)
  for (int i = 0; i < LIVE_RPB / 4; ++i) {
    const int64_t ray = (int64_t)blockIdx.x * LIVE_RPB + wave * (LIVE_RPB / 4) + i;
    if (ray >= N) break;
    int32_t c = 0;
    for (int s0 = 0; s0 < S; s0 += 64) {
      unsigned long long bits;
      wave_live_bits(w, ray * S, S, s0, lane, above, bits);
      c += __popcll(bits);
    }
    if (lane == 0) count[ray] = c;
    mine += c;
  }
  if (lane == 0) wsum[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive scan of part[0 .. nb) in place: thread t owns a contiguous run of ceil(nb / 1024) entries
__global__ __launch_bounds__(LIVE_SCAN_T) void k_live_scan(int32_t* __restrict__ part, int64_t nb, int32_t* __restrict__ n_live) {
  __shared__ int32_t sums[LIVE_SCAN_T];
  const int t = threadIdx.x;
  const int64_t per = (nb + LIVE_SCAN_T - 1) / LIVE_SCAN_T;
  const int64_t b0 = t * per, b1 = b0 + per < nb ? b0 + per : nb;
  int32_t run = 0;
  for (int64_t b = b0; b < b1; ++b) run += part[b];
  sums[t] = run;
  __syncthreads();
  for (int d = 1; d < LIVE_SCAN_T; d <<= 1) {   // Hillis-Steele over the 1024 run totals (inclusive)
    const int32_t v = t >= d ? sums[t - d] : 0;
    __syncthreads();
    sums[t] += v;
    __syncthreads();
  }
  int32_t off = t ? sums[t - 1] : 0;
  for (int64_t b = b0; b < b1; ++b) {
    const int32_t v = part[b];
    part[b] = off;
    off += v;
  }
  if (t == LIVE_SCAN_T - 1) *n_live = sums[t];
}

__global__ __launch_bounds__(256) void k_live_scatter(const float* __restrict__ w, int64_t N, int32_t S, float above,
                                                      const int32_t* __restrict__ count, const int32_t* __restrict__ part,
                                                      int32_t* __restrict__ live) {
  __shared__ int32_t base[LIVE_RPB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave == 0) {   // exclusive scan of the block's 64 ray counts, one lane per ray
    const int64_t ray = (int64_t)blockIdx.x * LIVE_RPB + lane;
    const int32_t c = ray < N ? count[ray] : 0;
    int32_t inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t v = __shfl_up(inc, d, 64);
      if (lane >= d) inc += v;
    }
    base[lane] = part[blockIdx.x] + inc - c;
  }
  __syncthreads();
  for (int i = 0; i < LIVE_RPB / 4; ++i) {
    const int r = wave * (LIVE_RPB / 4) + i;
    const int64_t ray = (int64_t)blockIdx.x * LIVE_RPB + r;
    if (ray >= N) break;
    int32_t pos = base[r];
    for (int s0 = 0; s0 < S; s0 += 64) {
      unsigned long long bits;
      const int me = wave_live_bits(w, ray * S, S, s0, lane, above, bits);
      const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bits >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bits, 0u));
      if (me) live[pos + below] = (int32_t)(ray * S + s0 + lane);
      pos += __popcll(bits);
    }
  }
}

}  // namespace

int64_t ego_live_blocks(int64_t N) { return (N + LIVE_RPB - 1) / LIVE_RPB; }

// weight [N][S] -> live [n_live] (sample indices ray * S + s with weight > above, ascending), count [N], part [ego_live_blocks(N)], *n_live
int ego_compact_live(const float* weight, int64_t N, int32_t S, float above, int32_t* live, int32_t* count, int32_t* part, int32_t* n_live,
                     void* stream) {
  EGO_REQUIRE(weight && live && count && part && n_live && N >= 1 && S >= 1 && N * (int64_t)S < (1ll << 31),
              "compact_live: null argument or N*S outside [1, 2^31)");
  const int64_t nb = ego_live_blocks(N);
  k_live_count<<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>(weight, N, S, above, count, part);
  if (int e = ego_launch_status("k_live_count")) return e;
  k_live_scan<<<1, LIVE_SCAN_T, 0, (hipStream_t)stream>>>(part, nb, n_live);
  if (int e = ego_launch_status("k_live_scan")) return e;
  k_live_scatter<<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>(weight, N, S, above, count, part, live);
  return ego_launch_status("k_live_scatter");
}

namespace {
// what ego_render_forward sent through the MLP: mode 2 = the live count, 1 = 32 x the active tiles (clipped at N S), 0 = N S
__global__ __launch_bounds__(1024) void k_shaded_count(int32_t mode, const int32_t* __restrict__ n_live, const uint8_t* __restrict__ act,
                                                       int64_t n_tiles, int64_t NS, int64_t* __restrict__ out) {
  __shared__ int64_t red[1024];
  int64_t c = 0;
  if (mode == 1)
    for (int64_t t = threadIdx.x; t < n_tiles; t += 1024) c += act[t] != 0;
  red[threadIdx.x] = c;
  __syncthreads();
  for (int d = 512; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int64_t tiles = red[0] * 32;
    *out = mode == 2 ? (int64_t)*n_live : mode == 1 ? (tiles < NS ? tiles : NS) : NS;
  }
}
}  // namespace

int ego_shaded_count(int32_t mode, const int32_t* n_live, const uint8_t* act, int64_t N, int32_t S, int64_t* out, void* stream) {
  const int64_t NS = N * (int64_t)S;
  k_shaded_count<<<1, 1024, 0, (hipStream_t)stream>>>(mode, n_live, act, (NS + 31) / 32, NS, out);
  return ego_launch_status("k_shaded_count");
}
