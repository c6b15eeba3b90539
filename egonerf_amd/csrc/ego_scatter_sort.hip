// libegonerf_hip.so, part 9a: the sort of the sorted table-gradient scatter.  The step's samples are binned by texel CELL once - three
// stable LSD radix sorts of (key, sample index), 9 bits per pass, all three sorts in the same launches - so that the scatters of
// ego_scatter_sorted.hip can write every gradient texel exactly once from sums taken in a fixed order.
//
//   ego_scatter_sort : coords -> three permutations + cell start offsets + line sub-block offsets + the walk's step lists.  It needs
//                      only the forward's coordinates: it runs on the side stream next to the dumping shade forward, and both fields
//                      (density, appearance) share its result.
//
// What a key is, which sort serves which plane and line, and where everything lies in the workspace is ego_sorted_geom.h, shared with
// the scatters; ego_scatter_sorted_workspace_bytes is here because the sort is the workspace's first user.

#include "ego_device.h"
#include "ego_host.h"
#include "ego_sorted_geom.h"

namespace {

// the unclamped west tap index + 1 (0 .. n) with lin_setup's arithmetic, or -1 when both taps are out of range
__device__ __forceinline__ int cell_of(float xhat, int n) {
  const float ix = __fmul_rn(__fadd_rn(xhat, 1.0f), 0.5f * (float)(n - 1));
  const float flc = fminf(fmaxf(floorf(ix), -2.0f), (float)n);
  const int i0 = (int)flc;
  return (i0 < -1 || i0 > n - 1) ? -1 : i0 + 1;
}

struct KeyArgs {
  uint32_t K[3], nb[3], bs[3];
};
// key of sort s = ((grid * nb + block of the third axis' cell) * (n_major + 1) + major cell) * (n_minor + 1) + minor cell; a sample
// without a gradient through the third axis (both taps out of range: its line weights are 0) goes to block 0
__global__ void k_sort_keys(const float* __restrict__ coords, int64_t M, int nr, int nth, int nph, KeyArgs A,
                            uint32_t* __restrict__ k0, uint32_t* __restrict__ k1, uint32_t* __restrict__ k2) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const f32x4 cc = ((const f32x4*)coords)[m];
  const uint32_t g = cc.w != 0.f ? 1u : 0u;
  const int cr = cell_of(cc.x, nr), cth = cell_of(cc.y, nth), cph = cell_of(cc.z, nph);
  const uint32_t b0 = cth < 0 ? 0u : (uint32_t)cth / A.bs[0], b1 = cph < 0 ? 0u : (uint32_t)cph / A.bs[1], b2 = cr < 0 ? 0u : (uint32_t)cr / A.bs[2];
  k0[m] = (cph < 0 || cr < 0) ? A.K[0] : ((g * A.nb[0] + b0) * (uint32_t)(nph + 1) + (uint32_t)cph) * (uint32_t)(nr + 1) + (uint32_t)cr;
  k1[m] = (cr < 0 || cth < 0) ? A.K[1] : ((g * A.nb[1] + b1) * (uint32_t)(nr + 1) + (uint32_t)cr) * (uint32_t)(nth + 1) + (uint32_t)cth;
  k2[m] = (cth < 0 || cph < 0) ? A.K[2] : ((g * A.nb[2] + b2) * (uint32_t)(nth + 1) + (uint32_t)cth) * (uint32_t)(nph + 1) + (uint32_t)cph;
}

// ---- stable LSD radix sort of (key, sample index), 9 bits per pass, the three sorts side by side (blockIdx.y) -----------------------
// Plain kernels (no look-back between workgroups, no library state): the whole sort is graph-capturable and bit-reproducible.  A pass =
//   k_radix_hist    : per 4096-element tile, the digit histogram (LDS integer atomics) -> hist[digit][tile]
//   k_radix_scan    : per digit, exclusive scan of its per-tile counts + the digit's total (the digit bases are a 512-value scan that every
//                     scatter workgroup does for itself): where each tile's run of each digit starts
//   k_radix_scatter : the tile again: every element's rank among the EARLIER elements of its digit (wave w owns elements [1024 w, 1024 w +
//                     1024) of the tile and walks them 64 at a time in order; inside an iteration the equal-digit lanes are found with 9
//                     ballots) -> stable position -> (key, value) stored
struct RadixArgs {
  const uint32_t* kin[3];
  const uint32_t* vin[3];    // nullptr: the value is the element's index (first pass)
  uint32_t* kout[3];
  uint32_t* vout[3];
  uint32_t* hist[3];
  uint32_t* dsum[3];         // [RADIX] per-digit totals of the pass
  int64_t M;
  uint32_t nblocks;
  int shift;
};

__global__ __launch_bounds__(256) void k_radix_hist(RadixArgs A) {
  __shared__ uint32_t h[RADIX];
  const int s = blockIdx.y, t = threadIdx.x;
  for (int i = t; i < RADIX; i += 256) h[i] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * RTILE;
#pragma unroll 4
  for (int j = 0; j < RTILE / 256; ++j) {
    const int64_t idx = base + j * 256 + t;
    if (idx < A.M) atomicAdd(&h[(A.kin[s][idx] >> A.shift) & (RADIX - 1)], 1u);
  }
  __syncthreads();
  for (int i = t; i < RADIX; i += 256) A.hist[s][(int64_t)i * A.nblocks + blockIdx.x] = h[i];
}

// exclusive scan of a workgroup's 256 values (one per thread); returns the thread's prefix, *total = the sum
__device__ __forceinline__ uint32_t block_excl_scan256(uint32_t v, uint32_t* wsum /* [4] shared */, uint32_t* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(inc, d, 64);
    if (lane >= d) inc += u;
  }
  __syncthreads();   // wsum may still be read from a previous call
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint32_t before = 0;
  for (int w = 0; w < wv; ++w) before += wsum[w];
  *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return before + inc - v;
}

// one workgroup per (digit, sort): in-place exclusive scan of the digit's per-tile counts; the digit's total goes to dsum[digit]
// (k_radix_scatter turns the 512 totals into digit bases itself)
__global__ __launch_bounds__(256) void k_radix_scan(RadixArgs A) {
  __shared__ uint32_t wsum[4];
  uint32_t* h = A.hist[blockIdx.y] + (int64_t)blockIdx.x * A.nblocks;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < A.nblocks; base += 256) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < A.nblocks ? h[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_excl_scan256(v, wsum, &total);
    if (i < A.nblocks) h[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) A.dsum[blockIdx.y][blockIdx.x] = carry;
}

__global__ __launch_bounds__(256) void k_radix_scatter(RadixArgs A) {
  __shared__ uint32_t wcnt[4][RADIX];
  __shared__ uint32_t lbase[RADIX], gbase[RADIX];   // where a digit's run starts inside the sorted tile / in the output
  __shared__ uint32_t skey[RTILE], sval[RTILE];     // the tile in sorted order: the output is then written in runs, not element by element
  __shared__ uint32_t wsum[4];
  const int s = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int i = t; i < 4 * RADIX; i += 256) (&wcnt[0][0])[i] = 0;
  __syncthreads();
  const int64_t tbase = (int64_t)blockIdx.x * RTILE, wbase = tbase + w * (RTILE / 4);
  uint32_t key[RTILE / 256];
#pragma unroll
  for (int it = 0; it < RTILE / 256; ++it) {
    const int64_t idx = wbase + it * 64 + lane;
    key[it] = idx < A.M ? A.kin[s][idx] : 0u;
    if (idx < A.M) atomicAdd(&wcnt[w][(key[it] >> A.shift) & (RADIX - 1)], 1u);
  }
  __syncthreads();
  {   // two digits per thread (2 t, 2 t + 1): the tile's digit starts, and the digit bases from the 512 digit totals of the pass
    const uint32_t c0 = wcnt[0][2 * t] + wcnt[1][2 * t] + wcnt[2][2 * t] + wcnt[3][2 * t];
    const uint32_t c1 = wcnt[0][2 * t + 1] + wcnt[1][2 * t + 1] + wcnt[2][2 * t + 1] + wcnt[3][2 * t + 1];
    uint32_t total;
    const uint32_t ex = block_excl_scan256(c0 + c1, wsum, &total);
    lbase[2 * t] = ex; lbase[2 * t + 1] = ex + c0;
    const uint32_t d0 = A.dsum[s][2 * t], d1 = A.dsum[s][2 * t + 1];
    const uint32_t exg = block_excl_scan256(d0 + d1, wsum, &total);
    gbase[2 * t] = exg + A.hist[s][(int64_t)(2 * t) * A.nblocks + blockIdx.x];
    gbase[2 * t + 1] = exg + d0 + A.hist[s][(int64_t)(2 * t + 1) * A.nblocks + blockIdx.x];
  }
  __syncthreads();
  for (int d = t; d < RADIX; d += 256) {   // counts -> where wave w's run of digit d starts in the sorted tile
    uint32_t run = lbase[d];
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) { const uint32_t c = wcnt[ww][d]; wcnt[ww][d] = run; run += c; }
  }
  __syncthreads();
  const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
#pragma unroll
  for (int it = 0; it < RTILE / 256; ++it) {
    const int64_t idx = wbase + it * 64 + lane;
    const bool ok = idx < A.M;
    const uint32_t d = (key[it] >> A.shift) & (RADIX - 1);
    unsigned long long m = __ballot(ok);
#pragma unroll
    for (int b = 0; b < RBITS; ++b) {
      const unsigned long long bal = __ballot(ok && ((d >> b) & 1u));
      m &= ((d >> b) & 1u) ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(m & lt);
    uint32_t off = 0;
    if (ok) off = wcnt[w][d];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (ok && rank == 0) wcnt[w][d] = off + (uint32_t)__popcll(m);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (ok) {
      skey[off + rank] = key[it];
      sval[off + rank] = A.vin[s] ? A.vin[s][idx] : (uint32_t)idx;
    }
  }
  __syncthreads();
  const int n_tile = (int)(A.M - tbase < RTILE ? A.M - tbase : RTILE);
  for (int i = t; i < n_tile; i += 256) {
    const uint32_t k = skey[i], d = (k >> A.shift) & (RADIX - 1);
    const uint32_t pos = gbase[d] + ((uint32_t)i - lbase[d]);
    A.kout[s][pos] = k;
    A.vout[s][pos] = sval[i];
  }
}

// start[k] = first sorted position whose key is >= k, k = 0 .. K + 1 (start[K] = the number of samples with a gradient)
struct StartArgs {
  const uint32_t* sorted[3];
  uint32_t* start[3];
  uint32_t* suboff[3];
  uint32_t* stepsum[3];
  uint32_t* costsum[3];
  uint4* steps[3];
  uint32_t* scanpart[3];   // k_step_scan's per-workgroup totals
  uint32_t K[3], LC[3], nmin1[3];
  int64_t M;
};

__global__ void k_cell_starts(StartArgs A) {
  const uint32_t* __restrict__ sorted = A.sorted[blockIdx.y];
  uint32_t* __restrict__ start = A.start[blockIdx.y];
  const uint32_t K = A.K[blockIdx.y];
  const int64_t M = A.M;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > K + 1) return;
  int64_t lo = 0, hi = M;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted[mid] < k) lo = mid + 1; else hi = mid;
  }
  start[k] = (uint32_t)lo;
}

// suboff[lc] = number of 256-sample sub-blocks of the line cells before lc (exclusive scan; suboff[LC] = total); one workgroup
__global__ __launch_bounds__(1024) void k_line_suboff(StartArgs A) {
  const uint32_t* __restrict__ start = A.start[blockIdx.y];
  uint32_t* __restrict__ suboff = A.suboff[blockIdx.y];
  const uint32_t LC = A.LC[blockIdx.y], nmin1 = A.nmin1[blockIdx.y];
  __shared__ uint32_t wsum[16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < LC; base += 1024) {
    const uint32_t lc = base + t;
    uint32_t n = 0;
    if (lc < LC) n = (start[(lc + 1) * nmin1] - start[lc * nmin1] + SUB - 1) / SUB;
    uint32_t inc = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t v = __shfl_up(inc, d, 64);
      if (lane >= d) inc += v;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wv; ++w) before += wsum[w];
    uint32_t all = 0;
    for (int w = 0; w < 16; ++w) all += wsum[w];
    if (lc < LC) suboff[lc] = carry + before + inc - n;
    carry += all;
    __syncthreads();
  }
  if (t == 0) suboff[LC] = carry;
}

// ---- the walk's step list -------------------------------------------------------------------------------------------------------------
// A STEP = up to 16 consecutive sorted samples of one cell (what a 16-lane group of k_sorted_walk handles at a time).
// stepsum[k] = number of steps of the cells before k (k = 0 .. K; the cells of grid 0 come first), one workgroup per sort;
// steps[j] = {first sorted position, cell, samples | first step of its cell << 8 | last << 9, 0}.  With the list the walk is dealt in
// EQUAL numbers of steps per group, whatever the cells' sizes - a first version that dealt cells in chunks had its slowest wave at 3.5 x
// the mean (tools/sorted_probe.py PROBE_PROF on a -DEGO_WALK_PROF build).
// cost of a cell's steps: a step = its fixed part (prefetches, set-up, record: 0.6 of an iteration's time, measured with
// -DEGO_WALK_PROF: 3.2 k against 5.3 k clocks in the 48-channel walk) + ceil(samples / 4) stage-2 iterations (U = 4 samples per group)
__device__ __forceinline__ uint32_t cell_cost(uint32_t n) {   // in fifths of an iteration: a step's fixed part = 3, an iteration = 5
  const uint32_t full = n / 16u, r = n % 16u;
  return full * 23u + (r ? 3u + 5u * ((r + 3u) / 4u) : 0u);
}

// stepsum / costsum = exclusive prefix sums over the sort's cells, in three launches: per 4096-cell workgroup the local prefixes + its
// total (PHASE 0), the totals' scan by one workgroup (1), the offsets added (2).  blockIdx.y = 0 steps, 1 cost; z = sort.  (A
// single-workgroup loop took 0.1 ms.)
template <int PHASE>
__global__ __launch_bounds__(1024) void k_step_scan(StartArgs A) {
  const int s = blockIdx.z;
  const uint32_t* __restrict__ start = A.start[s];
  const bool cost = blockIdx.y == 1;
  uint32_t* __restrict__ out = cost ? A.costsum[s] : A.stepsum[s];
  uint32_t* __restrict__ part = A.scanpart[s] + (cost ? (A.K[s] / 4096u + 2u) : 0u);
  const uint32_t K = A.K[s], nblk = (K + 4095u) / 4096u;
  __shared__ uint32_t wsum[16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (PHASE == 1) {   // one workgroup: exclusive scan of the workgroup totals, the grand total behind them
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nblk; base += 1024) {
      const uint32_t i = base + (uint32_t)t;
      const uint32_t v = i < nblk ? part[i] : 0u;
      uint32_t inc = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(inc, d, 64); if (lane >= d) inc += u; }
      if (lane == 63) wsum[wv] = inc;
      __syncthreads();
      uint32_t before = 0, all = 0;
      for (int w = 0; w < 16; ++w) { if (w < wv) before += wsum[w]; all += wsum[w]; }
      if (i < nblk) part[i] = carry + before + inc - v;
      carry += all;
      __syncthreads();
    }
    if (t == 0) { out[K] = carry; out[K + 1] = carry; }
    return;
  }
  if (blockIdx.x >= nblk) return;
  const uint32_t k0 = blockIdx.x * 4096u + 4u * (uint32_t)t;
  if (PHASE == 2) {
    const uint32_t off = part[blockIdx.x];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (k0 + i < K) out[k0 + i] += off;
    return;
  }
  uint32_t n[4], own = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t k = k0 + i;
    const uint32_t ns = k < K ? start[k + 1] - start[k] : 0u;
    n[i] = cost ? cell_cost(ns) : (ns + 15u) / 16u;
    own += n[i];
  }
  uint32_t inc = own;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(inc, d, 64); if (lane >= d) inc += u; }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int w = 0; w < 16; ++w) { if (w < wv) before += wsum[w]; all += wsum[w]; }
  uint32_t run = before + inc - own;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (k0 + i < K) out[k0 + i] = run;
    run += n[i];
  }
  if (t == 0) part[blockIdx.x] = all;
}

__global__ void k_step_fill(StartArgs A) {
  const int s = blockIdx.y;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= A.K[s]) return;
  const uint32_t c = k;
  const uint32_t a = A.start[s][c], n = A.start[s][c + 1] - a;
  if (!n) return;
  uint4* out = A.steps[s] + A.stepsum[s][k];
  const uint32_t nb = (n + 15u) / 16u;
  for (uint32_t b = 0; b < nb; ++b) {
    const uint32_t cnt = min(16u, n - 16u * b);
    out[b] = uint4{a + 16u * b, c, cnt | (b == 0 ? 256u : 0u) | (b + 1 == nb ? 512u : 0u), 0u};
  }
}

}  // namespace

extern "C" {

int64_t ego_scatter_sorted_workspace_bytes(const ego_scene* sc, int64_t N, int32_t S) {
  if (check_sizes(sc, N, S, "scatter_sorted_workspace_bytes")) return -1;
  return make_geom(sc->density.res, N * (int64_t)S > 0 ? N * (int64_t)S : 1).total;
}

int ego_scatter_sort(const ego_scene* sc, const float* coords, int64_t N, int32_t S, void* workspace, int64_t workspace_bytes, void* stream) {
  EGO_TRACE("ego_scatter_sort");
  if (int e = check_sizes(sc, N, S, "scatter_sort")) return e;
  if (N == 0) return EGO_OK;
  EGO_REQUIRE(coords && workspace && ((uintptr_t)workspace & 255) == 0, "scatter_sort: null argument or workspace not 256-byte aligned");
  for (int a = 0; a < 3; ++a)
    EGO_REQUIRE(sc->app.res[a] == sc->density.res[a], "scatter_sort: the density and appearance fields must share one resolution (they do: EgoNeRF.py:102-122)");
  const int64_t M = N * (int64_t)S;
  const SortGeom G = make_geom(sc->density.res, M);
  if (workspace_bytes < G.total) return ego_fail(EGO_E_BADARG, "scatter_sort: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)G.total);
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)workspace;
  uint32_t* kin[3] = {(uint32_t*)(base + G.keys_in[0]), (uint32_t*)(base + G.keys_in[1]), (uint32_t*)(base + G.keys_in[2])};
  KeyArgs ka{};
  for (int s = 0; s < 3; ++s) { ka.K[s] = G.K[s]; ka.nb[s] = G.nb[s]; ka.bs[s] = G.bs[s]; }
  k_sort_keys<<<(unsigned)((M + 255) / 256), 256, 0, st>>>(coords, M, G.res[0], G.res[1], G.res[2], ka, kin[0], kin[1], kin[2]);
  if (int e = ego_launch_status("k_sort_keys")) return e;
  // LSD passes ping-pong between (k1, v1) and (k2, perm); the last pass lands in (k2, perm)
  for (int p = 0; p < G.passes; ++p) {
    RadixArgs r{};
    const bool to2 = ((G.passes - 1 - p) & 1) == 0;
    for (int s = 0; s < 3; ++s) {
      r.kin[s] = p == 0 ? kin[s] : (const uint32_t*)(base + (to2 ? G.k1[s] : G.k2[s]));
      r.vin[s] = p == 0 ? nullptr : (const uint32_t*)(base + (to2 ? G.v1[s] : G.perm[s]));
      r.kout[s] = (uint32_t*)(base + (to2 ? G.k2[s] : G.k1[s]));
      r.vout[s] = (uint32_t*)(base + (to2 ? G.perm[s] : G.v1[s]));
      r.hist[s] = (uint32_t*)(base + G.hist[s]);
      r.dsum[s] = r.hist[s] + (int64_t)RADIX * G.nblocks;
    }
    r.M = M; r.nblocks = G.nblocks; r.shift = p * RBITS;
    k_radix_hist<<<dim3(G.nblocks, 3), 256, 0, st>>>(r);
    if (int e = ego_launch_status("k_radix_hist")) return e;
    k_radix_scan<<<dim3(RADIX, 3), 256, 0, st>>>(r);
    if (int e = ego_launch_status("k_radix_scan")) return e;
    k_radix_scatter<<<dim3(G.nblocks, 3), 256, 0, st>>>(r);
    if (int e = ego_launch_status("k_radix_scatter")) return e;
  }
  StartArgs sa{};
  for (int s = 0; s < 3; ++s) {
    sa.sorted[s] = (const uint32_t*)(base + G.k2[s]);
    sa.start[s] = (uint32_t*)(base + G.start[s]);
    sa.suboff[s] = (uint32_t*)(base + G.suboff[s]);
    sa.stepsum[s] = (uint32_t*)(base + G.stepsum[s]);
    sa.costsum[s] = (uint32_t*)(base + G.costsum[s]);
    sa.steps[s] = (uint4*)(base + G.steps[s]);
    sa.K[s] = G.K[s]; sa.LC[s] = G.LC[s]; sa.nmin1[s] = (uint32_t)G.res[sort_minor(s)] + 1;
  }
  sa.M = M;
  k_cell_starts<<<dim3((G.kmax + 2 + 255) / 256, 3), 256, 0, st>>>(sa);
  if (int e = ego_launch_status("k_cell_starts")) return e;
  k_line_suboff<<<dim3(1, 3), 1024, 0, st>>>(sa);
  if (int e = ego_launch_status("k_line_suboff")) return e;
  for (int s = 0; s < 3; ++s) sa.scanpart[s] = (uint32_t*)(base + G.scanpart[s]);
  {
    const unsigned nblk = (G.kmax + 4095) / 4096;
    k_step_scan<0><<<dim3(nblk, 2, 3), 1024, 0, st>>>(sa);
    if (int e = ego_launch_status("k_step_scan<0>")) return e;
    k_step_scan<1><<<dim3(1, 2, 3), 1024, 0, st>>>(sa);
    if (int e = ego_launch_status("k_step_scan<1>")) return e;
    k_step_scan<2><<<dim3(nblk, 2, 3), 1024, 0, st>>>(sa);
    if (int e = ego_launch_status("k_step_scan<2>")) return e;
  }
  k_step_fill<<<dim3((G.kmax + 255) / 256, 3), 256, 0, st>>>(sa);
  if (int e = ego_launch_status("k_step_fill")) return e;
  return EGO_OK;
}

}  // extern "C"
