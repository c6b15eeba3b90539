// The geometry of the sorted table-gradient scatter: what ego_scatter_sort.hip (the sort: samples -> three permutations, cell starts and
// the walk's step lists) and ego_scatter_sorted.hip (the scatters that consume them) must agree on, and nothing else - the constants,
// which sort serves which plane and line, the workspace layout (SortGeom / make_geom), and the plan of which lines ride along in the
// walk (line_blocks / fused_plan).  Every "does this line window fit the LDS" decision goes through line_window_fits().
#pragma once
#include "ego_host.h"
#include <stdint.h>
#include <stdlib.h>

constexpr int SUB = 256;       // samples per line sub-block
constexpr int RBITS = 9, RADIX = 1 << RBITS, RTILE = 4096;   // radix sort: digit bits, buckets, elements per workgroup tile (256 threads x 16)
constexpr int CMAX = 48;       // channels of the widest field (appearance)
constexpr int FUSED_MAX_WG = 320;   // workgroups of a fused launch (one per CU: 256 on MI355X; room for a larger part)

// sort s: major / minor axis of its key (0 r, 1 theta, 2 phi), the plane whose cells it bins and the line whose ranges it bins
//   sort 0: key (grid, phi cell, r cell)     -> cells of plane 1 (x = r, y = phi), ranges of line 0 (phi)
//   sort 1: key (grid, r cell, theta cell)   -> cells of plane 0 (x = r, y = theta), ranges of line 2 (r)
//   sort 2: key (grid, theta cell, phi cell) -> cells of plane 2 (x = theta, y = phi), ranges of line 1 (theta)
// a cell = the unclamped west tap index + 1 (0 .. n); a sample whose two taps of an axis are both out of range has no gradient through
// that axis and sorts behind everything else
__host__ __device__ constexpr int sort_major(int s) { return s == 0 ? 2 : s == 1 ? 0 : 1; }
__host__ __device__ constexpr int sort_minor(int s) { return s == 0 ? 0 : s == 1 ? 1 : 2; }
__host__ __device__ constexpr int sort_plane(int s) { return s == 0 ? 1 : s == 1 ? 0 : 2; }
__host__ __device__ constexpr int sort_line(int s) { return s == 0 ? 0 : s == 1 ? 2 : 1; }

struct SortGeom {
  int32_t res[3];      // N_r, N_theta, N_phi
  int64_t M;
  uint32_t K[3];       // keys per sort = 2 (n_major + 1) (n_minor + 1); key K = "no gradient through this pair of axes"
  uint32_t kmax;       // the largest K
  uint32_t LC[3];      // line cells per sort = 2 (n_major + 1)
  uint32_t nsub_max;   // upper bound of the line sub-blocks of one sort
  int bits;            // key bits (covers max K)
  // byte offsets into the workspace
  int64_t perm[3], start[3], suboff[3], scratch, total;
  int64_t stepsum[3], steps[3];   // the walk's step list: per cell the number of 16-sample steps before it; the steps themselves
  int64_t costsum[3];             // per cell the COST of the steps before it (what the walk is dealt by)
  // line blocks: sort s's key carries, above its two plane axes, the BLOCK of the sample's cell along the third axis (nb[s]
  // blocks of bs[s] cells), so that a workgroup of the walk needs only one block's texels of the fused line in LDS
  uint32_t nb[3], bs[3], kc[3];   // kc = cells of one (grid, block): (n_major + 1) (n_minor + 1)
  int64_t step_cap[3];            // entries of steps[s]
  // sort-phase view of the scratch region
  int64_t keys_in[3], k1[3], v1[3], k2[3], hist[3], scanpart[3];
  uint32_t nblocks;    // radix tiles (RTILE elements each)
  int passes;          // ceil(bits / 9)
  // scatter-phase view of the scratch region
  int64_t cellbuf[3], linepart[3];
  int64_t fx, fpart;   // fused form: the fixed-point scale block, the per-workgroup integer line tables
  int64_t bpart;       // the walk's per-wave shares of d(basis): [FUSED_MAX_WG x WALK_NW_BAS][6][64][4] floats
  int64_t fpart_stride;   // entries (8 bytes each) per workgroup table
  bool dense_cells;    // cell buffer indexed by cell (K <= M) or by the cell's first sorted position (K > M: at most M cells hold samples)
  uint32_t cell_slots[3];
};

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// ---- launch plan of the walk --------------------------------------------------------------------------------------------------------
// Sort s serves plane sort_plane(s) AND the line of the axis that is not in its key (line index sort_plane(s)).  A workgroup keeps ONE
// line block's window of that line's integer table for ONE grid in LDS: (bs + 1) x C x 8 bytes beside the waves' records; the sort keys
// carry the block (line_blocks / make_geom: the headline grid [150, 172, 516] needs 1 / 1 / 3 blocks for theta / phi / r at C = 48 -
// the r line alone would be 198 KB).  Only a line whose block window does not fit even in WALK_MAX_BLOCKS blocks keeps the two-pass form.
constexpr int FUSED_LDS_LIMIT = 160 * 1024 - 1024;
constexpr int WALK_MAX_BLOCKS = 16, WALK_MAX_SEG = 6 * WALK_MAX_BLOCKS;   // line blocks per sort; (sort, grid, block) segments of a launch
constexpr int WALK_NW_APP = 12, WALK_NW_DENS = 16, WALK_NW_BAS = 8;   // waves per workgroup: 144+ VGPRs at 48 channels (three waves per SIMD), ~110 at 16
struct FusedPlan {
  int nw;
  bool do_line[3];   // per sort
  int entries_max;   // 8-byte table entries per workgroup (0: no fused line at all)
  int lds_bytes;
};
__host__ __device__ constexpr int fused_line_axis(int s) { return 2 - (s == 0 ? 1 : s == 1 ? 0 : 2); }   // vm_line_ax(sort_plane(s))
inline int walk_wave_bytes(int C) { return 12 * 64 * 4 + (C / 16) * 4 * 64 * 4; }   // sizeof(WalkLds<C / 16>): asserted next to WalkLds
inline int walk_nw(int C) { return C > 16 ? WALK_NW_APP : WALK_NW_DENS; }

// LDS bytes left for a line window beside the C-channel walk's wave records and its deal table (1024 bytes)
inline int walk_line_room(int C) { return FUSED_LDS_LIMIT - walk_nw(C) * walk_wave_bytes(C) - 1024; }
// does one block's window (bs cells = bs + 1 texels, 8 bytes per channel) of a line fit there?  The workspace layout asks for the
// widest field (CMAX: the 16-channel walk has more room), fused_plan for the field it launches.
inline bool line_window_fits(uint32_t bs, int C) { return (int64_t)(bs + 1) * C * 8 <= walk_line_room(C); }

// the two-pass form (lockstep plane kernel + line kernels) stays reachable for A/B: EGO_SORTED_WALK=0; EGO_SORTED_LINES=separate keeps the
// two-pass LINES under the walk's planes.  Both are read per call: a sort and the scatters that use it must see the same values.
inline bool walk_wanted() {
  const char* e = getenv("EGO_SORTED_WALK");
  return !(e && e[0] == '0');
}
inline bool lines_separate() {
  const char* e = getenv("EGO_SORTED_LINES");
  return e && e[0] == 's';
}

// blocks of the third axis (n texels, n + 1 cells): the fewest whose window fits beside the 48-channel walk
inline void line_blocks(int n, uint32_t* nb, uint32_t* bs) {
  uint32_t k = 1;
  while (k < WALK_MAX_BLOCKS && !line_window_fits((uint32_t)(n + 1 + k - 1) / k, CMAX)) ++k;
  *nb = k; *bs = (uint32_t)(n + 1 + k - 1) / k;
}

inline SortGeom make_geom(const int32_t res[3], int64_t M) {
  SortGeom G{};
  G.M = M;
  uint32_t lcmax = 0;
  for (int a = 0; a < 3; ++a) G.res[a] = res[a];
  bool blocked = walk_wanted() && !lines_separate();
  if (blocked) {   // all or nothing: a line that does not fit even in WALK_MAX_BLOCKS blocks needs the two-pass kernels, which read the plain key layout
    for (int s = 0; s < 3; ++s) {
      uint32_t nb_, bs_;
      line_blocks(res[fused_line_axis(s)], &nb_, &bs_);
      if (!line_window_fits(bs_, CMAX)) blocked = false;
    }
  }
  for (int s = 0; s < 3; ++s) {
    const uint32_t nmaj = (uint32_t)res[sort_major(s)] + 1, nmin = (uint32_t)res[sort_minor(s)] + 1;
    G.nb[s] = 1; G.bs[s] = (uint32_t)res[fused_line_axis(s)] + 1;
    if (blocked) line_blocks(res[fused_line_axis(s)], &G.nb[s], &G.bs[s]);
    G.kc[s] = nmaj * nmin;
    G.K[s] = 2u * G.nb[s] * nmaj * nmin;
    G.LC[s] = 2u * nmaj;
    G.kmax = G.K[s] > G.kmax ? G.K[s] : G.kmax;
    lcmax = G.LC[s] > lcmax ? G.LC[s] : lcmax;
  }
  G.bits = 1;
  while ((1ull << G.bits) <= G.kmax) ++G.bits;      // keys 0 .. K inclusive
  G.nsub_max = (uint32_t)(M / SUB) + lcmax + 1;
  int64_t o = 0;
  for (int s = 0; s < 3; ++s) { G.perm[s] = o; o = align256(o + 4 * M); }
  for (int s = 0; s < 3; ++s) { G.start[s] = o; o = align256(o + 4 * ((int64_t)G.K[s] + 2)); }
  for (int s = 0; s < 3; ++s) { G.suboff[s] = o; o = align256(o + 4 * ((int64_t)G.LC[s] + 1)); }
  for (int s = 0; s < 3; ++s) { G.stepsum[s] = o; o = align256(o + 4 * ((int64_t)G.K[s] + 2)); }
  for (int s = 0; s < 3; ++s) { G.costsum[s] = o; o = align256(o + 4 * ((int64_t)G.K[s] + 2)); }
  for (int s = 0; s < 3; ++s) {
    // a cell of n samples takes ceil(n / 16) steps: at most M / 16 + one per cell that holds samples
    G.step_cap[s] = M / 16 + (M < (int64_t)G.K[s] ? M : (int64_t)G.K[s]) + 1;
    G.steps[s] = o; o = align256(o + 16 * G.step_cap[s]);
  }
  G.scratch = o;
  // sort phase
  int64_t a = o;
  G.passes = (G.bits + RBITS - 1) / RBITS;
  G.nblocks = (uint32_t)((M + RTILE - 1) / RTILE);
  for (int s = 0; s < 3; ++s) { G.keys_in[s] = a; a = align256(a + 4 * M); }
  for (int s = 0; s < 3; ++s) { G.k1[s] = a; a = align256(a + 4 * M); }
  for (int s = 0; s < 3; ++s) { G.v1[s] = a; a = align256(a + 4 * M); }
  for (int s = 0; s < 3; ++s) { G.k2[s] = a; a = align256(a + 4 * M); }
  for (int s = 0; s < 3; ++s) { G.hist[s] = a; a = align256(a + 4 * ((int64_t)RADIX * G.nblocks + RADIX)); }   // + the digit totals
  for (int s = 0; s < 3; ++s) { G.scanpart[s] = a; a = align256(a + 4 * 2 * ((int64_t)G.K[s] / 4096 + 2)); }   // k_step_scan's per-workgroup totals (steps, cost)
  // scatter phase
  int64_t b = o;
  // cell buffer: only cells that hold samples are ever written or read - at most min(K, M) of them (K x 4 x 48 floats was
  // 1.2 GB on the [300, 346, 1036] grid whatever the batch)
  G.dense_cells = (int64_t)G.kmax <= M;
  for (int s = 0; s < 3; ++s) {
    G.cell_slots[s] = G.dense_cells ? G.K[s] : (uint32_t)M;   // sparse: slot = the cell's first sorted position (< M, distinct per non-empty cell)
    G.cellbuf[s] = b; b = align256(b + 4 * (int64_t)G.cell_slots[s] * 4 * CMAX);
  }
  for (int s = 0; s < 3; ++s) { G.linepart[s] = b; b = align256(b + 4 * (int64_t)G.nsub_max * 2 * CMAX); }
  // fused form (shares the line-partial region's place in time, not its bytes: both forms are sized so that either can run)
  G.fx = b; b = align256(b + 256 + 4 * 7 * 128 + 4 * (WALK_MAX_SEG + 1));   // FxScale + k_fx_absmax's per-workgroup maxima + the walk's deal
  {
    // a workgroup's line table: one block's window of the third axis (bs + 1 texels) x the widest field's channels
    int64_t emax = 0;
    for (int s = 0; s < 3; ++s) {
      const int64_t e = (int64_t)(G.bs[s] + 1) * CMAX;
      if (line_window_fits(G.bs[s], CMAX) && e > emax) emax = e;
    }
    G.fpart_stride = emax;
    G.fpart = b; b = align256(b + 8 * G.fpart_stride * FUSED_MAX_WG);
  }
  G.bpart = b; b = align256(b + (int64_t)FUSED_MAX_WG * WALK_NW_BAS * 6 * 256 * 4);
  G.total = a > b ? a : b;
  return G;
}

// which lines the walk of a C-channel field takes along: a sort's line rides along when one block's window of it fits the LDS
inline FusedPlan fused_plan(const SortGeom& G, int C) {
  FusedPlan P{};
  P.nw = walk_nw(C);
  for (int s = 0; s < 3; ++s) {
    P.do_line[s] = !lines_separate() && line_window_fits(G.bs[s], C);
    const int entries = (int)(G.bs[s] + 1) * C;
    if (P.do_line[s] && entries > P.entries_max) P.entries_max = entries;
  }
  P.lds_bytes = FUSED_LDS_LIMIT - walk_line_room(C) + P.entries_max * 8;   // the wave records and the deal table + the widest window
  return P;
}

inline int check_sizes(const ego_scene* sc, int64_t N, int32_t S, const char* who) {
  if (!sc) return ego_fail(EGO_E_BADARG, "%s: null scene", who);
  if (!(N >= 0 && S >= 1 && N * (int64_t)S < (1ll << 31))) return ego_fail(EGO_E_BADARG, "%s: bad size (N * S must be below 2^31)", who);
  for (int a = 0; a < 3; ++a)
    if (sc->density.res[a] < 2 || sc->density.res[a] > 4096) return ego_fail(EGO_E_BADARG, "%s: table resolution out of range [2, 4096]", who);
  return EGO_OK;
}
