// libegonerf_hip.so, triangle meshes: the density on a lattice, an iso-surface extractor, and the gradient of the density
// feature at arbitrary points.  The reference meshes on the host (skimage's marching cubes on a Cartesian alpha volume); here:
//   k_mesh_field      lane = lattice node: position -> yin-yang chart -> normalised coordinates -> density_lookup<C> -> sigma, one kernel
//   k_mesh_classify   lane = node: inside / outside of the node and its seven far corners -> one byte of crossing owned edges, one byte of
//                     triangles of the cell over the node; both counts scanned inside the workgroup (block-local offsets) and summed
//   k_mesh_scan       one workgroup: exclusive scan of the per-workgroup sums, totals -> (V, F)
//   k_mesh_emit       lane = node: vertices of its crossing edges, faces of its cell; a vertex id = workgroup offset + local offset + rank
//   k_point_gradient  a 16-lane row owns a point, lane = channel: k_ray_geometry's per-sample body on points that bring no chart with them
// Marching tetrahedra on the Kuhn decomposition; the definition is in include/egonerf_hip.h and, executable, in tests/mesh_ref.py.
// No atomics anywhere: the order of vertices and faces is fixed and two calls return the same bits.
#include "ego_device.h"
#include "ego_host.h"
#include "ego_density.h"
#include "ego_vm_grad.h"

namespace {

constexpr int MESH_T = 256;         // nodes per workgroup of the field, classify and emit kernels
constexpr int MESH_SCAN_T = 1024;   // threads of the scan workgroup

// a cell's six tetrahedra: corners (bit a = one step along axis a) 000, e_p0, e_p0 + e_p1, 111 for the permutations p in the header's
// order, and the parity of p (1: det[c1 - c0, c2 - c0, c3 - c0] < 0 in index space)
__device__ const uint8_t TET_CORNER[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__device__ const uint8_t TET_ODD[6] = {0, 1, 1, 0, 0, 1};
// a tetrahedron's six edges as pairs of its corners, low corner first
__device__ const uint8_t EDGE_LO[6] = {0, 0, 0, 1, 1, 2};
__device__ const uint8_t EDGE_HI[6] = {1, 2, 3, 2, 3, 3};
// per inside mask (bit c = corner c inside): triangles and their edges, wound for a positively oriented tetrahedron so that
// (v1 - v0) x (v2 - v0) points to the outside (tests/mesh_ref.py: tet_case derives this table from the rule)
__device__ const uint8_t CASE_TRIS[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
__device__ const uint8_t CASE_EDGE[16][6] = {
    {0, 0, 0, 0, 0, 0}, {0, 1, 2, 0, 0, 0}, {0, 4, 3, 0, 0, 0}, {1, 2, 4, 1, 4, 3}, {1, 3, 5, 0, 0, 0}, {2, 0, 3, 2, 3, 5},
    {0, 4, 5, 0, 5, 1}, {2, 4, 5, 0, 0, 0}, {2, 5, 4, 0, 0, 0}, {0, 1, 5, 0, 5, 4}, {3, 0, 2, 3, 2, 5}, {1, 5, 3, 0, 0, 0},
    {1, 3, 4, 1, 4, 2}, {0, 3, 4, 0, 0, 0}, {0, 2, 1, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};

struct Node { int i0, i1, i2; };

// the workspace of an extraction: per workgroup the two sums (exclusive offsets after k_mesh_scan), per node the block-local offsets of its
// first vertex and first face, its crossing owned edges and its cell's triangle count
struct MeshWs {
  int64_t* partV;
  int64_t* partF;
  uint16_t* vloc;
  uint16_t* floc;
  uint8_t* flags;
  uint8_t* tris;
  int64_t nb, bytes;
};

inline int64_t lattice_count(const ego_lattice& L) { return (int64_t)L.n[0] * L.n[1] * L.n[2]; }

inline MeshWs mesh_workspace(const ego_lattice& L, void* base) {
  const int64_t count = lattice_count(L);
  auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  MeshWs w;
  w.nb = (count + MESH_T - 1) / MESH_T;
  char* p = (char*)base;
  int64_t o = 0;
  w.partV = (int64_t*)(p + o); o += up(w.nb * 8);
  w.partF = (int64_t*)(p + o); o += up(w.nb * 8);
  w.vloc = (uint16_t*)(p + o); o += up(count * 2);
  w.floc = (uint16_t*)(p + o); o += up(count * 2);
  w.flags = (uint8_t*)(p + o); o += up(count);
  w.tris = (uint8_t*)(p + o); o += up(count);
  w.bytes = o;
  return w;
}

__device__ __forceinline__ Node node_of(const ego_lattice& L, int m) {
  Node a;
  a.i0 = m % L.n[0];
  const int q = m / L.n[0];
  a.i1 = q % L.n[1];
  a.i2 = q / L.n[1];
  return a;
}

// the node `bits` away from a (a step along axis c where bit c is set), axis 2 of a panorama lattice modulo W: does it exist, and its id
__device__ __forceinline__ bool far_node(const ego_lattice& L, const Node a, int bits, Node& b, int& id) {
  b.i0 = a.i0 + (bits & 1); b.i1 = a.i1 + ((bits >> 1) & 1); b.i2 = a.i2 + ((bits >> 2) & 1);
  bool ok = b.i0 < L.n[0] && b.i1 < L.n[1];
  if (L.kind == EGO_LATTICE_PANORAMA) {
    if (b.i2 == L.n[2]) b.i2 = 0;
  } else {
    ok = ok && b.i2 < L.n[2];
  }
  id = ok ? (b.i2 * L.n[1] + b.i1) * L.n[0] + b.i0 : 0;
  return ok;
}

__device__ __forceinline__ void node_pos(const ego_lattice& L, const Node a, float p[3]) {
  if (L.kind == EGO_LATTICE_PANORAMA) {
    float ray[6];
    erp_ray(L.H, L.W, a.i1, a.i2, L.c2w, 1, ray);
    const float r = L.radii[a.i0];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = __fadd_rn(ray[c], __fmul_rn(r, ray[3 + c]));
  } else {
    p[0] = __fadd_rn(L.origin[0], __fmul_rn((float)a.i0, L.step[0]));
    p[1] = __fadd_rn(L.origin[1], __fmul_rn((float)a.i1, L.step[1]));
    p[2] = __fadd_rn(L.origin[2], __fmul_rn((float)a.i2, L.step[2]));
  }
}

// ---- the field on the lattice --------------------------------------------------------------------------------------------------------
// k_from_cartesian, k_normalize_coord, k_density_feature<C> and k_feature2density (csrc/ego_stages.hip) on one node, without the c7 buffers;
// r is normalised on the full-resolution grid (r_lut_fine where the scene has one: the plain exponential grid)
template <int C, bool LUT_LDS>
__global__ __launch_bounds__(MESH_T) void k_mesh_field(DevField F, DevCoords co, ego_lattice L, int softplus, float shift, int count,
                                                       float* __restrict__ values) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const float* lut = co.r_lut;
  if (LUT_LDS) {   // the radius LUT's binary search runs on a copy in LDS (up to RG_LUT_LDS entries)
    for (int e = threadIdx.x; e < co.n_lut; e += MESH_T) lds[e] = co.r_lut[e];
    __syncthreads();
    lut = lds;
  }
  const int64_t m = (int64_t)blockIdx.x * MESH_T + threadIdx.x;
  if (m >= count) return;
  float p[3];
  node_pos(L, node_of(L, (int)m), p);
  const YinYang y = yinyang_from_xyz(p[0], p[1], p[2], co);
  const float a_r = normalize_r(y.r, lut, co.n_lut, co.n_r);
  const float a_th = normalize_ang(y.th, co.th_near, co.th_inv), a_ph = normalize_ang(y.ph, co.ph_near, co.ph_inv);
  const float f = density_lookup<C>(F, y.yang, a_r, a_th, a_ph);
  values[m] = softplus ? softplus_shift(f, shift) : fmaxf(f, 0.f);
}

// ---- the extractor ---------------------------------------------------------------------------------------------------------------------
// bit b of `in`: corner b of the cell over node a exists and is inside (value >= level; NaN is outside); bit b of `ok`: it exists
__device__ __forceinline__ void corner_bits(const ego_lattice& L, const Node a, const float* __restrict__ values, float level, uint32_t& in,
                                            uint32_t& ok) {
  in = ok = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    Node n;
    int id;
    const bool there = far_node(L, a, b, n, id);
    const float v = values[id];
    ok |= (uint32_t)there << b;
    in |= (uint32_t)(there && v >= level) << b;
  }
}

__device__ __forceinline__ int tet_mask(uint32_t in, int t) {
  return (int)(((in >> TET_CORNER[t][0]) & 1u) | (((in >> TET_CORNER[t][1]) & 1u) << 1) | (((in >> TET_CORNER[t][2]) & 1u) << 2) |
               (((in >> TET_CORNER[t][3]) & 1u) << 3));
}

__global__ __launch_bounds__(MESH_T) void k_mesh_classify(ego_lattice L, const float* __restrict__ values, float level, int count, MeshWs W) {
  __shared__ uint32_t wave_total[MESH_T / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m = (int64_t)blockIdx.x * MESH_T + tid;
  uint32_t fl = 0, tr = 0;
  if (m < count) {
    const Node a = node_of(L, (int)m);
    uint32_t in, ok;
    corner_bits(L, a, values, level, in, ok);
#pragma unroll
    for (int k = 0; k < 7; ++k)   // owned edge k: to corner k + 1
      fl |= (((ok >> (k + 1)) & 1u) & (((in >> (k + 1)) ^ in) & 1u)) << k;
    if ((ok >> 7) & 1u) {         // the cell over this node exists
#pragma unroll
      for (int t = 0; t < 6; ++t) tr += CASE_TRIS[tet_mask(in, t)];
    }
    W.flags[m] = (uint8_t)fl;
    W.tris[m] = (uint8_t)tr;
  }
  // both counts in one word (at most 7 x 256 vertices and 12 x 256 faces per workgroup: 16 bits each), scanned across the workgroup
  const uint32_t mine = (uint32_t)__popc(fl) | (tr << 16);
  uint32_t inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(inc, d, 64);
    if (lane >= d) inc += v;
  }
  if (lane == 63) wave_total[wave] = inc;
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < MESH_T / 64; ++w) {
    if (w < wave) before += wave_total[w];
    total += wave_total[w];
  }
  if (m < count) {
    const uint32_t exc = before + inc - mine;
    W.vloc[m] = (uint16_t)(exc & 0xffffu);
    W.floc[m] = (uint16_t)(exc >> 16);
  }
  if (tid == 0) {
    W.partV[blockIdx.x] = total & 0xffffu;
    W.partF[blockIdx.x] = total >> 16;
  }
}

// exclusive scan of partV[0 .. nb) and partF[0 .. nb) in place, thread t owning a contiguous run of ceil(nb / 1024) entries (k_live_scan's
// form, csrc/ego_compact.hip, in 64 bits and on two arrays); the totals -> counts[0] = V, counts[1] = F.  A run is walked eight entries at a
// time, all loads of the eight ahead of their sums and stores: one round of memory latency per eight entries, not per entry
constexpr int MESH_SCAN_B = 8;

__global__ __launch_bounds__(MESH_SCAN_T) void k_mesh_scan(MeshWs W, int64_t* __restrict__ counts) {
  __shared__ int64_t sums[2][MESH_SCAN_T];
  int64_t* __restrict__ pv = W.partV;
  int64_t* __restrict__ pf = W.partF;
  const int t = threadIdx.x;
  const int64_t per = (W.nb + MESH_SCAN_T - 1) / MESH_SCAN_T;
  const int64_t b0 = (int64_t)t * per < W.nb ? (int64_t)t * per : W.nb, b1 = b0 + per < W.nb ? b0 + per : W.nb;
  int64_t rv = 0, rf = 0;
  for (int64_t b = b0; b < b1; b += MESH_SCAN_B) {
    int64_t v[MESH_SCAN_B], f[MESH_SCAN_B];
#pragma unroll
    for (int j = 0; j < MESH_SCAN_B; ++j) { v[j] = b + j < b1 ? pv[b + j] : 0; f[j] = b + j < b1 ? pf[b + j] : 0; }
#pragma unroll
    for (int j = 0; j < MESH_SCAN_B; ++j) { rv += v[j]; rf += f[j]; }
  }
  sums[0][t] = rv; sums[1][t] = rf;
  __syncthreads();
  for (int d = 1; d < MESH_SCAN_T; d <<= 1) {   // Hillis-Steele over the 1024 run totals (inclusive)
    const int64_t v = t >= d ? sums[0][t - d] : 0, f = t >= d ? sums[1][t - d] : 0;
    __syncthreads();
    sums[0][t] += v; sums[1][t] += f;
    __syncthreads();
  }
  int64_t ov = t ? sums[0][t - 1] : 0, of = t ? sums[1][t - 1] : 0;
  for (int64_t b = b0; b < b1; b += MESH_SCAN_B) {
    int64_t v[MESH_SCAN_B], f[MESH_SCAN_B];
#pragma unroll
    for (int j = 0; j < MESH_SCAN_B; ++j) { v[j] = b + j < b1 ? pv[b + j] : 0; f[j] = b + j < b1 ? pf[b + j] : 0; }
#pragma unroll
    for (int j = 0; j < MESH_SCAN_B; ++j) {
      if (b + j < b1) { pv[b + j] = ov; pf[b + j] = of; }
      ov += v[j]; of += f[j];
    }
  }
  if (t == MESH_SCAN_T - 1) { counts[0] = sums[0][t]; counts[1] = sums[1][t]; }
}

// the vertex of edge k of node `owner`: offset[owner] + popcount(flags[owner] & ((1 << k) - 1))
__device__ __forceinline__ int64_t vertex_id(const MeshWs& W, int owner, int k) {
  return W.partV[owner / MESH_T] + W.vloc[owner] + __popc((uint32_t)W.flags[owner] & ((1u << k) - 1u));
}

__global__ __launch_bounds__(MESH_T) void k_mesh_emit(ego_lattice L, const float* __restrict__ values, float level, int count, MeshWs W, int64_t V,
                                                      int64_t F, float* __restrict__ vertices, int32_t* __restrict__ faces) {
  const int64_t m64 = (int64_t)blockIdx.x * MESH_T + threadIdx.x;
  if (m64 >= count) return;
  const int m = (int)m64;
  const uint32_t fl = W.flags[m], tr = W.tris[m];
  if (!fl && !tr) return;
  const Node a = node_of(L, m);
  if (fl) {
    int64_t vid = W.partV[blockIdx.x] + W.vloc[m];
    float pa[3];
    node_pos(L, a, pa);
    const float fa = values[m];
#pragma unroll 1
    for (int k = 0; k < 7; ++k) {
      if (!((fl >> k) & 1u)) continue;
      Node b;
      int idb;
      far_node(L, a, k + 1, b, idb);
      float pb[3];
      node_pos(L, b, pb);
      float t = __fdiv_rn(__fsub_rn(level, fa), __fsub_rn(values[idb], fa));
      t = fabsf(t) < INFINITY ? fminf(fmaxf(t, 0.f), 1.f) : 0.5f;   // (the comparison is false for NaN too)
      if (vid < V) {   // (V is the caller's: nothing is written past what it allocated)
#pragma unroll
        for (int c = 0; c < 3; ++c) vertices[vid * 3 + c] = __fadd_rn(pa[c], __fmul_rn(t, __fsub_rn(pb[c], pa[c])));
      }
      ++vid;
    }
  }
  if (tr) {
    int64_t fid = W.partF[blockIdx.x] + W.floc[m];
    uint32_t in, ok;
    corner_bits(L, a, values, level, in, ok);
#pragma unroll 1
    for (int t = 0; t < 6; ++t) {
      const int mask = tet_mask(in, t), n_tri = CASE_TRIS[mask];
      // physical orientation of the tetrahedron = parity of its permutation x handedness of the lattice's axes
      const bool swap = ((TET_ODD[t] ^ (uint32_t)L.flip) & 1u) != 0;
      for (int j = 0; j < n_tri; ++j) {
        int32_t v3[3];
#pragma unroll
        for (int e3 = 0; e3 < 3; ++e3) {
          const int e = CASE_EDGE[mask][3 * j + e3];
          const int ca = TET_CORNER[t][EDGE_LO[e]], cb = TET_CORNER[t][EDGE_HI[e]];
          Node o;
          int owner;
          far_node(L, a, ca, o, owner);
          v3[e3] = (int32_t)vertex_id(W, owner, (cb ^ ca) - 1);
        }
        if (fid < F) {
          faces[fid * 3] = v3[0];
          faces[fid * 3 + 1] = swap ? v3[2] : v3[1];
          faces[fid * 3 + 2] = swap ? v3[1] : v3[2];
        }
        ++fid;
      }
    }
  }
}

// ---- gradient of the density feature at points ----------------------------------------------------------------------------------------
// k_ray_geometry's work split without the ray: a wave owns four points, a 16-lane row one of them, lane = channel 16 at a time
constexpr int PG_WAVES = 4;

__global__ __launch_bounds__(64 * PG_WAVES) void k_point_gradient(DevField dens, DevCoords co, int Cd, const float* __restrict__ xyz, int64_t M,
                                                                  int normalize, float* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, row = lane >> 4, c16 = lane & 15;
  const bool lut_lds = co.n_lut <= RG_LUT_LDS;
  const float* lut = lut_lds ? lds : co.r_lut;
  if (lut_lds)
    for (int e = tid; e < co.n_lut; e += 64 * PG_WAVES) lds[e] = co.r_lut[e];
  __syncthreads();
  const f32x4 no_dk[8] = {};
  const int64_t n_units = (M + 4 * PG_WAVES - 1) / (4 * PG_WAVES);
  for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const int64_t pt = (unit * PG_WAVES + wave) * 4 + row;
    if (pt >= M) continue;   // (a whole row leaves: row_sum16 stays inside rows; no workgroup barrier below)
    const float x = xyz[pt * 3], y = xyz[pt * 3 + 1], z = xyz[pt * 3 + 2];
    const YinYang yy = yinyang_from_xyz(x, y, z, co);
    const float rhat = normalize_r(yy.r, lut, co.n_lut, co.n_r);
    const int g = yy.yang;
    const LinD ax[3] = {lind_setup(rhat, dens.res[0]), lind_setup(normalize_ang(yy.th, co.th_near, co.th_inv), dens.res[1]),
                        lind_setup(normalize_ang(yy.ph, co.ph_near, co.ph_inv), dens.res[2])};
    float q[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // relu per plane (EgoNeRF.py:340,346)
      float qi[3] = {0.f, 0.f, 0.f};
      const float dot = row_sum16(plane_terms<true>(dens, Cd, g, i, ax, c16, nullptr, no_dk, qi));
      if (dot > 0.f) { q[0] += qi[0]; q[1] += qi[1]; q[2] += qi[2]; }
    }
    q[0] = row_sum16(q[0]); q[1] = row_sum16(q[1]); q[2] = row_sum16(q[2]);
    float gs[3];
    chart_jt(co, lut, g, rhat, x, y, z, q, gs);
    if (normalize) {
      float u[3];
      unit3(gs, u);
#pragma unroll
      for (int j = 0; j < 3; ++j) gs[j] = __fsub_rn(0.f, u[j]);
    }
    if (c16 < 3) out[pt * 3 + c16] = c16 == 0 ? gs[0] : (c16 == 1 ? gs[1] : gs[2]);
  }
}

// 0, or why the lattice cannot be used
inline const char* lattice_fault(const ego_lattice* L) {
  if (!L) return "null lattice";
  if (L->kind != EGO_LATTICE_BOX && L->kind != EGO_LATTICE_PANORAMA) return "unknown lattice kind";
  if (L->n[0] < 2 || L->n[1] < 2 || L->n[2] < 2) return "every axis of a lattice needs at least 2 nodes";
  if (lattice_count(*L) >= (1ll << 31)) return "a lattice must have fewer than 2^31 nodes";
  if (L->kind == EGO_LATTICE_PANORAMA) {
    if (L->n[1] != L->H || L->n[2] != L->W) return "a panorama lattice has n = (radii, H, W)";
    if (L->W < 3) return "the wrapping axis of a panorama lattice needs W >= 3";
    if (!L->radii) return "a panorama lattice needs its radii";
  }
  return nullptr;
}

}  // namespace

extern "C" {

int ego_mesh_field(const ego_scene* sc, const ego_lattice* lat, float* values, void* stream) {
  EGO_TRACE("ego_mesh_field");
  EGO_REQUIRE(sc && values, "mesh_field: null argument");
  if (const char* why = lattice_fault(lat)) return ego_fail(EGO_E_BADARG, "mesh_field: %s", why);
  EGO_REQUIRE(sc->r_lut && sc->n_r_lut >= 2 && sc->n_r >= 1, "mesh_field: the scene has no radius LUT");
  const ego_vm_field& f = sc->density;
  if (int e = check_field(f, "mesh_field")) return e;
  const int count = (int)lattice_count(*lat);
  const DevCoords co = make_coords(*sc, true);
  const bool lut_lds = co.n_lut <= RG_LUT_LDS;
  const size_t lds_bytes = lut_lds ? sizeof(float) * co.n_lut : 0;
  switch (f.n_comp) {   // ego_density_feature's instances
#define EGO_MESH_FIELD_CASE(C)                                                                                                                      \
    case C:                                                                                                                                         \
      if (lut_lds) k_mesh_field<C, true><<<nblk(count, MESH_T), MESH_T, lds_bytes, (hipStream_t)stream>>>(make_field(f), co, *lat, sc->act_softplus, \
                                                                                                       sc->density_shift, count, values);          \
      else k_mesh_field<C, false><<<nblk(count, MESH_T), MESH_T, 0, (hipStream_t)stream>>>(make_field(f), co, *lat, sc->act_softplus,               \
                                                                                        sc->density_shift, count, values);                         \
      break;
    EGO_MESH_FIELD_CASE(4) EGO_MESH_FIELD_CASE(8) EGO_MESH_FIELD_CASE(12) EGO_MESH_FIELD_CASE(16)
    EGO_MESH_FIELD_CASE(20) EGO_MESH_FIELD_CASE(24) EGO_MESH_FIELD_CASE(28) EGO_MESH_FIELD_CASE(32)
    EGO_MESH_FIELD_CASE(36) EGO_MESH_FIELD_CASE(40) EGO_MESH_FIELD_CASE(44) EGO_MESH_FIELD_CASE(48)
#undef EGO_MESH_FIELD_CASE
    default: return ego_fail(EGO_E_UNSUPPORTED, "mesh_field: n_comp %d (supported: multiples of 4 up to 48)", f.n_comp);
  }
  return ego_launch_status("k_mesh_field");
}

int64_t ego_mesh_workspace_bytes(const ego_lattice* lat) {
  if (lattice_fault(lat)) return -1;
  return mesh_workspace(*lat, nullptr).bytes;
}

int ego_mesh_count(const ego_lattice* lat, const float* values, float level, void* workspace, int64_t bytes, int64_t* counts_dev, void* stream) {
  EGO_TRACE("ego_mesh_count");
  if (const char* why = lattice_fault(lat)) return ego_fail(EGO_E_BADARG, "mesh_count: %s", why);
  EGO_REQUIRE(values && workspace && counts_dev, "mesh_count: null argument");
  EGO_REQUIRE(fabsf(level) < INFINITY, "mesh_count: the level must be finite");
  const MeshWs w = mesh_workspace(*lat, workspace);
  EGO_REQUIRE(bytes >= w.bytes, "mesh_count: the workspace is smaller than ego_mesh_workspace_bytes");
  EGO_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)counts_dev & 7) == 0, "mesh_count: workspace must be 256-byte and counts 8-byte aligned");
  const int count = (int)lattice_count(*lat);
  k_mesh_classify<<<(unsigned)w.nb, MESH_T, 0, (hipStream_t)stream>>>(*lat, values, level, count, w);
  if (int e = ego_launch_status("k_mesh_classify")) return e;
  k_mesh_scan<<<1, MESH_SCAN_T, 0, (hipStream_t)stream>>>(w, counts_dev);
  return ego_launch_status("k_mesh_scan");
}

int ego_mesh_emit(const ego_lattice* lat, const float* values, float level, const void* workspace, int64_t V, int64_t F, float* vertices,
                  int32_t* faces, void* stream) {
  EGO_TRACE("ego_mesh_emit");
  if (const char* why = lattice_fault(lat)) return ego_fail(EGO_E_BADARG, "mesh_emit: %s", why);
  EGO_REQUIRE(V >= 0 && F >= 0 && V < (1ll << 31) && F < (1ll << 31), "mesh_emit: V and F must lie in [0, 2^31)");
  if (V == 0 && F == 0) return EGO_OK;
  EGO_REQUIRE(values && workspace && (vertices || V == 0) && (faces || F == 0), "mesh_emit: null argument");
  EGO_REQUIRE(((uintptr_t)workspace & 255) == 0, "mesh_emit: workspace must be 256-byte aligned");
  const MeshWs w = mesh_workspace(*lat, (void*)workspace);
  k_mesh_emit<<<(unsigned)w.nb, MESH_T, 0, (hipStream_t)stream>>>(*lat, values, level, (int)lattice_count(*lat), w, V, F, vertices, faces);
  return ego_launch_status("k_mesh_emit");
}

int ego_point_gradient(const ego_scene* sc, const float* xyz, int64_t M, int32_t normalize, float* out, void* stream) {
  EGO_TRACE("ego_point_gradient");
  EGO_REQUIRE(sc, "point_gradient: null scene");
  EGO_REQUIRE(M >= 0 && M < (1ll << 31), "point_gradient: M outside [0, 2^31)");
  if (M == 0) return EGO_OK;
  EGO_REQUIRE(xyz && out, "point_gradient: null argument");
  EGO_REQUIRE(sc->r_lut && sc->n_r_lut >= 2 && sc->n_r >= 1, "point_gradient: the scene has no radius LUT");
  if (int e = check_vm_field(sc->density, "point_gradient", "density ", true, true)) return e;
  const DevCoords co = make_coords(*sc);
  const size_t lds_bytes = sizeof(float) * ((co.n_lut <= RG_LUT_LDS ? co.n_lut : 0) + 4);
  const int64_t units = (M + 4 * PG_WAVES - 1) / (4 * PG_WAVES);
  const unsigned grid = (unsigned)(units < 4096 ? units : 4096);
  k_point_gradient<<<grid, 64 * PG_WAVES, lds_bytes, (hipStream_t)stream>>>(make_field(sc->density), co, sc->density.n_comp, xyz, M, normalize != 0, out);
  return ego_launch_status("k_point_gradient");
}

}  // extern "C"
