// Host side shared by the translation units of libegonerf_hip.so: error plumbing, the builders of the kernel-argument structs of
// ego_device.h, and the ONE copy of each shape check in front of the kernels (a field's tables, the component envelope, the head
// shape).  (The tuned shape's shared constants, K orders and host checks are in ego_tuned.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <atomic>
#include "../../include/egonerf_hip.h"
#include "ego_device.h"   // DevField, DevCoords, DevOcc; the axis maps and table sizes

inline char* ego_err_buf() {
  static thread_local char buf[512] = "";
  return buf;
}

inline int ego_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(ego_err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

#define EGO_REQUIRE(cond, msg) \
  do {                         \
    if (!(cond)) return ego_fail(EGO_E_BADARG, "%s", msg); \
  } while (0)

// csrc/ego_shade.hip: can ego_shade_composite serve this scene and sample count? (asked by ego_render_forward)
bool ego_can_fold_composite(const ego_scene* sc, int32_t S);
bool ego_fold_is_balanced(int64_t N, int32_t S);
// ... and the compact path's pieces: the live-sample list (csrc/ego_compact.hip) and the shade over it (csrc/ego_shade.hip)
int64_t ego_live_blocks(int64_t N);
int ego_compact_live(const float* weight, int64_t N, int32_t S, float above, int32_t* live, int32_t* count, int32_t* part, int32_t* n_live,
                     void* stream);
int ego_shaded_count(int32_t mode, const int32_t* n_live, const uint8_t* act, int64_t N, int32_t S, int64_t* out, void* stream);
int ego_shade_live(const ego_scene* sc, const float* rays, const float* z, const float* coords, int64_t N, int32_t S, const int32_t* live,
                   const int32_t* n_live, float* rgb, void* stream);

// workgroups of b threads for n items
inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

inline int ego_launch_status(const char* kernel) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ego_fail((int)e, "%s: launch failed: %s", kernel, hipGetErrorString(e));
  return EGO_OK;
}

// utils.py:117-121: the `filter_size` normalised Gaussian taps of rgb_ssim's window (ego_rgb_ssim and ego_patch_ssim both take theirs
// from here); filt must hold filter_size doubles
inline void ego_ssim_taps(int filter_size, double filter_sigma, double* filt) {
  const int hw = filter_size / 2;
  const double shift = (2 * hw - filter_size + 1) / 2.0;
  double tot = 0.0;
  for (int i = 0; i < filter_size; ++i) {
    const double f = ((double)(i - hw) + shift) / filter_sigma;
    filt[i] = exp(-0.5 * f * f);
    tot += filt[i];
  }
  for (int i = 0; i < filter_size; ++i) filt[i] /= tot;
}

// compute units of the CURRENT device (what sizes a launch by wave slots: the march's split, the sorted walk's grid); queried once per
// device; racing first calls store the same value
inline int device_cus() {
  static std::atomic<int> cus_of[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
  int cus = cus_of[dev].load(std::memory_order_relaxed);
  if (!cus) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    cus_of[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

// ---- the scene's structs -> their kernel-argument copies (ego_device.h), and the checks in front of them ----------------------------
inline DevField make_field(const ego_vm_field& f) {
  DevField d;
  uintptr_t lo = ~(uintptr_t)0;
  for (int g = 0; g < 2; ++g)
    for (int i = 0; i < 3; ++i) {
      d.plane[g][i] = f.plane[g][i];
      d.line[g][i] = f.line[g][i];
      if (f.plane[g][i] && (uintptr_t)f.plane[g][i] < lo) lo = (uintptr_t)f.plane[g][i];
      if (f.line[g][i] && (uintptr_t)f.line[g][i] < lo) lo = (uintptr_t)f.line[g][i];
    }
  for (int i = 0; i < 3; ++i) d.res[i] = f.res[i];
  d.base = (const char*)lo;
  for (int g = 0; g < 2; ++g)
    for (int i = 0; i < 3; ++i) {
      d.poff[g][i] = (uint32_t)((uintptr_t)f.plane[g][i] - lo);
      d.loff[g][i] = (uint32_t)((uintptr_t)f.line[g][i] - lo);
    }
  return d;
}

inline DevCoords make_coords(const ego_scene& s, bool fine_pass = false) {
  DevCoords c;
  c.cx = s.center[0]; c.cy = s.center[1]; c.cz = s.center[2];
  c.th_near = s.ang_near[0]; c.ph_near = s.ang_near[1];
  c.th_inv = s.ang_inv[0]; c.ph_inv = s.ang_inv[1];
  c.r_lut = s.r_lut; c.n_lut = s.n_r_lut; c.n_r = s.n_r;
  if (fine_pass && s.r_lut_fine) { c.r_lut = s.r_lut_fine; c.n_lut = s.n_r_lut_fine; c.n_r = s.n_r_fine; }
  return c;
}

inline DevOcc make_occ(const ego_scene& sc, int coarse) {
  DevOcc o;
  o.vol = coarse ? nullptr : sc.occ;  // the coarse (proposal) pass always sees the full field
  o.res[0] = sc.occ_res[0]; o.res[1] = sc.occ_res[1]; o.res[2] = sc.occ_res[2];
  o.cell = (o.vol && o.res[0] >= 2 && o.res[1] >= 2 && o.res[2] >= 2) ? sc.occ_cell : nullptr;
  return o;
}

// all 12 table pointers of a field (ego_vm_field) or of a gradient struct (ego_vm_grad) are set
template <class T>
inline bool vm_tables_complete(const T& t) {
  for (int g = 0; g < 2; ++g)
    for (int i = 0; i < 3; ++i)
      if (!t.plane[g][i] || !t.line[g][i]) return false;
  return true;
}

// true iff every table of the field (elem_bytes per element, n_comp channels) ends within 4 GB of the lowest table address, i.e.
// DevField's 32-bit byte offsets address all of it.  The host layer allocates the tables of a field from one buffer.
inline bool ego_field_is_compact(const ego_vm_field& f, int elem_bytes) {
  if (!vm_tables_complete(f)) return false;
  uintptr_t lo = ~(uintptr_t)0, hi = 0;
  for (int g = 0; g < 2; ++g)
    for (int i = 0; i < 3; ++i) {
      const uintptr_t p = (uintptr_t)f.plane[g][i], l = (uintptr_t)f.line[g][i];
      const uintptr_t pe = p + (uintptr_t)vm_plane_elems(f.res, f.n_comp, i) * elem_bytes;
      const uintptr_t le = l + (uintptr_t)vm_line_elems(f.res, f.n_comp, i) * elem_bytes;
      lo = p < lo ? p : lo; lo = l < lo ? l : lo;
      hi = pe > hi ? pe : hi; hi = le > hi ? le : hi;
    }
  return hi - lo < ((uintptr_t)1 << 32);
}

// the component counts of the any-shape, stage and ray-gradient kernels: a multiple of 4 up to 48
inline bool generic_n_comp_ok(int C) { return C >= 4 && C <= 48 && (C & 3) == 0; }
inline int check_generic_n_comp(int C, const char* who, const char* which = "") {
  return generic_n_comp_ok(C) ? EGO_OK : ego_fail(EGO_E_UNSUPPORTED, "%s: %sn_comp %d (supported: multiples of 4 up to 48)", who, which, C);
}

// What a kernel asks of a field before it gathers from it, as a predicate: 0, or the first of 1 `envelope`: the component count above,
// 2 all 12 tables, 3 `res2`: resolutions >= 2, 4 `compact`: base + 32-bit offset addressing (the forward gathers) that does not hold
inline int vm_field_fault(const ego_vm_field& f, bool compact, bool envelope, bool res2 = true) {
  if (envelope && !generic_n_comp_ok(f.n_comp)) return 1;
  if (!vm_tables_complete(f)) return 2;
  if (res2 && (f.res[0] < 2 || f.res[1] < 2 || f.res[2] < 2)) return 3;
  return compact && !ego_field_is_compact(f, 4) ? 4 : 0;
}
// ... and as a refusal (`which`: "density ", "appearance " or ""): EGO_E_UNSUPPORTED for the component count, else EGO_E_BADARG
inline int check_vm_field(const ego_vm_field& f, const char* who, const char* which, bool compact, bool envelope, bool res2 = true) {
  switch (vm_field_fault(f, compact, envelope, res2)) {
    case 0: return EGO_OK;
    case 1: return check_generic_n_comp(f.n_comp, who, which);
    case 2: return ego_fail(EGO_E_BADARG, "%s: null %stable pointer", who, which);
    case 3: return ego_fail(EGO_E_BADARG, "%s: %sresolution < 2", who, which);
  }
  return ego_fail(EGO_E_BADARG, "%s: the 12 %stables of a field must lie within 4 GB of each other (allocate them from one buffer): "
                                "the gathers address taps as base + 32-bit offset", who, which);
}

// what every forward gather of a density field asks of it (the entry points of ego_stages.hip and ego_march.hip)
inline int check_field(const ego_vm_field& f, const char* what) { return check_vm_field(f, what, "", true, false); }

// The head shapes outside the tuned one that the any-shape, stage-backward and view-gradient kernels take: app_dim 1..32; with a
// network (`mlp`), featureC 64 or 128; with its input row (`encodings`), view_pe and fea_pe 0..8 and mlp_in = the row's width
// (tensorBase.py:68-75).  `outside` is the caller's code for a shape outside the envelope: EGO_E_UNSUPPORTED from the any-shape entry
// points, EGO_E_BADARG from the stage ops; an mlp_in that contradicts the other numbers is EGO_E_BADARG everywhere.
inline int check_head_shape(const ego_scene* sc, const char* who, int outside, bool mlp = true, bool encodings = true) {
  if (sc->app_dim < 1 || sc->app_dim > 32) return ego_fail(outside, "%s: app_dim %d (supported: 1..32)", who, sc->app_dim);
  if (!mlp) return EGO_OK;
  if (sc->mlp_hidden != 64 && sc->mlp_hidden != 128) return ego_fail(outside, "%s: featureC %d (supported: 64, 128)", who, sc->mlp_hidden);
  if (!encodings) return EGO_OK;
  if (sc->view_pe < 0 || sc->view_pe > 8 || sc->fea_pe < 0 || sc->fea_pe > 8)
    return ego_fail(outside, "%s: view_pe %d / fea_pe %d (supported: 0..8)", who, sc->view_pe, sc->fea_pe);
  const int in_c = sc->app_dim + 3 + 2 * sc->app_dim * sc->fea_pe + 6 * sc->view_pe;
  if (sc->mlp_in != in_c) return ego_fail(EGO_E_BADARG, "%s: mlp_in %d does not match the encoding widths (%d)", who, sc->mlp_in, in_c);
  return EGO_OK;
}

// ---- tracing ("tracing" row) ---------------------------------------------------------------------------
// EGO_ROCTX=1 in the environment: every entry point of the library that queues device work opens a roctx range named after itself
// (roctxRangePushA / roctxRangePop of librocprofiler-sdk-roctx.so, dlopen'ed on first use - no link-time dependency, nothing loaded
// and one predictable branch per call when the switch is off).  `rocprofv3 --marker-trace --kernel-trace -- python bench.py ...`
// then shows which library call (= which row of SURVEY 8(a)) every kernel of every config belongs to, without the stage probes.
struct EgoRoctx {
  int (*push)(const char*);
  int (*pop)();
};
const EgoRoctx* ego_roctx();   // csrc/ego_runtime.hip; nullptr when tracing is off or the roctx library is absent

struct EgoRange {
  const EgoRoctx* r;
  explicit EgoRange(const char* name) : r(ego_roctx()) { if (r) r->push(name); }
  ~EgoRange() { if (r) r->pop(); }
  EgoRange(const EgoRange&) = delete;
  EgoRange& operator=(const EgoRange&) = delete;
};
#define EGO_TRACE(name) EgoRange ego_trace_range_(name)
