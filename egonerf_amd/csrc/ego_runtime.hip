// libegonerf_hip.so: process-level plumbing (roctx hooks, ABI version, last error) and the device -> mapped-host copy kernel.
#include <dlfcn.h>
#include <stdlib.h>
#include "ego_device.h"
#include "ego_host.h"

// roctx hooks of EGO_TRACE (ego_host.h): resolved once, on the first traced call
const EgoRoctx* ego_roctx() {
  static const EgoRoctx* const hooks = []() -> const EgoRoctx* {
    const char* e = getenv("EGO_ROCTX");
    if (!e || !*e || *e == '0') return nullptr;
    static EgoRoctx h{};
    for (const char* lib : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
      void* so = dlopen(lib, RTLD_NOW | RTLD_GLOBAL);
      if (!so) continue;
      h.push = (int (*)(const char*))dlsym(so, "roctxRangePushA");
      h.pop = (int (*)())dlsym(so, "roctxRangePop");
      if (h.push && h.pop) return &h;
    }
    fprintf(stderr, "libegonerf_hip: EGO_ROCTX is set but no roctx library could be loaded; tracing ranges are off\n");
    return nullptr;
  }();
  return hooks;
}

extern "C" {

int ego_abi_version(void) { return EGO_ABI_VERSION; }
const char* ego_last_error(void) { return ego_err_buf(); }

// ---- device -> mapped host memory, by a kernel of a chosen (small) footprint --------------------------------------------------------
struct CopyOutArgs {
  const float* src[EGO_COPY_OUT_MAX];
  float* dst[EGO_COPY_OUT_MAX];
  int64_t n[EGO_COPY_OUT_MAX];   // floats
  int32_t count;
};

__global__ __launch_bounds__(256) void k_copy_out(CopyOutArgs A) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  for (int t = 0; t < A.count; ++t) {
    const float* __restrict__ s = A.src[t];
    float* __restrict__ d = A.dst[t];
    const int64_t n = A.n[t];
    if ((((uintptr_t)s | (uintptr_t)d) & 15) == 0) {
      const int64_t n4 = n >> 2;
      for (int64_t i = tid; i < n4; i += nth) __builtin_nontemporal_store(((const f32x4*)s)[i], (f32x4*)d + i);
      for (int64_t i = (n4 << 2) + tid; i < n; i += nth) d[i] = s[i];
    } else {
      for (int64_t i = tid; i < n; i += nth) d[i] = s[i];
    }
  }
}

int ego_copy_out(int32_t count, const float* const* src, float* const* dst, const int64_t* n_floats, int32_t workgroups, void* stream) {
  EGO_TRACE("ego_copy_out");
  EGO_REQUIRE(count >= 0 && count <= EGO_COPY_OUT_MAX && workgroups >= 1 && workgroups <= 65535, "copy_out: count / workgroups out of range");
  if (count == 0) return EGO_OK;
  EGO_REQUIRE(src && dst && n_floats, "copy_out: null argument");
  CopyOutArgs a{};
  int64_t total = 0;
  for (int t = 0; t < count; ++t) {
    EGO_REQUIRE(n_floats[t] >= 0 && (n_floats[t] == 0 || (src[t] && dst[t])), "copy_out: null buffer or negative size");
    a.src[t] = src[t]; a.dst[t] = dst[t]; a.n[t] = n_floats[t];
    total += n_floats[t];
  }
  a.count = count;
  if (total == 0) return EGO_OK;
  k_copy_out<<<workgroups, 256, 0, (hipStream_t)stream>>>(a);
  return ego_launch_status("k_copy_out");
}

}  // extern "C"
