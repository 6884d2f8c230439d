// The one host launch path.  All per-process device state of the library lives here and in capi.cpp: the device of the first launch, the CU
// count, and per kernel instantiation the dynamic-LDS attribute already set and the resident-workgroup count.
#pragma once
#include <atomic>
#include <mutex>
#include "hftt_host.h"

// One process drives ONE device (one process per GPU: DESIGN.md section 7): the caches above belong to the device of the first launch.  A launch
// from another device is refused (status 3) before anything is enqueued.  0 = ok.
int hftt_device_guard(const char* what);
// CU count of the current device at the first call, queried once (capi.cpp); -1 = the query failed.  The launchers read it in front of
// hftt_launch; from a second device that only reads the cache, and the launch behind it is refused.
int hftt_cus();

// Raise KERNEL's dynamic-LDS limit when lds exceeds the largest value this kernel has been given (never for lds == 0).  Every kernel
// instantiation has its own `attr`.  The rule does not ask whether the size needs the call: a kernel below the 64 KB that need none
// (resample_kernel, whose window size depends on the descriptor) gets it as well, once per new maximum.  Entry points may be called from any
// host thread: the cached values are atomics, and the attribute is raised under a lock so that `attr` never runs ahead of the runtime.
// 0 = ok; 2 = the runtime refused (error text set).
template <auto KERNEL>
int hftt_lds_attr(const char* what, int lds) {
  static std::atomic<int> attr{0};
  static std::mutex mu;
  if (lds <= attr.load(std::memory_order_acquire)) return 0;
  std::lock_guard<std::mutex> lock(mu);
  if (lds <= attr.load(std::memory_order_relaxed)) return 0;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) { hftt_set_error("%s: hipFuncSetAttribute(%d B LDS) failed: %s", what, lds, hipGetErrorString(e)); return 2; }
  attr.store(lds, std::memory_order_release);
  return 0;
}

// Guard, LDS attribute, launch, launch check -- in this order.  0 = enqueued; 2 = the runtime refused (error text set); 3 = second device.
template <auto KERNEL, typename... Args>
int hftt_launch(const char* what, dim3 grid, dim3 block, int lds, hipStream_t st, Args... args) {
  if (hftt_device_guard(what) != 0) return 3;
  if (int rc = hftt_lds_attr<KERNEL>(what, lds)) return rc;
  hipLaunchKernelGGL(KERNEL, grid, block, lds, st, args...);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { hftt_set_error("%s: launch failed: %s", what, hipGetErrorString(e)); return 2; }
  return 0;
}

// Grid of a persistent kernel over nblk work items: min(nblk, per_cu * CUs); -1 = the device query failed (error text set, the caller returns 2)
inline long hftt_persistent_grid(const char* what, long nblk, int per_cu) {
  const long cap = (long)per_cu * hftt_cus();
  if (cap <= 0) { hftt_set_error("%s: device query failed", what); return -1; }
  return nblk < cap ? nblk : cap;
}

// *wgs = workgroups of KERNEL that the whole device holds at once (occupancy x CUs), queried once per instantiation, behind the guard and the
// LDS attribute that the occupancy depends on.  Status as hftt_launch.
template <auto KERNEL>
int hftt_resident_wgs(const char* what, int threads, int lds, int* wgs) {
  static std::atomic<int> resident{0};
  if (resident.load(std::memory_order_relaxed) == 0) {
    if (hftt_device_guard(what) != 0) return 3;
    if (int rc = hftt_lds_attr<KERNEL>(what, lds)) return rc;
    int per_cu = 0;
    const int cus = hftt_cus();
    if (cus <= 0 || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(KERNEL), threads, lds) != hipSuccess || per_cu < 1) {
      hftt_set_error("%s: device / occupancy query failed", what);
      return 2;
    }
    resident.store(per_cu * cus, std::memory_order_relaxed);
  }
  *wgs = resident.load(std::memory_order_relaxed);
  return 0;
}
