// The one launch path of the persistent one-launch epochs (csrc/resident.hip, hybrid.hip,
// vanilla.hip, ushape.hip).  Their workgroups wait on each other inside the launch, so all G must
// be resident at once: fits() checks the occupancy of the instantiation that will be launched,
// launch() goes through hipLaunchCooperativeKernel, which refuses a grid the device cannot hold
// at once instead of queueing part of it (a plain launch, coop = 0, is the tests' A/B).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace sl {
namespace persist {

// Whether G workgroups of kernel fn (threads, lds bytes of dynamic LDS) are resident together on
// `device`.  check: the executor's shape check of the arguments ("" = accepted), reported first.
inline bool fits(std::string check, const void* fn, int threads, int lds, int G, int device, std::string* why) {
  if (check.empty()) {
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, device) != hipSuccess) {
      check = "device properties";
    } else {
      int nb = 0;
      // the attribute first: the occupancy of a kernel above the default dynamic-LDS limit
      hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, lds);
      if (e != hipSuccess || nb < 1) check = "occupancy";
      else if ((int64_t)nb * pr.multiProcessorCount < G) check = "workgroups not co-resident";
    }
  }
  if (why) *why = check;
  return check.empty();
}

// One launch of a.S steps on G workgroups: refuses arguments the check refuses, nothing to do for
// S <= 0, clears the hand-off counters (a.cnt, counter_bytes) on the stream, then launches.
// Cooperative costs +15-19 us of host time per launch, once per client epoch
// (MI355X_MICROARCH.md).
template <typename Args>
inline hipError_t launch(const std::string& check, const void* fn, int threads, int lds, int G, size_t counter_bytes,
                         const Args& a, hipStream_t st) {
  if (!check.empty()) return hipErrorInvalidValue;
  if (a.S <= 0) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.cnt, 0, counter_bytes, st);
  if (e != hipSuccess) return e;
  Args arg = a;
  void* params[] = {&arg};
  if (!a.coop) return hipLaunchKernel(fn, dim3(G), dim3(threads), params, (size_t)lds, st);
  return hipLaunchCooperativeKernel(fn, dim3(G), dim3(threads), params, (unsigned)lds, st);
}

}  // namespace persist
}  // namespace sl
