// common.hpp — what every HIP translation unit shares on the host side: error capture (hip_fail, TBNAV_HIP), the device guard and
// the device a create call picks.  It pulls in wave.hpp, the device side's wave-wide reductions and scans.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <string>

#include "tbnav_status.h"

namespace tbnav {

// Thread-local text of the last failing HIP call; surfaced through tbnav_last_hip_error().
std::string& last_hip_error_slot();

inline int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  char buf[512];
  std::snprintf(buf, sizeof buf, "%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
  last_hip_error_slot() = buf;
  return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver)
             ? TBNAV_ERR_NO_DEVICE
             : TBNAV_ERR_HIP;
}

#define TBNAV_HIP(call)                                                       \
  do {                                                                        \
    hipError_t tbnav_e_ = (call);                                             \
    if (tbnav_e_ != hipSuccess) return ::tbnav::hip_fail(tbnav_e_, #call, __FILE__, __LINE__); \
  } while (0)

// Makes `dev` the calling thread's device for a scope and puts the earlier one back; !ok: it could not, and nothing was changed.
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess) ok = true; }
  ~DeviceGuard() { if (ok && prev >= 0) (void)hipSetDevice(prev); }
};

// The device a create call runs on: a negative index asks for the calling thread's current device, an index past the device count
// is TBNAV_ERR_INVALID_ARG, and a machine without devices is TBNAV_ERR_NO_DEVICE with the text set.
inline int pick_device(int requested, int* dev) {
  int ndev = 0;
  const hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) return hip_fail(e == hipSuccess ? hipErrorNoDevice : e, "hipGetDeviceCount", __FILE__, __LINE__);
  if (requested < 0) TBNAV_HIP(hipGetDevice(&requested));
  if (requested >= ndev) return TBNAV_ERR_INVALID_ARG;
  *dev = requested;
  return TBNAV_OK;
}

}  // namespace tbnav

#include "wave.hpp"
