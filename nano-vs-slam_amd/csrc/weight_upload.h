// The device half of kp2d_finalize_weights / kp2d_lg_finalize_weights: a handle's packed blob onto its device.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "api_common.h"
#include "device_guard.h"

namespace kp2d {

// *blob is allocated on the first call and overwritten on every later one
inline int upload_blob(int device, float** blob, const std::vector<float>& host_blob) {
  DeviceGuard guard(device);
  if (!*blob) HIP_TRY(hipMalloc((void**)blob, host_blob.size() * sizeof(float)));
  HIP_TRY(hipMemcpy(*blob, host_blob.data(), host_blob.size() * sizeof(float), hipMemcpyHostToDevice));
  return KP2D_OK;
}

}  // namespace kp2d
