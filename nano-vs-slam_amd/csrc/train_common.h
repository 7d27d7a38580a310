// Device helpers shared by the training kernels (vlad_train.hip, vpr_head_train.hip): sums in a fixed order.
#pragma once
#include <hip/hip_runtime.h>

namespace kp2d {

// sum of n floats p[0], p[stride], ... in index order; eight loads in flight, the additions strictly sequential
__device__ __forceinline__ float ordered_sum(const float* p, size_t stride, int n) {
  float acc = 0.f;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = p[(size_t)(i + j) * stride];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += t[j];
  }
  for (; i < n; ++i) acc += p[(size_t)i * stride];
  return acc;
}

}  // namespace kp2d
