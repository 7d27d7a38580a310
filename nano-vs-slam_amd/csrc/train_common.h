// What the five training translation units share (vlad_train.hip, vpr_head_train.hip, seg_train.hip, depth_train.hip,
// keypoint_train.hip): sums in a fixed order on the device, and the pointer checks of their C-ABI entry points on the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

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

// ---- host: an entry point's pointers ---------------------------------------------------------------------------------------
inline bool misaligned(const void* p, size_t a) { return (uintptr_t)p % a != 0; }

// any of these pointers is null; any of these arrays of 4-byte elements is misaligned (a null pointer, an optional argument
// left out, is not)
template <typename... P> bool any_null(const P*... p) { return (... || !p); }
template <typename... P> bool any_misaligned4(const P*... p) { return (... || misaligned(p, 4)); }

}  // namespace kp2d
