// The counter-based draws of the library: splitmix64's finaliser.  kmeans.hip (the donor of an empty cluster) and mining.hip
// (the sampled negatives) hash their counters through it; tests restate it in Python integers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kp2d {

__host__ __device__ inline uint64_t km_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace kp2d
