// fp16 on the host without the type: what the weight packers (model_desc.cpp, lightglue_desc.cpp) write as split-fp16
// halves.  g++ has no _Float16 on every host the CPU tests build on.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace kp2d {

// (_Float16)f, round to nearest even, and back — in integer arithmetic, for host compilers without the type
inline uint16_t f16_bits(float f) {
  uint32_t x;
  std::memcpy(&x, &f, 4);
  const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
  x &= 0x7fffffffu;
  if (x > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);      // NaN
  if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);     // >= 65520 rounds to inf
  if (x < 0x38800000u) {                                       // below 2^-14: a subnormal half, rounded by the fp32 add
    float a;
    std::memcpy(&a, &x, 4);
    a += 0.5f;
    std::memcpy(&x, &a, 4);
    return (uint16_t)(sign | (x - 0x3f000000u));
  }
  const uint32_t odd = (x >> 13) & 1u;
  x += ((uint32_t)(15 - 127) << 23) + 0xfffu + odd;
  return (uint16_t)(sign | (x >> 13));
}
inline float f16_value(uint16_t h) {
  const int e = (h >> 10) & 31, mant = h & 1023;
  const float v = e == 0 ? std::ldexp((float)mant, -24) : e == 31 ? (mant ? NAN : INFINITY) : std::ldexp((float)(mant | 1024), e - 25);
  return (h & 0x8000u) ? -v : v;
}

}  // namespace kp2d
