// What every host file behind the C ABI shares: the thread-local error message, HIP_TRY and the workspace alignment.
// No HIP header here (model_desc.cpp and lightglue_desc.cpp compile without one); HIP_TRY expands where <hip/hip_runtime.h> is included.
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdio>

#include "../../include/kp2d.h"

namespace kp2d {

void set_last_error(const char* msg);   // thread-local message behind kp2d_last_error() (kp2d_api.cpp)

inline int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  set_last_error(buf);
  return code;
}

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t v, size_t a = ALIGN) { return (v + a - 1) / a * a; }

// One walk defines a scratch layout: a feature's layout function takes its pieces in order and returns typed pointers.
// base == nullptr is the sizing pass (every pointer null, bytes() the size); with the caller's buffer the same walk
// yields the pointers.  A piece starts at align_up(end, align); the layout's owner decides how bytes() is rounded.
struct Carve {
  char* base = nullptr;
  size_t end = 0;
  explicit Carve(void* scratch = nullptr) : base(static_cast<char*>(scratch)) {}
  template <class T>
  T* take(size_t count, size_t align = ALIGN) {
    const size_t at = align_up(end, align);
    end = at + count * sizeof(T);
    return base ? reinterpret_cast<T*>(base + at) : nullptr;
  }
  size_t bytes(size_t align = ALIGN) const { return align_up(end, align); }
};

}  // namespace kp2d

#define HIP_TRY(expr)                                                                                \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) return kp2d::fail(KP2D_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
  } while (0)
