// Host-side choice of the keypoint selection and class-id launches (post.hip launch_topk, launch_gather, launch_seg_argmax,
// launch_post_seg): which kernel and template instance runs, how much dynamic LDS it asks for, whether that takes the opt-in
// to the CU's whole LDS, and which of a kernel's internal paths the shape selects.  Every decision is made here once; the
// launchers only launch what was chosen, and the kernels ask the same constexpr predicates for their internal branches.
// Plain C++: the two tuning values (options.h Tuning: topk_small, gather_lds) are arguments and the device is never asked
// (tests/test_post_select_ref_cpu.py compiles it with g++).
#pragma once
#include <cstddef>
#include <cstdio>

namespace kp2d {

constexpr size_t LDS_PLAIN_MAX = 65536;   // dynamic LDS a launch may ask for without lds_opt_in (device_guard.h)

// ---------------------------------------------------------------------------------------------------------------------
// top-k
// ---------------------------------------------------------------------------------------------------------------------
constexpr int TOPK_LDS_MAX = 16384;       // keys that fit the LDS path
constexpr int TOPK_KPT = 8;               // keys a thread caches in registers
// KP2D_TOPK_SMALL is honoured up to here: the 256-thread form then never asks for more LDS than LDS_PLAIN_MAX
// (4096 keys: 32 KB of keys + 9.3 KB of histogram and exchange buffer)
constexpr int TOPK_SMALL_LIMIT = 4096;

enum TopkKernel {
  TOPK_256 = 0,   // topk_kernel<256>
  TOPK_1024,      // topk_kernel<1024>
  TOPK_GLOBAL,    // topk_global_kernel: more than TOPK_LDS_MAX keys, sorted in place in the caller's idx row
};

// the frame's keys live in the threads' registers (read from memory once); else every pass reads the frame again
constexpr bool topk_cached(int n, int nthr) { return n <= TOPK_KPT * nthr; }
// `ksort` keys (a power of two) sort with one key per thread in a register; else in the loop over LDS
constexpr bool topk_register_sort(int ksort, int nthr) { return ksort <= nthr; }

struct TopkForm {
  int kernel;        // TopkKernel
  int nthr;          // threads per workgroup
  int kpow;          // key slots in LDS: the smallest power of two >= min(k, n), at least 2 (TOPK_GLOBAL: 0)
  size_t lds;        // dynamic LDS bytes (TOPK_GLOBAL: 0, its LDS is static)
  bool lds_opt_in;   // more than LDS_PLAIN_MAX: lds_opt_in before the launch (only TOPK_1024 ever)
  bool cached;       // topk_cached(n, nthr)
  bool reg_sort;     // every count sorts in registers (kpow <= nthr); else counts above nthr take the LDS loop
};

// 0, or the launcher's error code
inline int choose_topk(int n, int k, int topk_small, TopkForm& f) {
  f = TopkForm{};
  if (k < 1 || n < 1) return -1300;
  const int keff = k < n ? k : n;      // more than n keys can never be selected
  if (keff > TOPK_LDS_MAX) {
    f.kernel = TOPK_GLOBAL;
    f.nthr = 1024;
    return 0;
  }
  int kpow = 2;                         // >= 2: the sort network always touches two key slots
  while (kpow < keff) kpow <<= 1;
  const int small = topk_small < TOPK_SMALL_LIMIT ? topk_small : TOPK_SMALL_LIMIT;
  f.kernel = keff <= small ? TOPK_256 : TOPK_1024;
  f.nthr = f.kernel == TOPK_256 ? 256 : 1024;
  f.kpow = kpow;
  // [kpow] keys | prefix | (pad) | hist[256] | 4 counters | the register sort's exchange buffer (sized for 1024 threads)
  f.lds = (size_t)kpow * 8 + 16 + 260 * 4 + 1024 * 8;
  f.lds_opt_in = f.lds > LDS_PLAIN_MAX;
  f.cached = topk_cached(n, f.nthr);
  f.reg_sort = topk_register_sort(kpow, f.nthr);
  return 0;
}

// e.g. "topk<1024,kpow=4096,cached,loop>", "topk<256,kpow=128,uncached,reg>", "topk<1024,kpow=8192,cached,loop,optin>"
inline void topk_form_name(const TopkForm& f, char* dst, size_t n) {
  if (f.kernel == TOPK_GLOBAL) { std::snprintf(dst, n, "topk<global>"); return; }
  std::snprintf(dst, n, "topk<%d,kpow=%d,%s,%s%s>", f.nthr, f.kpow, f.cached ? "cached" : "uncached", f.reg_sort ? "reg" : "loop",
                f.lds_opt_in ? ",optin" : "");
}

// ---------------------------------------------------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------------------------------------------------
enum GatherKernel {
  GATHER_DIRECT = 0,   // gather_kernel
  GATHER_LDS,          // gather_lds_kernel<planes>
};

// gather_lds_kernel's copy of the planes into LDS: 16 bytes per step, or float by float
constexpr bool gather_vec_copy(int n) { return (n & 3) == 0; }
// gather_lds_kernel's stores of a keypoint's channels: 16 bytes per step, or float by float
constexpr bool gather_vec_store(int planes, int C) { return planes % 4 == 0 && (C & 3) == 0; }

struct GatherForm {
  int kernel;        // GatherKernel
  int planes;        // GATHER_LDS: channel planes per workgroup (8, 4, 2); else 0
  bool vec_copy;     // GATHER_LDS: gather_vec_copy(n)
  bool vec_store;    // GATHER_LDS: gather_vec_store(planes, C)
  size_t lds;        // dynamic LDS bytes
  bool lds_opt_in;   // the 4-plane form: lds_opt_in before the launch (up to 80 KB)
};

// 0, or the launcher's error code
inline int choose_gather(int B, int C, int n, int k, bool gather_lds, GatherForm& f) {
  f = GatherForm{};
  if (C < 2) return -1310;      // (x, y ride on channels 0 and 1)
  // LDS form: selections of at least an eighth of the cells, planes that fit 64 KB in groups of 8 / 4 / 2 channels, and
  // enough frames to fill the chip with (frame, channel group) workgroups (one frame: 0.268 vs 0.265 ms with the direct form)
  if (gather_lds && (long)k * 8 >= n && (C & 7) == 0 && (long)B * (C / 8) >= 128) {
    // Four planes per workgroup keep the 16-byte stores of a keypoint's row; past 64 KB that takes the opt-in to the
    // CU's whole LDS (4800 cells at 240 x 320: 76.8 KB, two workgroups per CU).  Two planes per workgroup wrote 8 bytes
    // per keypoint from sixteen workgroups per frame: 30 us at 64 frames.
    if ((long)n * 8 * 4 <= (long)LDS_PLAIN_MAX) f.planes = 8;
    else if ((long)n * 4 * 4 <= 80 * 1024) f.planes = 4;
    else if ((long)n * 2 * 4 <= (long)LDS_PLAIN_MAX) f.planes = 2;
  }
  if (f.planes == 0) return 0;      // GATHER_DIRECT
  f.kernel = GATHER_LDS;
  f.vec_copy = gather_vec_copy(n);
  f.vec_store = gather_vec_store(f.planes, C);
  f.lds = (size_t)n * f.planes * 4;
  f.lds_opt_in = f.planes == 4;
  return 0;
}

// e.g. "gather<direct>", "gather<lds8,vcopy,vstore>", "gather<lds4,scopy,vstore,optin>", "gather<lds2,vcopy,sstore>"
inline void gather_form_name(const GatherForm& f, char* dst, size_t n) {
  if (f.kernel == GATHER_DIRECT) { std::snprintf(dst, n, "gather<direct>"); return; }
  std::snprintf(dst, n, "gather<lds%d,%s,%s%s>", f.planes, f.vec_copy ? "vcopy" : "scopy", f.vec_store ? "vstore" : "sstore",
                f.lds_opt_in ? ",optin" : "");
}

// ---------------------------------------------------------------------------------------------------------------------
// dense class ids
// ---------------------------------------------------------------------------------------------------------------------
struct ArgmaxForm {
  bool quad;    // seg_argmax4: four pixels per thread, 16-byte loads and stores; else seg_argmax_kernel, pixel by pixel
  bool fused;   // launch_post_seg: post and argmax as ONE launch (post_seg_kernel); else one launch each
};

// seg_mis / ids_mis: the two pointers' offsets from a 16-byte boundary (address & 15)
inline ArgmaxForm choose_argmax(int HW, unsigned seg_mis, unsigned ids_mis) {
  ArgmaxForm f{};
  f.quad = (HW & 3) == 0 && seg_mis == 0 && ids_mis == 0;
  return f;
}

// the channel counts post_kernel is instantiated for
constexpr bool post_channels_ok(int C) { return C == 32 || C == 64 || C == 128; }

// launch_post_seg: the fused launch takes the quad argmax, one batch size and a descriptor width post_kernel has
inline ArgmaxForm choose_post_seg(int HW, unsigned seg_mis, unsigned ids_mis, int post_B, int seg_B, int post_C) {
  ArgmaxForm f = choose_argmax(HW, seg_mis, ids_mis);
  f.fused = f.quad && post_B == seg_B && post_channels_ok(post_C);
  return f;
}

// "argmax<fused,quad>", "argmax<two,quad>", "argmax<two,scalar>"
inline void argmax_form_name(const ArgmaxForm& f, char* dst, size_t n) {
  std::snprintf(dst, n, "argmax<%s,%s>", f.fused ? "fused" : "two", f.quad ? "quad" : "scalar");
}

}  // namespace kp2d
