// Host-side choice of the NetVLAD launch (netvlad.hip launch_netvlad, plan.cpp vlad_tail): how a frame's pixels are cut into
// slabs and tiles, which pass-1 kernel and template instance runs, and which branch the ordered sum of the partials takes.
// Every decision is made here once; the launcher only launches what was chosen and the plan spells it in the per-layer
// profile (netvlad_form_name).  Plain C++: the two tuning values (options.h Tuning: vlad_px, vlad_split) are arguments and
// the device is never asked (tests/test_pooler_ref_cpu.py compiles it with g++).
#pragma once
#include <cstdio>

namespace kp2d {

constexpr int VLAD_VT = 64;   // pixels per LDS tile of pass 1

// Slabs per frame.  Depends on the frame size only: the order of the partial sums (and with it the last bits of the
// descriptor) must not change with the batch or sub-batch a frame happens to travel in (test_full_size_properties).
inline int netvlad_nsplit(int S, int vlad_px) {
  const int per = vlad_px;            // pixels per workgroup (tuning knob)
  int n = (S + per - 1) / per;
  return n < 1 ? 1 : n;
}

// Workgroups per slab.  1 (slab mode): a workgroup walks its whole slab.  > 1 (tile mode: few frames per call, where nsplit
// workgroups per frame would leave the chip idle): one workgroup per 64-pixel tile of the slab; the finish pass then adds the
// tile partials of a slab in tile order before it adds the slabs — the same additions in the same order as a
// workgroup walking the slab, so the result does not depend on which mode a frame was processed in.
inline int netvlad_tiles_per_slab(int S, int B, int vlad_px) {
  const int ns = netvlad_nsplit(S, vlad_px);
  if ((long)B * ns >= 256) return 1;
  const int per = (S + ns - 1) / ns;
  return (per + VLAD_VT - 1) / VLAD_VT;
}

// How vlad_ordered_sum forms one slab's value from its tile partials (the device code asks this very function)
enum VladSum {
  VLAD_SUM_DIRECT = 0,   // tps == 1: the slab's only partial
  VLAD_SUM_UNROLLED,     // tps <= 8: all tile partials in flight at once, then added in tile order
  VLAD_SUM_LOOP,         // more tiles: one after another, in tile order
};
constexpr int netvlad_sum_branch(int tps) { return tps <= 1 ? VLAD_SUM_DIRECT : tps <= 8 ? VLAD_SUM_UNROLLED : VLAD_SUM_LOOP; }

enum VladKernel {
  VLAD_MFMA = 0,   // netvlad_partial_mfma_kernel<KT, SPLIT>: K in {32, 64}, C <= 64; inst = KT (1, 2)
  VLAD_GENERIC,    // netvlad_partial_kernel<NOWN>: every other accepted shape; inst = NOWN (16, 32)
};

struct VladForm {
  int kernel;        // VladKernel
  int inst;          // template instance (see VladKernel)
  bool split;        // VLAD_MFMA: split-fp16 soft-assignment logits (the f16x3 mode unless KP2D_VLAD_SPLIT=0); else exact fp32
  bool lds_opt_in;   // VLAD_GENERIC<32>: more than 64 KB of LDS, asked for once per device
};

// 0, or the launcher's error code for a shape no kernel takes
inline int choose_netvlad(int K, int C, int prec, bool vlad_split, VladForm& f) {
  f = VladForm{};
  if (K > 64 || (K & 3) || (C & 3) || K * C > 8192 || K < 4) return -1100;
  if ((K == 32 || K == 64) && C <= 64) {
    f.kernel = VLAD_MFMA;
    f.inst = K / 32;
    f.split = prec == 1 && vlad_split;
    return 0;
  }
  f.kernel = VLAD_GENERIC;
  f.inst = K * C <= 4096 ? 16 : 32;      // (32: TINY_F, 64 clusters x 128 channels, 83 KB of LDS)
  f.lds_opt_in = f.inst == 32;
  return 0;
}

// The form as the profile spells it, e.g. "netvlad<mfma2,split,tile ns=4 tps=5 sum=unrolled>"
inline void netvlad_form_name(const VladForm& f, int nsplit, int tps, char* dst, size_t n) {
  static const char* const kSum[] = {"direct", "unrolled", "loop"};
  std::snprintf(dst, n, "netvlad<%s%d,%s,%s ns=%d tps=%d sum=%s>", f.kernel == VLAD_MFMA ? "mfma" : "generic", f.inst,
                f.split ? "split" : "exact", tps > 1 ? "tile" : "slab", nsplit, tps > 1 ? tps : 1,
                kSum[netvlad_sum_branch(tps)]);
}

}  // namespace kp2d
