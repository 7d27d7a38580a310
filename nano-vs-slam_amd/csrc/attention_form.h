// Host-side choice of the attention launch (attention.hip launch_attention): which kernel, which template instance, on
// which grid.  Every decision is made here once; the launcher only launches what it chose.  Plain C++: the three tuning
// values (options.h Tuning: att_ksplit, att_q, att_affine) are arguments and the device is never asked
// (tests/test_lightglue_forms.py compiles it with g++).
#pragma once

namespace kp2d {

enum AttKernel {
  ATT_FP32 = 0,   // attention_kernel<DB>: exact fp32 MFMA (prec 0, or head dim > 16); inst = DB (1, 2, 4)
  ATT_KSPLIT,     // attention_ksplit_kernel: 32 queries per workgroup, the keys split over its four waves; inst = 0
  ATT_SPLIT,      // attention_split_kernel<NTHR, WPS>: NTHR / 2 queries per workgroup, every wave walks all keys; inst = NTHR
};

struct AttForm {
  int kernel;         // AttKernel
  int inst;           // template instance (see AttKernel)
  bool affine;        // ATT_SPLIT: 1-D grid decoded in XCD-affine (frame, head) order; else the plain (tiles, heads, B) grid
  int gx, gy, gz;     // grid
  int block;          // threads per workgroup
};

// 0, or the launcher's error code for a shape no kernel takes
inline int choose_attention(int S, int T, int heads, int B, int C, int prec, long att_ksplit, int att_q, bool att_affine,
                            AttForm& f) {
  f = AttForm{};
  const int d = heads > 0 ? C / heads : 0;
  if (heads < 1 || C % heads || d > 64 || (d & 3) || (C & 3)) return -1402;
  if (prec == 1 && d <= 16) {
    // short sequences that leave most of the chip idle in the query-tiled kernel: split the keys over the waves
    if ((long)((S + 127) / 128) * heads * B < att_ksplit && T >= 128) {
      f.kernel = ATT_KSPLIT; f.gx = (S + 31) / 32; f.gy = heads; f.gz = B; f.block = 256;
      return 0;
    }
    // 256 queries per workgroup halve the K / V staging per query (18 % of the kernel at 128); short sequences
    // keep 128 so that the grid still covers the chip
    const bool big = att_q == 256 && (long)((S + 255) / 256) * heads * B >= 512;
    f.kernel = ATT_SPLIT;
    f.inst = big ? 512 : 256;
    f.block = f.inst;
    const int tiles = (S + f.inst / 2 - 1) / (f.inst / 2);
    // (tiles * pairs, 1, 1): XCD-affine pair order (see the kernel); needs pairs % 8 == 0
    f.affine = (heads * B) % 8 == 0 && att_affine;
    if (f.affine) { f.gx = tiles * heads * B; f.gy = 1; f.gz = 1; }
    else { f.gx = tiles; f.gy = heads; f.gz = B; }
    return 0;
  }
  f.kernel = ATT_FP32;
  f.inst = d <= 16 ? 1 : d <= 32 ? 2 : 4;
  f.gx = (S + 63) / 64; f.gy = heads; f.gz = B; f.block = 256;
  return 0;
}

}  // namespace kp2d
