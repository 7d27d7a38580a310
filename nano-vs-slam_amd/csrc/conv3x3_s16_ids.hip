// conv3x3_f16x3_s16_kernel<ST_IDS>: the class logits behind a 64-channel S16P tensor when the caller wants only the dense
// class map (KP2D_FWD_NO_SEG_LOGITS, plan.cpp): same DMA waves, same products in the same order as the forms that write
// logits, and an epilogue that stores one int64 per pixel instead of 28 floats (conv3x3_s16_kernel.inc).  A translation unit
// of its own: conv3x3_s16.hip's set of code objects stays what tests/test_host_logic.py counts.
#include "conv3x3_s16_kernel.inc"

namespace kp2d {

// (a: tiles_x / tiles_y already those of conv_policy.h's choice — launch_conv3x3_f16x3_s16)
int launch_conv3x3_f16x3_s16_ids(const ConvArgs& a, int grid, long nitems, hipStream_t s) {
  static PerDeviceOnce lds_once;
  if (int e = lds_opt_in(lds_once, reinterpret_cast<const void*>(&conv3x3_f16x3_s16_kernel<ST_IDS, 2, 4>))) return e;
  hipLaunchKernelGGL((conv3x3_f16x3_s16_kernel<ST_IDS, 2, 4>), dim3(grid), dim3(D_THREADS), d_lds(32, 4), s, a, (int)nitems);
  return (int)hipGetLastError();
}

}  // namespace kp2d
