// conv3x3_f16x3_s16_kernel's launch side (the kernel template and what it is for: conv3x3_s16_kernel.inc; its ids-only
// instantiation lives in conv3x3_s16_ids.hip) and the S16P -> planar copy of a tapped layer.
#include "conv3x3_s16_kernel.inc"

namespace kp2d {

// ---- launch side -----------------------------------------------------------------------------------------------------
template <int STORE, int NN, int NCH = 2>
static int s16_launch_one(const ConvArgs& a, int grid, long nitems, hipStream_t s) {
  static PerDeviceOnce lds_once;      // per instantiation and device
  if (int e = lds_opt_in(lds_once, reinterpret_cast<const void*>(&conv3x3_f16x3_s16_kernel<STORE, NN, NCH>))) return e;
  hipLaunchKernelGGL((conv3x3_f16x3_s16_kernel<STORE, NN, NCH>), dim3(grid), dim3(D_THREADS), d_lds(16 * NN, NCH), s, a, (int)nitems);
  return (int)hipGetLastError();
}

// what conv_policy.h choose_s16() chose
int launch_conv3x3_f16x3_s16(const ConvArgs& a0, const ConvChoice& c, hipStream_t s) {
  ConvArgs a = a0;
  a.tiles_x = c.tiles_x; a.tiles_y = c.tiles_y;
  switch (a.store) {
    case ST_NCHW: return s16_launch_one<ST_NCHW, 2, 4>(a, c.grid, c.nitems, s);
    case ST_IDS:
      conv3x3_note_variant("<s16>ids");      // (what kp2d_profile_get reports; see conv_policy.h choose_s16)
      return launch_conv3x3_f16x3_s16_ids(a, c.grid, c.nitems, s);
    case ST_S16P: return s16_launch_one<ST_S16P, 2>(a, c.grid, c.nitems, s);
    case ST_NHWC: return s16_launch_one<ST_NHWC, 4>(a, c.grid, c.nitems, s);
    case ST_NHWC_BOTH: return s16_launch_one<ST_NHWC_BOTH, 4>(a, c.grid, c.nitems, s);
    case ST_S16P_BOTH: return s16_launch_one<ST_S16P_BOTH, 4>(a, c.grid, c.nitems, s);
    default: return s16_launch_one<ST_NHWC_POOL, 4>(a, c.grid, c.nitems, s);
  }
}

// ---- S16P -> planar fp32 (kp2d_set_tap on a layer whose output is kept split): x = float(hi) + float(lo), which is the
// fp32 activation to within its last bit or two (lo is x - hi rounded to 11 bits) ----
__global__ __launch_bounds__(256) void s16p_to_nchw_kernel(const _Float16* __restrict__ in, float* __restrict__ out, int C, int H, int W, int Ct, int c0, long total) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int x = (int)(e % W);
  long r = e / W;
  const int y = (int)(r % H);
  r /= H;
  const int c = (int)(r % C);
  const long b = r / C;
  const int cc = c + c0;
  const _Float16* p = in + (((b * (Ct / 16) + cc / 16) * H + y) * 2 * (long)W + x) * 16 + (cc & 15);
  out[e] = (float)p[0] + (float)p[(long)W * 16];
}
int launch_s16p_to_nchw(const float* in, float* out, int B, int C, int H, int W, int Ct, int c0, hipStream_t s) {
  const long total = (long)B * C * H * W;
  if (total <= 0) return 0;
  hipLaunchKernelGGL(s16p_to_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const _Float16*>(in), out, C, H, W, Ct, c0, total);
  return (int)hipGetLastError();
}

}  // namespace kp2d
