// Fine-tuning of the place-recognition head's Conv + BatchNorm + (Leaky)ReLU layers on the device
// (kp2d_cbr_forward_train, kp2d_cbr_backward; include/kp2d.h): convlad1..3 of the reference's VPRHead
// (modules/decoders/vpr.py:22-51, modules/base.py:14-46) under autograd, BatchNorm on its running statistics; and the same
// layers as the reference's model.train() runs them (kp2d_cbr_forward_batchnorm, kp2d_cbr_backward_batchnorm,
// kp2d_dropout2d_mask): BatchNorm on the batch's own statistics with the running statistics' update, Dropout2d.
//
//   forward    c = conv3x3(x, w) (stride 1, padding 1, no bias);  y = act(scale c + shift),  act(v) = v > 0 ? v : slope v
//   backward   dpre = dy (y > 0 ? 1 : slope);  dbeta[co] = sum dpre;  dgamma[co] = sum dpre (c - mean) invstd
//              dc = dpre scale;  dw[co,ci,ky,kx] = sum_{n,y,x} dc[n,co,y,x] x[n,ci,y+ky-1,x+kx-1]
//              dx[n,ci,y,x] = sum_{co,ky,kx} dc[n,co,y-ky+1,x-kx+1] w[co,ci,ky,kx]
//
// Tensors are planar [N, C, H, W] fp32.  The three convolution-shaped products are implicit GEMMs on
// v_mfma_f32_16x16x4_f32 (exact fp32, bit for bit an fma chain); an output tile is 8 rows x 16 columns of the map.
// hc_pack_kernel, hc_conv_kernel, hc_dw_kernel and hc_dw_sum_kernel live in train_conv.h, which seg_train.hip shares.
//   hc_pack_kernel      w [Cout][Cin][3][3] -> [cin][tap][cout] as hc_conv_kernel stages it; the data gradient's form swaps
//                       the channel axes and turns the taps by 180 degrees, so dx is the forward kernel run on dc
//   hc_conv_kernel      grid (tiles, N): A = weights [16 cout][4 cin], B = input [4 cin][16 pixels of a row]; a wave owns two
//                       rows of the tile and every output channel; K = 9 Cin walked as chunks of 16 input channels staged in
//                       LDS (halo tile 16 x 10 x 18, weight slab 16 x 9 x Cout); epilogue: c and y, or the plain result
//   hc_dpre_kernel      grid (Cout, N): dpre and dc of one channel plane, its two BatchNorm sums in a fixed order
//   hc_bn_sum_kernel    the frames' BatchNorm sums added in frame order
//   hc_dw_kernel        grid (slabs, Cin / 16): A = dc [16 cout][4 pixels], B = x shifted by the tap [4 pixels][16 cin]; a slab
//                       is a fixed run of tiles (at most 128 slabs), accumulated in registers, one partial per slab
//   hc_dw_sum_kernel    the slabs' partials added in slab order
// Batch statistics (M = N H W values per channel; formulas in include/kp2d.h), all on grid (Cout, N) but the one-block ones:
//   hb_plane_kernel     a plane's mean and its sum of squared distances from that mean (two passes, never E[c^2] - mean^2)
//   hb_stats_kernel     one block: the planes merged by Chan's formula in frame order -> mean, invstd, the running update
//   hb_apply_kernel     y = act(gamma invstd (c - mean) + beta) drop
//   hb_dsum_kernel      g = dy drop act'(y) and a plane's (sum g, sum g xhat); hc_bn_sum_kernel adds the frames
//   hb_dc_kernel        dc = gamma invstd (g - dbeta / M - xhat dgamma / M), which hc_dw_kernel and hc_conv_kernel then read
//   hb_drop_kernel      the [N, C] dropout factors from the counter-based draw of mix64.h
// No float atomics; the slab cut depends on (N, H, W) alone and every sum runs in a fixed order: bit-identical from run to
// run, and (on running statistics) a frame whose dy is zero everywhere contributes exact zeros whatever its x, y and c
// hold; on batch statistics every frame enters the mean and the variance, so that property does not hold there.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "api_common.h"
#include "device_guard.h"
#include "mix64.h"
#include "train_common.h"
#include "train_conv.h"

using namespace kp2d;

namespace {

// ---- BatchNorm and activation backward of one channel plane ---------------------------------------------------------------
__global__ __launch_bounds__(256) void hc_dpre_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ c,
                                                      const float* __restrict__ scale, const float* __restrict__ mean,
                                                      const float* __restrict__ invstd, float slope, float* __restrict__ dc,
                                                      float* __restrict__ part, int CO, size_t HW) {
  __shared__ float s_r[8];
  const int co = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const size_t base = ((size_t)b * CO + co) * HW;
  const float sc = scale[co], mu = mean[co], is = invstd[co];
  float s0 = 0.f, s1 = 0.f;
  for (size_t e = tid; e < HW; e += 256) {
    const float g = dy[base + e];
    const float dp = y[base + e] > 0.f ? g : slope * g;
    s0 += dp;
    s1 = fmaf(dp, (c[base + e] - mu) * is, s1);
    dc[base + e] = dp * sc;
  }
  for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); }
  if ((tid & 63) == 0) { s_r[tid >> 6] = s0; s_r[4 + (tid >> 6)] = s1; }
  __syncthreads();
  if (tid == 0) {
    float* o = part + ((size_t)b * CO + co) * 2;
    o[0] = (s_r[0] + s_r[1]) + (s_r[2] + s_r[3]);
    o[1] = (s_r[4] + s_r[5]) + (s_r[6] + s_r[7]);
  }
}

__global__ __launch_bounds__(128) void hc_bn_sum_kernel(const float* __restrict__ part, float* __restrict__ dgamma, float* __restrict__ dbeta, int N, int CO) {
  const int co = threadIdx.x;
  if (co >= CO) return;
  dbeta[co] = ordered_sum(part + (size_t)co * 2, (size_t)CO * 2, N);
  dgamma[co] = ordered_sum(part + (size_t)co * 2 + 1, (size_t)CO * 2, N);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct HeadPlan {
  float *wp, *dc, *bn, *dwp;
  size_t total;
};

// one walk for both calls: the packed weights (forward: its own form; backward: the data gradient's), and the backward's
// dc, per-frame BatchNorm sums and per-slab weight-gradient partials
HeadPlan head_plan(void* scratch, int N, int H, int W, int Cin, int Cout) {
  HeadPlan p{};
  Carve c(scratch);
  const size_t HW = (size_t)H * W;
  p.wp = c.take<float>((size_t)9 * Cin * Cout);
  p.dc = c.take<float>((size_t)N * Cout * HW);
  p.bn = c.take<float>((size_t)N * Cout * 2);
  p.dwp = c.take<float>((size_t)geo_of(N, H, W).slabs * Cout * Cin * 9);
  p.total = c.bytes();
  return p;
}

bool bad_slope(double s) { return !(s >= 0.0 && s < 1.0); }

// ---- BatchNorm on the batch's own statistics, Dropout2d ---------------------------------------------------------------
// Every kernel below that walks a channel plane runs on grid (Cout, N) with 256 threads; a plane's sums are formed like
// hc_dpre_kernel's: a thread's strided elements in order, the wave's 64 by xor shuffles, the four waves as (0 + 1) + (2 + 3).

// the sum of one value per thread over the workgroup, in every thread; s_r: four floats nobody else uses
__device__ __forceinline__ float plane_sum(float v, float* s_r) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) s_r[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_r[0] + s_r[1]) + (s_r[2] + s_r[3]);
}

// part[(b CO + co) 2] = (the plane's mean, the plane's sum of squared distances from that mean): two passes over the plane
__global__ __launch_bounds__(256) void hb_plane_kernel(const float* __restrict__ c, float* __restrict__ part, int CO, size_t HW) {
  __shared__ float s_r[8];
  const int co = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* p = c + ((size_t)b * CO + co) * HW;
  float s = 0.f;
  for (size_t e = tid; e < HW; e += 256) s += p[e];
  const float mu = plane_sum(s, s_r) / (float)HW;
  float q = 0.f;
  for (size_t e = tid; e < HW; e += 256) {
    const float d = p[e] - mu;
    q = fmaf(d, d, q);
  }
  q = plane_sum(q, s_r + 4);
  if (tid == 0) {
    float* o = part + ((size_t)b * CO + co) * 2;
    o[0] = mu;
    o[1] = q;
  }
}

// Chan's merge of N planes of HW values each, in frame order: mean = (sum mean_b) / N,
// M2 = sum M2_b + HW sum (mean_b - mean)^2; var = M2 / (N HW); and the running statistics' update
__global__ __launch_bounds__(128) void hb_stats_kernel(const float* __restrict__ part, float* __restrict__ mean, float* __restrict__ invstd,
                                                       float* __restrict__ run_mean, float* __restrict__ run_var, int N, int CO, float hw,
                                                       float eps, float keep, float mom, float mom_unbiased) {
  const int co = threadIdx.x;
  if (co >= CO) return;
  const float* p = part + (size_t)co * 2;
  const float mu = ordered_sum(p, (size_t)CO * 2, N) / (float)N;
  const float within = ordered_sum(p + 1, (size_t)CO * 2, N);
  float between = 0.f;
  for (int b = 0; b < N; ++b) {
    const float d = p[(size_t)b * CO * 2] - mu;
    between = fmaf(d, d, between);
  }
  const float var = fmaf(hw, between, within) / ((float)N * hw);
  mean[co] = mu;
  invstd[co] = 1.f / sqrtf(var + eps);
  if (run_mean) run_mean[co] = fmaf(keep, run_mean[co], mom * mu);
  if (run_var) run_var[co] = fmaf(keep, run_var[co], mom_unbiased * var);
}

// y = act(gamma invstd (c - mean) + beta) drop[b, co]
__global__ __launch_bounds__(256) void hb_apply_kernel(const float* __restrict__ c, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const float* __restrict__ drop, float slope, float* __restrict__ y, int CO, size_t HW) {
  const int co = blockIdx.x, b = blockIdx.y;
  const size_t base = ((size_t)b * CO + co) * HW;
  const float sc = gamma[co] * invstd[co], mu = mean[co], be = beta[co];
  const float f = drop ? drop[(size_t)b * CO + co] : 1.f;
  for (size_t e = threadIdx.x; e < HW; e += 256) {
    const float v = fmaf(c[base + e] - mu, sc, be);
    y[base + e] = (v > 0.f ? v : slope * v) * f;
  }
}

// g = dy drop (y > 0 ? 1 : slope); part[(b CO + co) 2] = (sum g, sum g xhat), xhat = (c - mean) invstd
__global__ __launch_bounds__(256) void hb_dsum_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ c,
                                                      const float* __restrict__ mean, const float* __restrict__ invstd,
                                                      const float* __restrict__ drop, float slope, float* __restrict__ part, int CO, size_t HW) {
  __shared__ float s_r[8];
  const int co = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const size_t base = ((size_t)b * CO + co) * HW;
  const float mu = mean[co], is = invstd[co];
  const float f = drop ? drop[(size_t)b * CO + co] : 1.f;
  float s0 = 0.f, s1 = 0.f;
  for (size_t e = tid; e < HW; e += 256) {
    const float d = dy[base + e] * f;
    const float g = y[base + e] > 0.f ? d : slope * d;
    s0 += g;
    s1 = fmaf(g, (c[base + e] - mu) * is, s1);
  }
  s0 = plane_sum(s0, s_r);
  s1 = plane_sum(s1, s_r + 4);
  if (tid == 0) {
    float* o = part + ((size_t)b * CO + co) * 2;
    o[0] = s0;
    o[1] = s1;
  }
}

// dc = gamma invstd (g - dbeta / M - xhat dgamma / M)
__global__ __launch_bounds__(256) void hb_dc_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ c,
                                                    const float* __restrict__ gamma, const float* __restrict__ mean,
                                                    const float* __restrict__ invstd, const float* __restrict__ drop,
                                                    const float* __restrict__ dgamma, const float* __restrict__ dbeta, float slope,
                                                    float inv_m, float* __restrict__ dc, int CO, size_t HW) {
  const int co = blockIdx.x, b = blockIdx.y;
  const size_t base = ((size_t)b * CO + co) * HW;
  const float mu = mean[co], is = invstd[co], sc = gamma[co] * is;
  const float mb = dbeta[co] * inv_m, mg = dgamma[co] * inv_m;
  const float f = drop ? drop[(size_t)b * CO + co] : 1.f;
  for (size_t e = threadIdx.x; e < HW; e += 256) {
    const float d = dy[base + e] * f;
    const float g = y[base + e] > 0.f ? d : slope * d;
    const float xh = (c[base + e] - mu) * is;
    dc[base + e] = sc * ((g - mb) - xh * mg);
  }
}

// the draw of kp2d_dropout2d_mask (include/kp2d.h states the counter layout)
__host__ __device__ inline uint64_t drop_draw(uint64_t seed, uint32_t step, uint32_t layer, uint32_t n, uint32_t c) {
  return km_mix(km_mix(km_mix(seed + 0x9E3779B97F4A7C15ull) ^ (((uint64_t)step << 32) | layer)) ^ (((uint64_t)n << 32) | c));
}

__global__ __launch_bounds__(256) void hb_drop_kernel(float* __restrict__ drop, int N, int C, double p, float kept, uint64_t seed,
                                                      uint32_t step, uint32_t layer) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= N * C) return;
  const double u = (double)(drop_draw(seed, step, layer, (uint32_t)(e / C), (uint32_t)(e % C)) >> 11) * 0x1p-53;
  drop[e] = u >= p ? kept : 0.f;
}

}  // namespace

extern "C" {

size_t kp2d_cbr_train_scratch_bytes(int N, int H, int W, int Cin, int Cout) {
  int code;
  if (conv_shape_problem(N, H, W, Cin, Cout, true, &code)) return 0;
  return head_plan(nullptr, N, H, W, Cin, Cout).total;
}

int kp2d_cbr_forward_train(const float* x, const float* w, const float* scale, const float* shift, double slope, int N, int H,
                           int W, int Cin, int Cout, float* y, float* c, void* scratch, size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = conv_shape_problem(N, H, W, Cin, Cout, true, &code))
    return fail(code, "cbr_forward_train: %s (N %d, H %d, W %d, Cin %d, Cout %d)", why, N, H, W, Cin, Cout);
  if (bad_slope(slope)) return fail(KP2D_ERR_ARG, "cbr_forward_train: slope %g outside [0, 1)", slope);
  if (any_null(x, w, scale, shift, y, c, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, w, scale, shift, y, c) || misaligned(scratch, 16))
    return fail(KP2D_ERR_ARG, "cbr_forward_train: float arrays must be 4-byte aligned, scratch 16-byte");
  const HeadPlan p = head_plan(scratch, N, H, W, Cin, Cout);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_ARG, "cbr_forward_train scratch %zu B < required %zu B (kp2d_cbr_train_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  ConvA a{};
  a.scale = scale; a.shift = shift; a.c_out = c; a.y_out = y; a.slope = (float)slope;
  return conv_forward<false>({"cbr_forward_train", x, w, p.wp, N, H, W, Cin, Cout, st}, a);
}

int kp2d_cbr_backward(const float* x, const float* w, const float* scale, const float* mean, const float* invstd, double slope,
                      const float* y, const float* c, const float* dy, int N, int H, int W, int Cin, int Cout, float* d_weight,
                      float* d_gamma, float* d_beta, float* dx, void* scratch, size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = conv_shape_problem(N, H, W, Cin, Cout, true, &code))
    return fail(code, "cbr_backward: %s (N %d, H %d, W %d, Cin %d, Cout %d)", why, N, H, W, Cin, Cout);
  if (bad_slope(slope)) return fail(KP2D_ERR_ARG, "cbr_backward: slope %g outside [0, 1)", slope);
  if (any_null(x, w, scale, mean, invstd, y, c, dy, d_weight, d_gamma, d_beta, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, w, scale, mean, invstd, y, c, dy, d_weight, d_gamma, d_beta, dx) || misaligned(scratch, 16))
    return fail(KP2D_ERR_ARG, "cbr_backward: float arrays must be 4-byte aligned, scratch 16-byte");
  const HeadPlan p = head_plan(scratch, N, H, W, Cin, Cout);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_ARG, "cbr_backward scratch %zu B < required %zu B (kp2d_cbr_train_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  const size_t HW = (size_t)H * W;
  hipLaunchKernelGGL(hc_dpre_kernel, dim3(Cout, N), dim3(256), 0, st, dy, y, c, scale, mean, invstd, (float)slope, p.dc, p.bn, Cout, HW);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(hc_bn_sum_kernel, dim3(1), dim3(128), 0, st, p.bn, d_gamma, d_beta, N, Cout);
  HIP_TRY(hipGetLastError());
  return conv_backward_tail<false>({"cbr_backward", x, w, p.wp, N, H, W, Cin, Cout, st}, p.dc, p.dwp, d_weight, dx);
}

int kp2d_cbr_forward_batchnorm(const float* x, const float* w, const float* gamma, const float* beta, double eps, double slope,
                               const float* drop, double momentum, float* running_mean, float* running_var, int N, int H, int W,
                               int Cin, int Cout, float* y, float* c, float* mean, float* invstd, void* scratch,
                               size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = conv_shape_problem(N, H, W, Cin, Cout, true, &code))
    return fail(code, "cbr_forward_batchnorm: %s (N %d, H %d, W %d, Cin %d, Cout %d)", why, N, H, W, Cin, Cout);
  const double M = (double)N * H * W;
  if (M < 2.0) return fail(KP2D_ERR_ARG, "cbr_forward_batchnorm: batch statistics need N * H * W >= 2 values per channel, got %g", M);
  if (bad_slope(slope)) return fail(KP2D_ERR_ARG, "cbr_forward_batchnorm: slope %g outside [0, 1)", slope);
  if (!(eps >= 0.0 && eps < INFINITY)) return fail(KP2D_ERR_ARG, "cbr_forward_batchnorm: eps %g must be finite and not negative", eps);
  if (!(momentum >= 0.0 && momentum <= 1.0)) return fail(KP2D_ERR_ARG, "cbr_forward_batchnorm: momentum %g outside [0, 1]", momentum);
  if (any_null(x, w, gamma, beta, y, c, mean, invstd, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, w, gamma, beta, drop, running_mean, running_var, y, c, mean, invstd) || misaligned(scratch, 16))
    return fail(KP2D_ERR_ARG, "cbr_forward_batchnorm: float arrays must be 4-byte aligned, scratch 16-byte");
  const HeadPlan p = head_plan(scratch, N, H, W, Cin, Cout);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_ARG, "cbr_forward_batchnorm scratch %zu B < required %zu B (kp2d_cbr_train_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  const size_t HW = (size_t)H * W;
  ConvA a{};      // the plain result, no affine
  a.y_out = c;
  if (int e = conv_forward<false>({"cbr_forward_batchnorm", x, w, p.wp, N, H, W, Cin, Cout, st}, a)) return e;
  hipLaunchKernelGGL(hb_plane_kernel, dim3(Cout, N), dim3(256), 0, st, c, p.bn, Cout, HW);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(hb_stats_kernel, dim3(1), dim3(128), 0, st, p.bn, mean, invstd, running_mean, running_var, N, Cout, (float)HW,
                     (float)eps, (float)(1.0 - momentum), (float)momentum, (float)(momentum * (M / (M - 1.0))));
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(hb_apply_kernel, dim3(Cout, N), dim3(256), 0, st, c, gamma, beta, mean, invstd, drop, (float)slope, y, Cout, HW);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_cbr_backward_batchnorm(const float* x, const float* w, const float* gamma, const float* mean, const float* invstd,
                                double slope, const float* drop, const float* y, const float* c, const float* dy, int N, int H,
                                int W, int Cin, int Cout, float* d_weight, float* d_gamma, float* d_beta, float* dx, void* scratch,
                                size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = conv_shape_problem(N, H, W, Cin, Cout, true, &code))
    return fail(code, "cbr_backward_batchnorm: %s (N %d, H %d, W %d, Cin %d, Cout %d)", why, N, H, W, Cin, Cout);
  const double M = (double)N * H * W;
  if (M < 2.0) return fail(KP2D_ERR_ARG, "cbr_backward_batchnorm: batch statistics need N * H * W >= 2 values per channel, got %g", M);
  if (bad_slope(slope)) return fail(KP2D_ERR_ARG, "cbr_backward_batchnorm: slope %g outside [0, 1)", slope);
  if (any_null(x, w, gamma, mean, invstd, y, c, dy, d_weight, d_gamma, d_beta, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, w, gamma, mean, invstd, drop, y, c, dy, d_weight, d_gamma, d_beta, dx) || misaligned(scratch, 16))
    return fail(KP2D_ERR_ARG, "cbr_backward_batchnorm: float arrays must be 4-byte aligned, scratch 16-byte");
  const HeadPlan p = head_plan(scratch, N, H, W, Cin, Cout);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_ARG, "cbr_backward_batchnorm scratch %zu B < required %zu B (kp2d_cbr_train_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  const size_t HW = (size_t)H * W;
  hipLaunchKernelGGL(hb_dsum_kernel, dim3(Cout, N), dim3(256), 0, st, dy, y, c, mean, invstd, drop, (float)slope, p.bn, Cout, HW);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(hc_bn_sum_kernel, dim3(1), dim3(128), 0, st, p.bn, d_gamma, d_beta, N, Cout);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(hb_dc_kernel, dim3(Cout, N), dim3(256), 0, st, dy, y, c, gamma, mean, invstd, drop, d_gamma, d_beta, (float)slope,
                     (float)(1.0 / M), p.dc, Cout, HW);
  HIP_TRY(hipGetLastError());
  return conv_backward_tail<false>({"cbr_backward_batchnorm", x, w, p.wp, N, H, W, Cin, Cout, st}, p.dc, p.dwp, d_weight, dx);
}

int kp2d_dropout2d_mask(float* drop, int N, int C, double p, uint64_t seed, int64_t step, int layer, void* stream) {
  if (N < 1 || C < 1 || (int64_t)N * C > INT32_MAX) return fail(KP2D_ERR_ARG, "dropout2d_mask: N %d, C %d: needs N, C >= 1 and N * C < 2^31", N, C);
  if (!(p >= 0.0 && p < 1.0)) return fail(KP2D_ERR_ARG, "dropout2d_mask: p %g outside [0, 1)", p);
  if (step < 0 || step > (int64_t)UINT32_MAX || layer < 0) return fail(KP2D_ERR_ARG, "dropout2d_mask: step %lld outside [0, 2^32) or layer %d negative", (long long)step, layer);
  if (!drop) return fail(KP2D_ERR_ARG, "null argument");
  if (misaligned(drop, 4)) return fail(KP2D_ERR_ARG, "dropout2d_mask: drop must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(drop, st);
  hipLaunchKernelGGL(hb_drop_kernel, dim3((N * C + 255) / 256), dim3(256), 0, st, drop, N, C, p, (float)(1.0 / (1.0 - p)), seed, (uint32_t)step,
                     (uint32_t)layer);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

}  // extern "C"
