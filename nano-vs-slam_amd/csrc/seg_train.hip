// Fine-tuning of the segmentation head on the device (include/kp2d.h): what the V2 SegmentationHead of the reference
// (modules/decoders/segmentation.py:8-157) needs beside the Conv + BatchNorm + (Leaky)ReLU layers of vpr_head_train.hip.
//
//   kp2d_conv_bias_forward_train / _backward   the head's last layer, c = conv3x3(x, w) + bias with any 1 <= Cout <= 128: the
//                       implicit GEMMs of train_conv.h in their MASK form (Cout padded to a multiple of 16 in the packed
//                       weights, padded channels staged as zeros and never stored); dx is that kernel run on dy with dy's
//                       channels masked; sb_plane_kernel / sb_sum_kernel: dbias, a plane's sum and the frames in frame order
//   kp2d_seg_loss       ce_weight CE + dice_weight Dice over dense labels, two passes:
//     sl_sums_kernel    grid (groups <= 1024): a group walks a fixed run of 1024-pixel chunks; per chunk every thread forms the
//                       maximum, the sum of exponentials and the CE term of its four pixels, then wave w sums classes
//                       w, w + 4, ... over the chunk's pixels (lane l: pixels l, l + 64, ... in order, then the butterfly)
//     sl_merge_kernel   one block: the groups' partials in group order -> loss, valid, stray, and the per-class coefficients
//     sl_grad_kernel    a thread per pixel: the softmax again, dlogits; the probabilities are never stored
//   kp2d_maxpool2_*     2 x 2 stride-2 max pooling; the backward finds the argmax again (first maximum in row-major order)
//   kp2d_shuffle_cat_*  pixel shuffle by 2 of one tensor, concatenated with a second; backward of the shuffled part
// No float atomics; every cut depends on the shapes alone: bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "api_common.h"
#include "device_guard.h"
#include "train_common.h"
#include "train_conv.h"

using namespace kp2d;

namespace {

// ---- the last layer ----------------------------------------------------------------------------------------------------
struct BiasPlan {
  float *wp, *bp, *dwp;
  size_t total;
};

// the packed weights (padded), the per-frame bias sums and the per-slab weight-gradient partials
BiasPlan bias_plan(void* scratch, int N, int H, int W, int Cin, int Cout) {
  BiasPlan p{};
  Carve c(scratch);
  p.wp = c.take<float>((size_t)9 * Cin * pad16(Cout));
  p.bp = c.take<float>((size_t)N * Cout);
  p.dwp = c.take<float>((size_t)geo_of(N, H, W).slabs * Cout * Cin * 9);
  p.total = c.bytes();
  return p;
}

// part[b CO + co] = the sum of one plane of dy: a thread's strided elements in order, the wave's 64, the four waves
__global__ __launch_bounds__(256) void sb_plane_kernel(const float* __restrict__ dy, float* __restrict__ part, int CO, size_t HW) {
  __shared__ float s_r[4];
  const int co = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* p = dy + ((size_t)b * CO + co) * HW;
  float s = 0.f;
  for (size_t e = tid; e < HW; e += 256) s += p[e];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) s_r[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) part[(size_t)b * CO + co] = (s_r[0] + s_r[1]) + (s_r[2] + s_r[3]);
}

__global__ __launch_bounds__(128) void sb_sum_kernel(const float* __restrict__ part, float* __restrict__ dbias, int N, int CO) {
  const int co = threadIdx.x;
  if (co < CO) dbias[co] = ordered_sum(part + co, (size_t)CO, N);
}

// ---- the loss ------------------------------------------------------------------------------------------------------------
constexpr int LP = 1024;            // pixels of a chunk: four per thread
constexpr int MAX_GROUPS = 1024;
constexpr int MAX_CLASSES = 128;
constexpr float DICE_EPS = 1e-7f;

struct LossGeo {
  long long total, chunks, cpg;     // pixels, chunks, chunks per group
  int groups;
};

LossGeo loss_geo(int N, int64_t HW) {
  LossGeo g{};
  g.total = (long long)N * HW;
  g.chunks = (g.total + LP - 1) / LP;
  g.cpg = (g.chunks + MAX_GROUPS - 1) / MAX_GROUPS;
  g.groups = (int)((g.chunks + g.cpg - 1) / g.cpg);
  return g;
}

struct LossPlan {
  float* part;        // [groups][1 + 3 C]: the CE sum, then per class I, sum p, sum t
  long long* cnt;     // [groups][2]: valid, stray
  float* coef;        // [2 C + 1]: per class a and b of dDice / dp = a t + b (times dice_weight), then ce_weight / valid
  size_t total;
};

LossPlan loss_plan(void* scratch, int N, int64_t HW, int C) {
  LossPlan p{};
  Carve c(scratch);
  const LossGeo g = loss_geo(N, HW);
  p.cnt = c.take<long long>((size_t)g.groups * 2);
  p.part = c.take<float>((size_t)g.groups * (1 + 3 * C));
  p.coef = c.take<float>((size_t)2 * C + 1);
  p.total = c.bytes();
  return p;
}

// a label as a class of [0, C), -1: ignored, -2: stray
template <typename T>
__device__ __forceinline__ int class_of(const T* labels, long long gp, long long ignore, int C) {
  const long long v = (long long)labels[gp];
  if (ignore != KP2D_SEG_NO_IGNORE && v == ignore) return -1;
  return (v < 0 || v >= C) ? -2 : (int)v;
}

template <typename T>
__global__ __launch_bounds__(256) void sl_sums_kernel(const float* __restrict__ z, const T* __restrict__ labels, long long ignore, int C,
                                                      long long HW, LossGeo g, float* __restrict__ part, long long* __restrict__ cnt) {
  __shared__ float s_m[LP], s_s[LP];
  __shared__ int s_lab[LP];
  __shared__ long long s_base[LP];
  __shared__ float s_acc[3 * MAX_CLASSES];
  __shared__ float s_rf[4];
  __shared__ int s_ri[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < 3 * C; e += 256) s_acc[e] = 0.f;
  float ce = 0.f;
  int valid = 0, stray = 0;
  const long long q_end = ((long long)blockIdx.x + 1) * g.cpg < g.chunks ? ((long long)blockIdx.x + 1) * g.cpg : g.chunks;
  for (long long q = (long long)blockIdx.x * g.cpg; q < q_end; ++q) {
    __syncthreads();              // the previous chunk's class sums are done with the per-pixel values
#pragma unroll
    for (int i = 0; i < LP / 256; ++i) {
      const int pl = tid + 256 * i;
      const long long gp = q * LP + pl;
      int lab = -1;
      if (gp < g.total) {
        lab = class_of(labels, gp, ignore, C);
        if (lab == -2) ++stray;
      }
      if (lab >= 0) {
        const long long n = gp / HW, base = n * C * HW + (gp - n * HW);
        float m = z[base];
        for (int c = 1; c < C; ++c) m = fmaxf(m, z[base + (long long)c * HW]);
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(z[base + (long long)c * HW] - m);
        ce += (m - z[base + (long long)lab * HW]) + logf(s);
        ++valid;
        s_m[pl] = m;
        s_s[pl] = s;
        s_base[pl] = base;
      }
      s_lab[pl] = lab;
    }
    __syncthreads();
    for (int c = wave; c < C; c += 4) {
      float si = 0.f, sp = 0.f, st = 0.f;
      for (int pl = lane; pl < LP; pl += 64) {
        const int lab = s_lab[pl];
        if (lab < 0) continue;
        const float p = expf(z[s_base[pl] + (long long)c * HW] - s_m[pl]) / s_s[pl];
        sp += p;
        if (lab == c) { si += p; st += 1.f; }
      }
      for (int o = 32; o > 0; o >>= 1) { si += __shfl_xor(si, o); sp += __shfl_xor(sp, o); st += __shfl_xor(st, o); }
      if (lane == 0) { s_acc[3 * c] += si; s_acc[3 * c + 1] += sp; s_acc[3 * c + 2] += st; }      // class c belongs to this wave alone
    }
  }
  for (int o = 32; o > 0; o >>= 1) { ce += __shfl_xor(ce, o); valid += __shfl_xor(valid, o); stray += __shfl_xor(stray, o); }
  if (lane == 0) { s_rf[wave] = ce; s_ri[wave] = valid; s_ri[4 + wave] = stray; }
  __syncthreads();
  float* o = part + (size_t)blockIdx.x * (1 + 3 * C);
  for (int e = tid; e < 3 * C; e += 256) o[1 + e] = s_acc[e];
  if (tid == 0) {
    o[0] = (s_rf[0] + s_rf[1]) + (s_rf[2] + s_rf[3]);
    cnt[(size_t)blockIdx.x * 2] = (long long)s_ri[0] + s_ri[1] + s_ri[2] + s_ri[3];
    cnt[(size_t)blockIdx.x * 2 + 1] = (long long)s_ri[4] + s_ri[5] + s_ri[6] + s_ri[7];
  }
}

__global__ __launch_bounds__(256) void sl_merge_kernel(const float* __restrict__ part, const long long* __restrict__ cnt, int groups, int C,
                                                       float wce, float wdice, float* __restrict__ coef, float* __restrict__ loss,
                                                       long long* __restrict__ valid_out, long long* __restrict__ stray_out) {
  __shared__ float s_tot[1 + 3 * MAX_CLASSES];
  __shared__ float s_term[MAX_CLASSES];
  const int tid = threadIdx.x, Q = 1 + 3 * C;
  for (int q = tid; q < Q; q += 256) s_tot[q] = ordered_sum(part + q, (size_t)Q, groups);
  __syncthreads();
  if (tid < C) {
    const float I = s_tot[1 + 3 * tid], S = s_tot[2 + 3 * tid] + s_tot[3 + 3 * tid];
    const bool present = s_tot[3 + 3 * tid] > 0.f;
    const float D = fmaxf(S, DICE_EPS);
    s_term[tid] = present ? 1.f - 2.f * I / D : 0.f;
    coef[tid] = present ? wdice * (-2.f / ((float)C * D)) : 0.f;
    coef[C + tid] = present && S > DICE_EPS ? wdice * (2.f * I / ((float)C * D * D)) : 0.f;
  }
  __syncthreads();
  if (tid == 0) {
    long long valid = 0, stray = 0;
    for (int g = 0; g < groups; ++g) { valid += cnt[(size_t)g * 2]; stray += cnt[(size_t)g * 2 + 1]; }
    float dice = 0.f;
    for (int c = 0; c < C; ++c) dice += s_term[c];
    dice /= (float)C;
    const float ce = valid > 0 ? s_tot[0] / (float)valid : 0.f;
    coef[2 * C] = valid > 0 ? wce / (float)valid : 0.f;
    *loss = wce * ce + wdice * dice;
    *valid_out = valid;
    *stray_out = stray;
  }
}

// dz_j = (ce_weight / valid) (p_j - t_j) + p_j (g_j - sum_c p_c g_c),  g_c = a_c t_c + b_c
template <typename T>
__global__ __launch_bounds__(256) void sl_grad_kernel(const float* __restrict__ z, const T* __restrict__ labels, long long ignore, int C,
                                                      long long HW, long long total, const float* __restrict__ coef,
                                                      float* __restrict__ dz) {
  __shared__ float s_coef[2 * MAX_CLASSES + 1];
  for (int e = threadIdx.x; e < 2 * C + 1; e += 256) s_coef[e] = coef[e];
  __syncthreads();
  const long long gp = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gp >= total) return;
  const long long n = gp / HW, base = n * C * HW + (gp - n * HW);
  const int lab = class_of(labels, gp, ignore, C);
  if (lab < 0) {
    for (int c = 0; c < C; ++c) dz[base + (long long)c * HW] = 0.f;
    return;
  }
  float m = z[base];
  for (int c = 1; c < C; ++c) m = fmaxf(m, z[base + (long long)c * HW]);
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += expf(z[base + (long long)c * HW] - m);
  const float a = s_coef[lab], k = s_coef[2 * C];
  float dot = 0.f;
  for (int c = 0; c < C; ++c) {
    const float p = expf(z[base + (long long)c * HW] - m) / s;
    dot = fmaf(p, s_coef[C + c] + (c == lab ? a : 0.f), dot);
  }
  for (int c = 0; c < C; ++c) {
    const float p = expf(z[base + (long long)c * HW] - m) / s;
    const float gc = s_coef[C + c] + (c == lab ? a : 0.f);
    dz[base + (long long)c * HW] = fmaf(k, p - (c == lab ? 1.f : 0.f), p * (gc - dot));
  }
}

// ---- 2 x 2 max pooling ---------------------------------------------------------------------------------------------------
// torch's rule: a later element replaces the maximum when it is greater or NaN, so the first maximum in row-major order wins
__device__ __forceinline__ int window_argmax(const float* __restrict__ p, int W, float* best) {
  float b = p[0];
  int at = 0;
  const float v1 = p[1], v2 = p[W], v3 = p[W + 1];
  if (v1 > b || v1 != v1) { b = v1; at = 1; }
  if (v2 > b || v2 != v2) { b = v2; at = 2; }
  if (v3 > b || v3 != v3) { b = v3; at = 3; }
  *best = b;
  return at;
}

__global__ __launch_bounds__(256) void mp_forward_kernel(const float* __restrict__ x, float* __restrict__ y, long long planes, int H, int W) {
  const int Ho = H / 2, Wo = W / 2;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= planes * Ho * Wo) return;
  const int j = (int)(e % Wo), i = (int)((e / Wo) % Ho);
  const long long pl = e / ((long long)Wo * Ho);
  float best;
  window_argmax(x + pl * H * W + (long long)(2 * i) * W + 2 * j, W, &best);
  y[e] = best;
}

__global__ __launch_bounds__(256) void mp_backward_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                                          long long planes, int H, int W) {
  const int Ho = H / 2, Wo = W / 2;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= planes * H * W) return;
  const int xx = (int)(e % W), yy = (int)((e / W) % H);
  const long long pl = e / ((long long)W * H);
  const int i = yy >> 1, j = xx >> 1;
  float v = 0.f;      // a last odd row or column is in no window
  if (i < Ho && j < Wo) {
    float best;
    const int at = window_argmax(x + pl * H * W + (long long)(2 * i) * W + 2 * j, W, &best);
    if (at == 2 * (yy & 1) + (xx & 1)) v = dy[pl * Ho * Wo + (long long)i * Wo + j];
  }
  dx[e] = v;
}

// ---- pixel shuffle + concatenation -----------------------------------------------------------------------------------------
// out[n, c, 2 i + a, 2 j + b] = A[n, 4 c + 2 a + b, i, j] (c < C);  out[n, C + cb] = B[n, cb]
__global__ __launch_bounds__(256) void sc_forward_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ out,
                                                         int N, int C, int Cb, int h, int w) {
  const int H = 2 * h, W = 2 * w;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)N * (C + Cb) * H * W) return;
  const int x = (int)(e % W), y = (int)((e / W) % H);
  const long long pc = e / ((long long)W * H);
  const int ch = (int)(pc % (C + Cb));
  const long long n = pc / (C + Cb);
  if (ch < C) out[e] = A[((n * 4 * C + 4 * ch + 2 * (y & 1) + (x & 1)) * h + (y >> 1)) * w + (x >> 1)];
  else out[e] = B[((n * Cb + (ch - C)) * H + y) * W + x];
}

// dA[n, 4 c + 2 a + b, i, j] = dout[n, c, 2 i + a, 2 j + b]
__global__ __launch_bounds__(256) void sc_backward_kernel(const float* __restrict__ dout, float* __restrict__ dA, int N, int C, int Cb, int h,
                                                          int w) {
  const int H = 2 * h, W = 2 * w;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)N * 4 * C * h * w) return;
  const int j = (int)(e % w), i = (int)((e / w) % h);
  const long long pk = e / ((long long)w * h);
  const int kk = (int)(pk % (4 * C));
  const long long n = pk / (4 * C);
  dA[e] = dout[((n * (C + Cb) + (kk >> 2)) * H + 2 * i + ((kk >> 1) & 1)) * W + 2 * j + (kk & 1)];
}

constexpr long long MAX_ELEMS = 1ll << 38;      // of a pool or shuffle tensor: the grid of 256-thread blocks stays below 2^31

const char* plane_problem(int N, int C, int H, int W, int* code) {
  *code = KP2D_ERR_ARG;
  if (N < 1 || C < 1 || H < 1 || W < 1) return "N, C, H and W must be at least 1";
  *code = KP2D_ERR_UNSUPPORTED;
  if ((long long)N * C > MAX_ELEMS / H / W) return "more than 2^38 elements";
  return nullptr;
}

unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" {

size_t kp2d_conv_bias_scratch_bytes(int N, int H, int W, int Cin, int Cout) {
  int code;
  if (conv_shape_problem(N, H, W, Cin, Cout, false, &code)) return 0;
  return bias_plan(nullptr, N, H, W, Cin, Cout).total;
}

int kp2d_conv_bias_forward_train(const float* x, const float* w, const float* bias, int N, int H, int W, int Cin, int Cout, float* y,
                                 void* scratch, size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = conv_shape_problem(N, H, W, Cin, Cout, false, &code))
    return fail(code, "conv_bias_forward_train: %s (N %d, H %d, W %d, Cin %d, Cout %d)", why, N, H, W, Cin, Cout);
  if (any_null(x, w, bias, y, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, w, bias, y) || misaligned(scratch, 16))
    return fail(KP2D_ERR_ARG, "conv_bias_forward_train: float arrays must be 4-byte aligned, scratch 16-byte");
  const BiasPlan p = bias_plan(scratch, N, H, W, Cin, Cout);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_ARG, "conv_bias_forward_train scratch %zu B < required %zu B (kp2d_conv_bias_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  ConvMA a{};
  a.y_out = y; a.bias = bias;
  return conv_forward<true>({"conv_bias_forward_train", x, w, p.wp, N, H, W, Cin, Cout, st}, a);
}

int kp2d_conv_bias_backward(const float* x, const float* w, const float* dy, int N, int H, int W, int Cin, int Cout, float* d_weight,
                            float* d_bias, float* dx, void* scratch, size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = conv_shape_problem(N, H, W, Cin, Cout, false, &code))
    return fail(code, "conv_bias_backward: %s (N %d, H %d, W %d, Cin %d, Cout %d)", why, N, H, W, Cin, Cout);
  if (any_null(x, w, dy, d_weight, d_bias, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, w, dy, d_weight, d_bias, dx) || misaligned(scratch, 16))
    return fail(KP2D_ERR_ARG, "conv_bias_backward: float arrays must be 4-byte aligned, scratch 16-byte");
  const BiasPlan p = bias_plan(scratch, N, H, W, Cin, Cout);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_ARG, "conv_bias_backward scratch %zu B < required %zu B (kp2d_conv_bias_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  hipLaunchKernelGGL(sb_plane_kernel, dim3(Cout, N), dim3(256), 0, st, dy, p.bp, Cout, (size_t)H * W);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(sb_sum_kernel, dim3(1), dim3(128), 0, st, p.bp, d_bias, N, Cout);
  HIP_TRY(hipGetLastError());
  return conv_backward_tail<true>({"conv_bias_backward", x, w, p.wp, N, H, W, Cin, Cout, st}, dy, p.dwp, d_weight, dx);
}

static const char* loss_shape_problem(int N, int64_t HW, int C, int* code) {
  *code = KP2D_ERR_ARG;
  if (N < 1 || N > 65535) return "N outside [1, 65535]";
  if (HW < 1) return "H * W must be at least 1";
  if (C < 1) return "C must be at least 1";
  *code = KP2D_ERR_UNSUPPORTED;
  if (C > MAX_CLASSES) return "C above 128";
  if (HW > ((int64_t)1 << 30)) return "H * W above 2^30";
  return nullptr;
}

size_t kp2d_seg_loss_scratch_bytes(int N, int64_t HW, int C) {
  int code;
  if (loss_shape_problem(N, HW, C, &code)) return 0;
  return loss_plan(nullptr, N, HW, C).total;
}

int kp2d_seg_loss(const float* logits, const void* labels, int label_dtype, int N, int64_t HW, int C, int64_t ignore_index,
                  double ce_weight, double dice_weight, float* loss, float* dlogits, int64_t* valid, int64_t* stray, void* scratch,
                  size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = loss_shape_problem(N, HW, C, &code)) return fail(code, "seg_loss: %s (N %d, HW %lld, C %d)", why, N, (long long)HW, C);
  if (label_dtype != KP2D_SEG_U8 && label_dtype != KP2D_SEG_I32 && label_dtype != KP2D_SEG_I64)
    return fail(KP2D_ERR_ARG, "seg_loss: label_dtype = %d (KP2D_SEG_U8, KP2D_SEG_I32 or KP2D_SEG_I64)", label_dtype);
  if (!(ce_weight >= 0.0 && ce_weight < INFINITY && dice_weight >= 0.0 && dice_weight < INFINITY))
    return fail(KP2D_ERR_ARG, "seg_loss: weights %g, %g must be finite and not negative", ce_weight, dice_weight);
  if (any_null(logits, labels, loss, dlogits, valid, stray, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(logits, loss, dlogits) || misaligned(valid, 8) || misaligned(stray, 8) || misaligned(scratch, 16) ||
      (label_dtype == KP2D_SEG_I64 && misaligned(labels, 8)) || (label_dtype == KP2D_SEG_I32 && misaligned(labels, 4)))
    return fail(KP2D_ERR_ARG, "seg_loss: misaligned argument");
  const LossPlan p = loss_plan(scratch, N, HW, C);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_ARG, "seg_loss scratch %zu B < required %zu B (kp2d_seg_loss_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(logits, st);
  const LossGeo g = loss_geo(N, HW);
  const long long ign = (long long)ignore_index, hw = (long long)HW;
  if (label_dtype == KP2D_SEG_U8)
    hipLaunchKernelGGL(sl_sums_kernel<uint8_t>, dim3(g.groups), dim3(256), 0, st, logits, (const uint8_t*)labels, ign, C, hw, g, p.part, p.cnt);
  else if (label_dtype == KP2D_SEG_I32)
    hipLaunchKernelGGL(sl_sums_kernel<int32_t>, dim3(g.groups), dim3(256), 0, st, logits, (const int32_t*)labels, ign, C, hw, g, p.part, p.cnt);
  else
    hipLaunchKernelGGL(sl_sums_kernel<int64_t>, dim3(g.groups), dim3(256), 0, st, logits, (const int64_t*)labels, ign, C, hw, g, p.part, p.cnt);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(sl_merge_kernel, dim3(1), dim3(256), 0, st, p.part, p.cnt, g.groups, C, (float)ce_weight, (float)dice_weight, p.coef, loss,
                     (long long*)valid, (long long*)stray);
  HIP_TRY(hipGetLastError());
  const dim3 grid(blocks_of(g.total));
  if (label_dtype == KP2D_SEG_U8)
    hipLaunchKernelGGL(sl_grad_kernel<uint8_t>, grid, dim3(256), 0, st, logits, (const uint8_t*)labels, ign, C, hw, g.total, p.coef, dlogits);
  else if (label_dtype == KP2D_SEG_I32)
    hipLaunchKernelGGL(sl_grad_kernel<int32_t>, grid, dim3(256), 0, st, logits, (const int32_t*)labels, ign, C, hw, g.total, p.coef, dlogits);
  else
    hipLaunchKernelGGL(sl_grad_kernel<int64_t>, grid, dim3(256), 0, st, logits, (const int64_t*)labels, ign, C, hw, g.total, p.coef, dlogits);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_maxpool2_forward_train(const float* x, int N, int C, int H, int W, float* y, void* stream) {
  int code;
  if (const char* why = plane_problem(N, C, H, W, &code)) return fail(code, "maxpool2_forward_train: %s (N %d, C %d, H %d, W %d)", why, N, C, H, W);
  if (H < 2 || W < 2) return fail(KP2D_ERR_ARG, "maxpool2_forward_train: H %d and W %d must be at least 2", H, W);
  if (any_null(x, y)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, y)) return fail(KP2D_ERR_ARG, "maxpool2_forward_train: float arrays must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  const long long planes = (long long)N * C;
  hipLaunchKernelGGL(mp_forward_kernel, dim3(blocks_of(planes * (H / 2) * (W / 2))), dim3(256), 0, st, x, y, planes, H, W);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_maxpool2_backward(const float* x, const float* dy, int N, int C, int H, int W, float* dx, void* stream) {
  int code;
  if (const char* why = plane_problem(N, C, H, W, &code)) return fail(code, "maxpool2_backward: %s (N %d, C %d, H %d, W %d)", why, N, C, H, W);
  if (H < 2 || W < 2) return fail(KP2D_ERR_ARG, "maxpool2_backward: H %d and W %d must be at least 2", H, W);
  if (any_null(x, dy, dx)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, dy, dx)) return fail(KP2D_ERR_ARG, "maxpool2_backward: float arrays must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  const long long planes = (long long)N * C;
  hipLaunchKernelGGL(mp_backward_kernel, dim3(blocks_of(planes * H * W)), dim3(256), 0, st, x, dy, dx, planes, H, W);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

static const char* shuffle_problem(int N, int C, int Cb, int h, int w, int* code) {
  *code = KP2D_ERR_ARG;
  if (N < 1 || C < 1 || Cb < 0 || h < 1 || w < 1) return "N, C, h and w must be at least 1 and Cb at least 0";
  *code = KP2D_ERR_UNSUPPORTED;
  if (h > (1 << 20) || w > (1 << 20) || (long long)N * ((long long)C + Cb) > MAX_ELEMS / (4ll * h * w)) return "more than 2^38 elements";
  return nullptr;
}

int kp2d_shuffle_cat_forward(const float* a, const float* b, int N, int C, int Cb, int h, int w, float* out, void* stream) {
  int code;
  if (const char* why = shuffle_problem(N, C, Cb, h, w, &code)) return fail(code, "shuffle_cat_forward: %s (N %d, C %d, Cb %d, h %d, w %d)", why, N, C, Cb, h, w);
  if (!a || (!b && Cb > 0) || !out) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(a, b, out)) return fail(KP2D_ERR_ARG, "shuffle_cat_forward: float arrays must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(a, st);
  hipLaunchKernelGGL(sc_forward_kernel, dim3(blocks_of((long long)N * (C + Cb) * 4 * h * w)), dim3(256), 0, st, a, b, out, N, C, Cb, h, w);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_shuffle_cat_backward(const float* dout, int N, int C, int Cb, int h, int w, float* da, void* stream) {
  int code;
  if (const char* why = shuffle_problem(N, C, Cb, h, w, &code)) return fail(code, "shuffle_cat_backward: %s (N %d, C %d, Cb %d, h %d, w %d)", why, N, C, Cb, h, w);
  if (any_null(dout, da)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(dout, da)) return fail(KP2D_ERR_ARG, "shuffle_cat_backward: float arrays must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(dout, st);
  hipLaunchKernelGGL(sc_backward_kernel, dim3(blocks_of((long long)N * 4 * C * h * w)), dim3(256), 0, st, dout, da, N, C, Cb, h, w);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

}  // extern "C"
