// Training of the V2 attention head's SegFormerAttentionModule on the device (include/kp2d.h): every stage's forward, which
// returns what its backward needs, and every stage's backward.  Exact fp32; the matrix products run on
// v_mfma_f32_16x16x4_f32 (bit for bit an fma chain over the reduction index in ascending order); the attention logits alone
// are float64 on v_mfma_f64_16x16x4_f64 (logit_tile says why).
//
//   ln_*               the reference's channel LayerNorm, a thread per pixel; dg and db: lnsum_plane_kernel sums a (frame,
//                      channel) plane (thread t: pixels t, t + 256, ... in order, the wave's butterfly, the four waves),
//                      strided_sum_kernel adds the frames in frame order
//   pw_kernel<MODE>    y[m][p] = sum_k A[m][k] B[k][p]: a wave owns 16 pixels and walks the 16-row tiles of the output;
//                      MODE 0: a 1 x 1 convolution (forward, or dx with the weights read transposed), MODE 1: to_kv's 2 x 2
//                      stride-2 patches read in place (k = 4 ci + 2 a + b), MODE 2: to_kv's dx, stored to the patches' pixels
//   pw_dw_kernel<MODE> dw[m][k] = sum_p dy[m][p] X[k][p] over a slab, a fixed run of pixels in (frame, pixel) order, one
//                      partial per slab (at most 128), added in slab order by strided_sum_kernel
//   dwc_*              depthwise 3 x 3 (padding 1, bias): forward and dx a thread per element, dw and dbias per plane as above
//   att_fwd_kernel     a wave per (16 queries, head, frame): online softmax over key tiles of 16 in ascending order; stores O
//                      and one log-sum-exp per query (with what its rounding dropped), nothing of size S x T; logit_tile: the logits in float64
//   att_delta_kernel   delta = sum_c dO O, as the diagonal of the same MFMA chain that forms dO V^T
//   att_dq_kernel      a wave per 16 queries walks the keys in ascending order: P again from q, k and the log-sum-exp, dQ
//   att_dkv_kernel     a wave per 16 keys walks the queries in ascending order: dK and dV (the receiving side scans)
// No float atomics; every cut depends on the shapes alone: bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "api_common.h"
#include "device_guard.h"
#include "train_common.h"

using namespace kp2d;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int HEADS = 4;
constexpr int MAX_SLABS = 128;
constexpr int MIN_SLAB = 64;              // pixels of the smallest slab
constexpr long long MAX_HW = 1ll << 24;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

// ---- sums over pixels ------------------------------------------------------------------------------------------------------
// out[e] = part[e] + part[e + stride] + ... (count terms, in that order)
__global__ __launch_bounds__(256) void strided_sum_kernel(const float* __restrict__ part, size_t stride, int count, float* __restrict__ out, int n) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) out[e] = ordered_sum(part + e, stride, count);
}

__device__ __forceinline__ float block_sum(float s, float* s_r) {      // every thread calls; valid in thread 0
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_r[threadIdx.x >> 6] = s;
  __syncthreads();
  return (s_r[0] + s_r[1]) + (s_r[2] + s_r[3]);
}

// part[b 2C + c] = sum_p dy (x - mean) rinv (xm given) and part[b 2C + C + c] = sum_p dy; without xm: part[b C + c] = sum_p dy
__global__ __launch_bounds__(256) void lnsum_plane_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                          const float* __restrict__ rinv, float* __restrict__ part, int C, size_t HW) {
  __shared__ float s_r[4];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* p = dy + ((size_t)b * C + c) * HW;
  float sb = 0.f, sg = 0.f;
  if (x) {
    const float* px = x + ((size_t)b * C + c) * HW;
    const float* pm = mean + (size_t)b * HW;
    const float* pr = rinv + (size_t)b * HW;
    for (size_t e = tid; e < HW; e += 256) {
      const float g = p[e];
      sb += g;
      sg += g * ((px[e] - pm[e]) * pr[e]);
    }
    sg = block_sum(sg, s_r);
    sb = block_sum(sb, s_r);
    if (tid == 0) { part[(size_t)b * 2 * C + c] = sg; part[(size_t)b * 2 * C + C + c] = sb; }
  } else {
    for (size_t e = tid; e < HW; e += 256) sb += p[e];
    sb = block_sum(sb, s_r);
    if (tid == 0) part[(size_t)b * C + c] = sb;
  }
}

// ---- channel LayerNorm -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ln_forward_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ bb,
                                                         float eps, int C, long long HW, long long total, float* __restrict__ y,
                                                         float* __restrict__ mean, float* __restrict__ rinv) {
  const long long gp = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gp >= total) return;
  const long long n = gp / HW, base = n * C * HW + (gp - n * HW);
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += x[base + c * HW];
  const float mu = s / (float)C;
  float v = 0.f;
  for (int c = 0; c < C; ++c) { const float d = x[base + c * HW] - mu; v = fmaf(d, d, v); }
  const float D = sqrtf(v / (float)C) + eps;
  for (int c = 0; c < C; ++c) y[base + c * HW] = fmaf((x[base + c * HW] - mu) / D, g[c], bb[c]);
  mean[gp] = mu;
  rinv[gp] = 1.f / D;
}

// dx = (a - mean_c a) / D - d (sum_c a d) / (C s D^2), a = g dy, d = x - mean, s = sqrt(var), D = s + eps; s = 0: second term 0
__global__ __launch_bounds__(256) void ln_backward_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ mean,
                                                          const float* __restrict__ dy, float eps, int C, long long HW, long long total,
                                                          float* __restrict__ dx) {
  const long long gp = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gp >= total) return;
  const long long n = gp / HW, base = n * C * HW + (gp - n * HW);
  const float mu = mean[gp];
  float v = 0.f, sa = 0.f, sad = 0.f;
  for (int c = 0; c < C; ++c) {
    const float d = x[base + c * HW] - mu, a = g[c] * dy[base + c * HW];
    v = fmaf(d, d, v);
    sa += a;
    sad = fmaf(a, d, sad);
  }
  const float s = sqrtf(v / (float)C), D = s + eps;
  const float ma = sa / (float)C;
  const float k = s > 0.f ? sad / ((float)C * s * D * D) : 0.f;
  for (int c = 0; c < C; ++c) {
    const float d = x[base + c * HW] - mu, a = g[c] * dy[base + c * HW];
    dx[base + c * HW] = (a - ma) / D - d * k;
  }
}

// ---- pointwise products ------------------------------------------------------------------------------------------------------
struct PwA {
  const float* x;       // the B operand's tensor
  const float* w;       // the A operand: element (m, k) at w[m a_rs + k a_ks]
  const float* bias;    // [M] or null
  float* y;
  float* pre;           // with gelu: the value before it
  int M, K, a_rs, a_ks;
  int C, H, W, Wo;      // MODE 1, 2: the full map and its channels; the pixels are the Ho x Wo patches
  int P;                // pixels of a frame on the product's pixel axis
  int gelu;
};

__device__ __forceinline__ float gelu_exact(float v) { return v * 0.5f * (1.f + erff(v * 0.70710678118654752440f)); }

// element (k, pixel p of frame b) of the B operand
template <int MODE>
__device__ __forceinline__ float pw_b(const PwA& a, int b, int k, int p) {
  if (MODE == 1) {
    const int i = p / a.Wo, j = p - i * a.Wo;
    return a.x[((size_t)b * a.C + (k >> 2)) * a.H * a.W + (size_t)(2 * i + ((k >> 1) & 1)) * a.W + 2 * j + (k & 1)];
  }
  return a.x[((size_t)b * a.K + k) * a.P + p];
}

template <int MODE>
__global__ __launch_bounds__(256) void pw_kernel(const PwA a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, k = lane >> 4;
  const int b = blockIdx.y, p = blockIdx.x * 64 + wave * 16 + j;
  const bool live = p < a.P;
  size_t obase = 0;       // MODE 2: the patch's first pixel
  if (MODE == 2 && live) {
    const int i = p / a.Wo, jj = p - i * a.Wo;
    obase = (size_t)(2 * i) * a.W + 2 * jj;
  }
  for (int n = 0; n < a.M / 16; ++n) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < a.K / 4; ++kk) {
      const int ki = 4 * kk + k;
      const float av = a.w[(size_t)(16 * n + j) * a.a_rs + (size_t)ki * a.a_ks];
      const float bv = live ? pw_b<MODE>(a, b, ki, p) : 0.f;
      acc = mfma4(av, bv, acc);
    }
    if (!live) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {       // register r of lane (j, k): row 16 n + 4 k + r at pixel p
      const int m = 16 * n + 4 * k + r;
      float v = acc[r];
      if (a.bias) v += a.bias[m];
      if (MODE == 2) {
        a.y[((size_t)b * a.C + (m >> 2)) * a.H * a.W + obase + (size_t)((m >> 1) & 1) * a.W + (m & 1)] = v;
        continue;
      }
      const size_t idx = ((size_t)b * a.M + m) * a.P + p;
      if (a.gelu) { a.pre[idx] = v; v = gelu_exact(v); }
      a.y[idx] = v;
    }
  }
}

// the pixels no 2 x 2 patch covers (an odd map's last row or column): exact zeros
__global__ __launch_bounds__(256) void patch_rim_kernel(float* __restrict__ dx, long long planes, int H, int W) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= planes * H * W) return;
  const int xx = (int)(e % W), yy = (int)((e / W) % H);
  if (yy >= 2 * (H / 2) || xx >= 2 * (W / 2)) dx[e] = 0.f;
}

struct DwA {
  const float* dy;      // [N][M][P]
  const float* x;
  float* part;          // [slabs][M][K]
  long long total, pps; // pixels of all frames, pixels per slab (a multiple of 4)
  int M, K;
  int C, H, W, Wo, P;
};

template <int MODE>
__global__ __launch_bounds__(256) void pw_dw_kernel(const DwA a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, k = lane >> 4;
  const int kcol = blockIdx.y * 16 + j;
  const int NT = a.M / 16;
  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const long long g0 = (long long)blockIdx.x * a.pps;
  const long long g1 = g0 + a.pps < a.total ? g0 + a.pps : a.total;
  PwA v{};
  v.x = a.x; v.K = a.K; v.C = a.C; v.H = a.H; v.W = a.W; v.Wo = a.Wo; v.P = a.P;
  for (long long g = g0; g < g1; g += 4) {
    const long long gp = g + k;
    const bool live = gp < g1;
    const int b = live ? (int)(gp / a.P) : 0, p = live ? (int)(gp - (long long)b * a.P) : 0;
    const float bv = live ? pw_b<MODE>(v, b, kcol, p) : 0.f;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int n = wave + 4 * it;
      if (n < NT) {
        const float av = live ? a.dy[((size_t)b * a.M + 16 * n + j) * a.P + p] : 0.f;
        acc[it] = mfma4(av, bv, acc[it]);
      }
    }
  }
  float* dst = a.part + (size_t)blockIdx.x * a.M * a.K;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int n = wave + 4 * it;
    if (n < NT)
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[(size_t)(16 * n + 4 * k + r) * a.K + kcol] = acc[it][r];
  }
}

// dpre = dy gelu'(pre), gelu'(v) = Phi(v) + v phi(v)
__global__ __launch_bounds__(256) void gelu_backward_kernel(const float* __restrict__ pre, const float* __restrict__ dy, float* __restrict__ dpre,
                                                            long long n) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const float v = pre[e];
  const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752440f));
  const float pdf = expf(-0.5f * v * v) * 0.39894228040143267794f;
  dpre[e] = dy[e] * fmaf(v, pdf, cdf);
}

// ---- depthwise 3 x 3 -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dwc_forward_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ y, long long total, int C, int H, int W) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int xx = (int)(e % W), yy = (int)((e / W) % H);
  const long long pl = e / ((long long)W * H);
  const int c = (int)(pl % C);
  const float* px = x + pl * H * W;
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int gy = yy + t / 3 - 1, gx = xx + t % 3 - 1;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) s = fmaf(w[c * 9 + t], px[(long long)gy * W + gx], s);
  }
  y[e] = s + bias[c];
}

// dx[y][x] = sum_t w[t] dy[y - (ky - 1)][x - (kx - 1)]
__global__ __launch_bounds__(256) void dwc_dx_kernel(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx,
                                                     long long total, int C, int H, int W) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int xx = (int)(e % W), yy = (int)((e / W) % H);
  const long long pl = e / ((long long)W * H);
  const int c = (int)(pl % C);
  const float* pd = dy + pl * H * W;
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int gy = yy - (t / 3 - 1), gx = xx - (t % 3 - 1);
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) s = fmaf(w[c * 9 + t], pd[(long long)gy * W + gx], s);
  }
  dx[e] = s;
}

// part[b 10 C + 9 c + t] = sum_p dy[p] x[p shifted by tap t], part[b 10 C + 9 C + c] = sum_p dy[p]
__global__ __launch_bounds__(256) void dwc_dw_plane_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part,
                                                           int C, int H, int W) {
  __shared__ float s_r[4];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const long long HW = (long long)H * W;
  const float* px = x + ((long long)b * C + c) * HW;
  const float* pd = dy + ((long long)b * C + c) * HW;
  float s[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) s[t] = 0.f;
  for (long long e = tid; e < HW; e += 256) {
    const int xx = (int)(e % W), yy = (int)(e / W);
    const float g = pd[e];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int gy = yy + t / 3 - 1, gx = xx + t % 3 - 1;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) s[t] = fmaf(g, px[(long long)gy * W + gx], s[t]);
    }
    s[9] += g;
  }
#pragma unroll
  for (int t = 0; t < 10; ++t) {
    const float v = block_sum(s[t], s_r);
    if (tid == 0) part[(size_t)b * 10 * C + (t < 9 ? 9 * c + t : 9 * C + c)] = v;
  }
}

// ---- attention -----------------------------------------------------------------------------------------------------------------
// The scaled logits of a 16 x 16 tile, in float64 on v_mfma_f64_16x16x4_f64: the one product of this file that is not fp32.
// At logits of +-60 an ulp of a float32 logit is 3.8e-6, and every probability the backward forms again as exp(logit - lse)
// carries it: with fp32 logits (one chain, or a tree of four-channel chains) dK and dV lay at 1.3 to 1.5 x 16 * 2^-24 against
// float64.  The operands are the fp32 values widened (exact), so the products are exact and the sum is good to 2^-53; the
// running maximum and the log-sum-exp are kept in float64 too (the latter stored as two floats), and only the exponent's
// argument, logit - max or logit - lse, is rounded to fp32.  The f64 result layout differs from the f32 one (register r of
// lane (j, k): row k + 4 r), so the tile goes through LDS once and comes back as d[r] = row 4 k + r, column j, the f32
// layout the rest of each kernel uses.  The forward and both backward kernels form their logits here (a and b may swap).
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <int HD>
__device__ __forceinline__ void logit_tile(const float (&a)[HD / 4], const float (&b)[HD / 4], double (*s_t)[17], double scale, int j, int k,
                                           double (&d)[4]) {
  f64x4 acc = {0., 0., 0., 0.};
#pragma unroll
  for (int kk = 0; kk < HD / 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[kk], (double)b[kk], acc, 0, 0, 0);
  __syncthreads();      // the previous tile's reads are done
#pragma unroll
  for (int r = 0; r < 4; ++r) s_t[k + 4 * r][j] = acc[r];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) d[r] = s_t[4 * k + r][j] * scale;
}

// q, o, dO [N][C][S]: head h owns channels h HD ... ; kv [N][2 C][T]: keys in the first C channels, values in the second
template <int HD>
__global__ __launch_bounds__(64) void att_fwd_kernel(const float* __restrict__ q, const float* __restrict__ kv, float* __restrict__ o,
                                                     float* __restrict__ lse, int C, int S, int T, double scale) {
  __shared__ float s_p[16][17];
  __shared__ double s_t[16][17];
  const int lane = threadIdx.x, j = lane & 15, k = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
  const float* qb = q + ((size_t)b * C + h * HD) * S;
  const float* kb = kv + ((size_t)b * 2 * C + h * HD) * T;
  const float* vb = kb + (size_t)C * T;
  float qa[HD / 4];
#pragma unroll
  for (int kk = 0; kk < HD / 4; ++kk) qa[kk] = q0 + j < S ? qb[(size_t)(4 * kk + k) * S + q0 + j] : 0.f;
  double m[4];
  float l[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int t0 = 0; t0 < T; t0 += 16) {
    const bool key = t0 + j < T;
    float kt[HD / 4];
#pragma unroll
    for (int kk = 0; kk < HD / 4; ++kk) kt[kk] = key ? kb[(size_t)(4 * kk + k) * T + t0 + j] : 0.f;
    double s[4];
    logit_tile<HD>(qa, kt, s_t, scale, j, k, s);
    float p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {       // d[r] of lane (j, k): query q0 + 4 k + r, key t0 + j
      const double v = key ? s[r] : -INFINITY;
      double mx = v;
      for (int of = 8; of > 0; of >>= 1) mx = fmax(mx, __shfl_xor(mx, of));
      const double mn = fmax(m[r], mx);       // finite: a tile has at least one key
      const float f = expf((float)(m[r] - mn));
      p[r] = expf((float)(v - mn));
      float ps = p[r];
      for (int of = 8; of > 0; of >>= 1) ps += __shfl_xor(ps, of);
      l[r] = fmaf(l[r], f, ps);
      acc[r] *= f;
      m[r] = mn;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) s_p[4 * k + r][j] = p[r];
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int t = t0 + 4 * kk + k;
      acc = mfma4(s_p[j][4 * kk + k], (j < HD && t < T) ? vb[(size_t)j * T + t] : 0.f, acc);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {         // register r: query q0 + 4 k + r, channel j
    const int qi = q0 + 4 * k + r;
    if (qi >= S) continue;
    if (j < HD) o[((size_t)b * C + h * HD + j) * S + qi] = acc[r] / l[r];
    if (j == 0) {       // the log-sum-exp, and what its rounding dropped: near 60 an ulp is 4e-6, which the backward's P would carry
      const double ld = m[r] + (double)logf(l[r]);
      const float hi = (float)ld;
      lse[((size_t)b * HEADS + h) * S + qi] = hi;
      lse[(size_t)gridDim.z * HEADS * S + ((size_t)b * HEADS + h) * S + qi] = (float)(ld - (double)hi);
    }
  }
}

template <int HD>
__global__ __launch_bounds__(64) void att_delta_kernel(const float* __restrict__ o, const float* __restrict__ dO, float* __restrict__ delta, int C,
                                                       int S) {
  const int lane = threadIdx.x, j = lane & 15, k = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
  const size_t base = ((size_t)b * C + h * HD) * S;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < HD / 4; ++kk) {
    const bool live = q0 + j < S;
    const size_t at = base + (size_t)(4 * kk + k) * S + q0 + j;
    acc = mfma4(live ? dO[at] : 0.f, live ? o[at] : 0.f, acc);
  }
  // register r of lane (j, k): dO of query 4 k + r times O of query j; the diagonal is 4 k + r = j
  if ((j >> 2) == k && q0 + j < S) {
    const int r = j & 3;
    delta[((size_t)b * HEADS + h) * S + q0 + j] = r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
  }
}

template <int HD>
__global__ __launch_bounds__(64) void att_dq_kernel(const float* __restrict__ q, const float* __restrict__ kv, const float* __restrict__ lse,
                                                    const float* __restrict__ delta, const float* __restrict__ dO, float* __restrict__ dq, int C,
                                                    int S, int T, double scale) {
  __shared__ float s_p[16][17];
  __shared__ double s_t[16][17];
  const int lane = threadIdx.x, j = lane & 15, k = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
  const size_t qoff = ((size_t)b * C + h * HD) * S;
  const float* kb = kv + ((size_t)b * 2 * C + h * HD) * T;
  const float* vb = kb + (size_t)C * T;
  float qa[HD / 4], da[HD / 4];
#pragma unroll
  for (int kk = 0; kk < HD / 4; ++kk) {
    const bool live = q0 + j < S;
    const size_t at = qoff + (size_t)(4 * kk + k) * S + q0 + j;
    qa[kk] = live ? q[at] : 0.f;
    da[kk] = live ? dO[at] : 0.f;
  }
  float lr[4], lo[4], dr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qi = q0 + 4 * k + r;
    lr[r] = qi < S ? lse[((size_t)b * HEADS + h) * S + qi] : 0.f;
    lo[r] = qi < S ? lse[(size_t)gridDim.z * HEADS * S + ((size_t)b * HEADS + h) * S + qi] : 0.f;
    dr[r] = qi < S ? delta[((size_t)b * HEADS + h) * S + qi] : 0.f;
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int t0 = 0; t0 < T; t0 += 16) {
    const bool key = t0 + j < T;
    f32x4 dp = {0.f, 0.f, 0.f, 0.f};
    float kt[HD / 4];
#pragma unroll
    for (int kk = 0; kk < HD / 4; ++kk) {
      const size_t at = (size_t)(4 * kk + k) * T + t0 + j;
      kt[kk] = key ? kb[at] : 0.f;
      dp = mfma4(da[kk], key ? vb[at] : 0.f, dp);
    }
    double s[4];
    logit_tile<HD>(qa, kt, s_t, scale, j, k, s);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = key ? expf((float)((s[r] - (double)lr[r]) - (double)lo[r])) : 0.f;
      s_p[4 * k + r][j] = p * (dp[r] - dr[r]);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int t = t0 + 4 * kk + k;
      acc = mfma4(s_p[j][4 * kk + k], (j < HD && t < T) ? kb[(size_t)j * T + t] : 0.f, acc);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qi = q0 + 4 * k + r;
    if (qi < S && j < HD) dq[qoff + (size_t)j * S + qi] = acc[r] * (float)scale;
  }
}

template <int HD>
__global__ __launch_bounds__(64) void att_dkv_kernel(const float* __restrict__ q, const float* __restrict__ kv, const float* __restrict__ lse,
                                                     const float* __restrict__ delta, const float* __restrict__ dO, float* __restrict__ dkv, int C,
                                                     int S, int T, double scale) {
  __shared__ float s_p[16][17], s_d[16][17];
  __shared__ double s_t[16][17];
  const int lane = threadIdx.x, j = lane & 15, k = lane >> 4;
  const int t0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
  const float* qb = q + ((size_t)b * C + h * HD) * S;
  const float* db = dO + ((size_t)b * C + h * HD) * S;
  const size_t koff = ((size_t)b * 2 * C + h * HD) * T, voff = koff + (size_t)C * T;
  const float* lb = lse + ((size_t)b * HEADS + h) * S;
  const float* eb = delta + ((size_t)b * HEADS + h) * S;
  float ka[HD / 4], va[HD / 4];
#pragma unroll
  for (int kk = 0; kk < HD / 4; ++kk) {
    const bool live = t0 + j < T;
    ka[kk] = live ? kv[koff + (size_t)(4 * kk + k) * T + t0 + j] : 0.f;
    va[kk] = live ? kv[voff + (size_t)(4 * kk + k) * T + t0 + j] : 0.f;
  }
  f32x4 dk = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < S; q0 += 16) {
    const bool qry = q0 + j < S;
    f32x4 dpt = {0.f, 0.f, 0.f, 0.f};
    float qt[HD / 4];
#pragma unroll
    for (int kk = 0; kk < HD / 4; ++kk) {
      const size_t at = (size_t)(4 * kk + k) * S + q0 + j;
      qt[kk] = qry ? qb[at] : 0.f;
      dpt = mfma4(va[kk], qry ? db[at] : 0.f, dpt);
    }
    double st[4];
    logit_tile<HD>(ka, qt, s_t, scale, j, k, st);
    const float lq = qry ? lb[q0 + j] : 0.f, lo = qry ? lb[(size_t)gridDim.z * HEADS * S + q0 + j] : 0.f, dl = qry ? eb[q0 + j] : 0.f;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {       // register r of lane (j, k): key t0 + 4 k + r, query q0 + j
      const float p = qry ? expf((float)((st[r] - (double)lq) - (double)lo)) : 0.f;
      s_p[4 * k + r][j] = p;
      s_d[4 * k + r][j] = p * (dpt[r] - dl);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int qi = q0 + 4 * kk + k;
      const bool live = j < HD && qi < S;
      dv = mfma4(s_p[j][4 * kk + k], live ? db[(size_t)j * S + qi] : 0.f, dv);
      dk = mfma4(s_d[j][4 * kk + k], live ? qb[(size_t)j * S + qi] : 0.f, dk);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int t = t0 + 4 * k + r;
    if (t < T && j < HD) {
      dkv[koff + (size_t)j * T + t] = dk[r] * (float)scale;
      dkv[voff + (size_t)j * T + t] = dv[r];
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
bool ch_ok(int c) { return c == 48 || c == 64 || c == 96 || c == 128; }

const char* shape_problem(int N, int H, int W, int Cin, int Cout, int* code) {
  *code = KP2D_ERR_ARG;
  if (N < 1 || N > 65535) return "N outside [1, 65535]";
  if (H < 1 || W < 1) return "H and W must be at least 1";
  if (Cin < 1 || Cout < 1) return "channel counts must be at least 1";
  *code = KP2D_ERR_UNSUPPORTED;
  if (!ch_ok(Cin) || !ch_ok(Cout)) return "channel counts must be 48, 64, 96 or 128";
  if ((long long)H * W > MAX_HW) return "H * W above 2^24";
  return nullptr;
}

struct SlabGeo {
  long long total, pps;
  int slabs;
};

SlabGeo slab_geo(int N, long long P) {
  SlabGeo g{};
  g.total = (long long)N * P;
  g.pps = ((g.total + MAX_SLABS - 1) / MAX_SLABS + 3) / 4 * 4;
  if (g.pps < MIN_SLAB) g.pps = MIN_SLAB;
  g.slabs = (int)((g.total + g.pps - 1) / g.pps);
  return g;
}

struct Plan {
  float *part, *chan, *delta;
  size_t total;
};

// one layout for every call of the family: the weight-gradient partials (the 2 x 2 patches' 4 Cin columns at most), the
// per-frame channel sums (10 per channel at most) and the attention backward's delta
Plan plan_of(void* scratch, int N, int H, int W, int Cin, int Cout) {
  Plan p{};
  Carve c(scratch);
  const long long px = (long long)N * H * W;
  const long long slabs = (px + MIN_SLAB - 1) / MIN_SLAB < MAX_SLABS ? (px + MIN_SLAB - 1) / MIN_SLAB : MAX_SLABS;
  p.part = c.take<float>((size_t)slabs * Cout * Cin * 4);
  p.chan = c.take<float>((size_t)N * 10 * (Cin > Cout ? Cin : Cout));
  p.delta = c.take<float>((size_t)N * HEADS * H * W);
  p.total = c.bytes();
  return p;
}

#define ATT_PROLOGUE(who, N, H, W, Cin, Cout)                                                                                       \
  int code;                                                                                                                         \
  if (const char* why = shape_problem(N, H, W, Cin, Cout, &code))                                                                   \
    return fail(code, who ": %s (N %d, H %d, W %d, channels %d, %d)", why, N, H, W, Cin, Cout)

#define ATT_SCRATCH(who, N, H, W, Cin, Cout)                                                                                        \
  if (!scratch || misaligned(scratch, 16)) return fail(KP2D_ERR_ARG, who ": scratch must be 16-byte aligned and not null");         \
  const Plan plan = plan_of(scratch, N, H, W, Cin, Cout);                                                                           \
  if (scratch_bytes < plan.total)                                                                                                   \
    return fail(KP2D_ERR_ARG, who " scratch %zu B < required %zu B (kp2d_att_train_scratch_bytes)", scratch_bytes, plan.total)

// dbias [C] from dy [N][C][HW] through chan [N][C]
int channel_sums(const float* dy, float* chan, float* out, int N, int C, size_t HW, hipStream_t st) {
  hipLaunchKernelGGL(lnsum_plane_kernel, dim3(C, N), dim3(256), 0, st, dy, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                     chan, C, HW);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(strided_sum_kernel, dim3(blocks_of(C)), dim3(256), 0, st, chan, (size_t)C, N, out, C);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

template <int MODE>
int weight_gradient(const DwA& d0, const SlabGeo& g, float* dw, hipStream_t st) {
  DwA d = d0;
  d.total = g.total; d.pps = g.pps;
  hipLaunchKernelGGL(pw_dw_kernel<MODE>, dim3(g.slabs, d.K / 16), dim3(256), 0, st, d);
  HIP_TRY(hipGetLastError());
  const int nw = d.M * d.K;
  hipLaunchKernelGGL(strided_sum_kernel, dim3(blocks_of(nw)), dim3(256), 0, st, d.part, (size_t)nw, g.slabs, dw, nw);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

}  // namespace

extern "C" {

size_t kp2d_att_train_scratch_bytes(int N, int H, int W, int Cin, int Cout) {
  int code;
  if (shape_problem(N, H, W, Cin, Cout, &code)) return 0;
  return plan_of(nullptr, N, H, W, Cin, Cout).total;
}

int kp2d_layernorm_forward_train(const float* x, const float* g, const float* b, int N, int C, int H, int W, double eps, float* y,
                                 float* mean, float* rinv, void* stream) {
  ATT_PROLOGUE("layernorm_forward_train", N, H, W, C, C);
  if (!(eps >= 0.0 && eps < INFINITY)) return fail(KP2D_ERR_ARG, "layernorm_forward_train: eps %g must be finite and not negative", eps);
  if (any_null(x, g, b, y, mean, rinv)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, g, b, y, mean, rinv)) return fail(KP2D_ERR_ARG, "layernorm_forward_train: float arrays must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  const long long HW = (long long)H * W, total = N * HW;
  hipLaunchKernelGGL(ln_forward_kernel, dim3(blocks_of(total)), dim3(256), 0, st, x, g, b, (float)eps, C, HW, total, y, mean, rinv);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_layernorm_backward(const float* x, const float* g, const float* mean, const float* rinv, const float* dy, int N, int C, int H,
                            int W, double eps, float* dx, float* dg, float* db, void* scratch, size_t scratch_bytes, void* stream) {
  ATT_PROLOGUE("layernorm_backward", N, H, W, C, C);
  if (!(eps >= 0.0 && eps < INFINITY)) return fail(KP2D_ERR_ARG, "layernorm_backward: eps %g must be finite and not negative", eps);
  if (any_null(x, g, mean, rinv, dy, dx, dg, db)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, g, mean, rinv, dy, dx, dg, db)) return fail(KP2D_ERR_ARG, "layernorm_backward: float arrays must be 4-byte aligned");
  ATT_SCRATCH("layernorm_backward", N, H, W, C, C);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  const long long HW = (long long)H * W, total = N * HW;
  hipLaunchKernelGGL(ln_backward_kernel, dim3(blocks_of(total)), dim3(256), 0, st, x, g, mean, dy, (float)eps, C, HW, total, dx);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(lnsum_plane_kernel, dim3(C, N), dim3(256), 0, st, dy, x, mean, rinv, plan.chan, C, (size_t)HW);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(strided_sum_kernel, dim3(blocks_of(C)), dim3(256), 0, st, plan.chan, (size_t)2 * C, N, dg, C);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(strided_sum_kernel, dim3(blocks_of(C)), dim3(256), 0, st, plan.chan + C, (size_t)2 * C, N, db, C);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_pointwise_forward_train(const float* x, const float* w, const float* bias, int N, int H, int W, int Cin, int Cout, int gelu,
                                 float* y, float* pre, void* stream) {
  ATT_PROLOGUE("pointwise_forward_train", N, H, W, Cin, Cout);
  if (any_null(x, w, y) || (gelu && !pre)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, w, bias, y, pre)) return fail(KP2D_ERR_ARG, "pointwise_forward_train: float arrays must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  PwA a{};
  a.x = x; a.w = w; a.bias = bias; a.y = y; a.pre = pre; a.M = Cout; a.K = Cin; a.a_rs = Cin; a.a_ks = 1; a.P = H * W; a.gelu = gelu ? 1 : 0;
  hipLaunchKernelGGL(pw_kernel<0>, dim3((a.P + 63) / 64, N), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_gelu_backward(const float* pre, const float* dy, int64_t n, float* dpre, void* stream) {
  if (n < 1 || n > ((int64_t)1 << 38)) return fail(KP2D_ERR_ARG, "gelu_backward: n %lld outside [1, 2^38]", (long long)n);
  if (any_null(pre, dy, dpre)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(pre, dy, dpre)) return fail(KP2D_ERR_ARG, "gelu_backward: float arrays must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(pre, st);
  hipLaunchKernelGGL(gelu_backward_kernel, dim3(blocks_of(n)), dim3(256), 0, st, pre, dy, dpre, (long long)n);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_pointwise_backward(const float* x, const float* w, const float* dy, int N, int H, int W, int Cin, int Cout, float* dx,
                            float* d_weight, float* d_bias, void* scratch, size_t scratch_bytes, void* stream) {
  ATT_PROLOGUE("pointwise_backward", N, H, W, Cin, Cout);
  if (any_null(x, w, dy, d_weight)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, w, dy, dx, d_weight, d_bias)) return fail(KP2D_ERR_ARG, "pointwise_backward: float arrays must be 4-byte aligned");
  ATT_SCRATCH("pointwise_backward", N, H, W, Cin, Cout);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  const int P = H * W;
  DwA d{};
  d.dy = dy; d.x = x; d.part = plan.part; d.M = Cout; d.K = Cin; d.P = P;
  if (int rc = weight_gradient<0>(d, slab_geo(N, P), d_weight, st)) return rc;
  if (d_bias)
    if (int rc = channel_sums(dy, plan.chan, d_bias, N, Cout, (size_t)P, st)) return rc;
  if (dx) {       // dx[ci][p] = sum_co w[co][ci] dy[co][p]
    PwA a{};
    a.x = dy; a.w = w; a.y = dx; a.M = Cin; a.K = Cout; a.a_rs = 1; a.a_ks = Cin; a.P = P;
    hipLaunchKernelGGL(pw_kernel<0>, dim3((P + 63) / 64, N), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  return KP2D_OK;
}

int kp2d_patch2_forward_train(const float* x, const float* w, int N, int C, int H, int W, float* y, void* stream) {
  ATT_PROLOGUE("patch2_forward_train", N, H, W, C, C);
  if (C > 64) return fail(KP2D_ERR_UNSUPPORTED, "patch2_forward_train: C %d must be 48 or 64 (the result has 2 C channels)", C);
  if (H < 2 || W < 2) return fail(KP2D_ERR_ARG, "patch2_forward_train: H %d and W %d must be at least 2", H, W);
  if (any_null(x, w, y)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, w, y)) return fail(KP2D_ERR_ARG, "patch2_forward_train: float arrays must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  PwA a{};
  a.x = x; a.w = w; a.y = y; a.M = 2 * C; a.K = 4 * C; a.a_rs = 4 * C; a.a_ks = 1; a.C = C; a.H = H; a.W = W; a.Wo = W / 2;
  a.P = (H / 2) * (W / 2);
  hipLaunchKernelGGL(pw_kernel<1>, dim3((a.P + 63) / 64, N), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_patch2_backward(const float* x, const float* w, const float* dy, int N, int C, int H, int W, float* dx, float* d_weight,
                         void* scratch, size_t scratch_bytes, void* stream) {
  ATT_PROLOGUE("patch2_backward", N, H, W, C, C);
  if (C > 64) return fail(KP2D_ERR_UNSUPPORTED, "patch2_backward: C %d must be 48 or 64 (dy has 2 C channels)", C);
  if (H < 2 || W < 2) return fail(KP2D_ERR_ARG, "patch2_backward: H %d and W %d must be at least 2", H, W);
  if (any_null(x, w, dy, d_weight)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, w, dy, dx, d_weight)) return fail(KP2D_ERR_ARG, "patch2_backward: float arrays must be 4-byte aligned");
  ATT_SCRATCH("patch2_backward", N, H, W, C, 2 * C);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  const int P = (H / 2) * (W / 2);
  DwA d{};
  d.dy = dy; d.x = x; d.part = plan.part; d.M = 2 * C; d.K = 4 * C; d.C = C; d.H = H; d.W = W; d.Wo = W / 2; d.P = P;
  if (int rc = weight_gradient<1>(d, slab_geo(N, P), d_weight, st)) return rc;
  if (dx) {       // dx[ci][2 i + a][2 j + b] = sum_co w[co][4 ci + 2 a + b] dy[co][i][j]
    PwA a{};
    a.x = dy; a.w = w; a.y = dx; a.M = 4 * C; a.K = 2 * C; a.a_rs = 1; a.a_ks = 4 * C; a.C = C; a.H = H; a.W = W; a.Wo = W / 2; a.P = P;
    hipLaunchKernelGGL(pw_kernel<2>, dim3((P + 63) / 64, N), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    if ((H | W) & 1) {
      const long long planes = (long long)N * C;
      hipLaunchKernelGGL(patch_rim_kernel, dim3(blocks_of(planes * H * W)), dim3(256), 0, st, dx, planes, H, W);
      HIP_TRY(hipGetLastError());
    }
  }
  return KP2D_OK;
}

int kp2d_dwconv3_forward_train(const float* x, const float* w, const float* bias, int N, int C, int H, int W, float* y, void* stream) {
  ATT_PROLOGUE("dwconv3_forward_train", N, H, W, C, C);
  if (any_null(x, w, bias, y)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, w, bias, y)) return fail(KP2D_ERR_ARG, "dwconv3_forward_train: float arrays must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  const long long total = (long long)N * C * H * W;
  hipLaunchKernelGGL(dwc_forward_kernel, dim3(blocks_of(total)), dim3(256), 0, st, x, w, bias, y, total, C, H, W);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_dwconv3_backward(const float* x, const float* w, const float* dy, int N, int C, int H, int W, float* dx, float* d_weight,
                          float* d_bias, void* scratch, size_t scratch_bytes, void* stream) {
  ATT_PROLOGUE("dwconv3_backward", N, H, W, C, C);
  if (any_null(x, w, dy, d_weight, d_bias)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, w, dy, dx, d_weight, d_bias)) return fail(KP2D_ERR_ARG, "dwconv3_backward: float arrays must be 4-byte aligned");
  ATT_SCRATCH("dwconv3_backward", N, H, W, C, C);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  hipLaunchKernelGGL(dwc_dw_plane_kernel, dim3(C, N), dim3(256), 0, st, x, dy, plan.chan, C, H, W);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(strided_sum_kernel, dim3(blocks_of(9 * C)), dim3(256), 0, st, plan.chan, (size_t)10 * C, N, d_weight, 9 * C);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(strided_sum_kernel, dim3(blocks_of(C)), dim3(256), 0, st, plan.chan + 9 * C, (size_t)10 * C, N, d_bias, C);
  HIP_TRY(hipGetLastError());
  if (dx) {
    const long long total = (long long)N * C * H * W;
    hipLaunchKernelGGL(dwc_dx_kernel, dim3(blocks_of(total)), dim3(256), 0, st, dy, w, dx, total, C, H, W);
    HIP_TRY(hipGetLastError());
  }
  return KP2D_OK;
}

static const char* attention_problem(int N, int C, int H, int W, int* code) {
  if (const char* why = shape_problem(N, H, W, C, C, code)) return why;
  *code = KP2D_ERR_ARG;
  if (H < 2 || W < 2) return "H and W must be at least 2 (one 2 x 2 key patch)";
  *code = KP2D_ERR_UNSUPPORTED;
  if (C > 64) return "C must be 48 or 64 (head dimension 12 or 16)";
  return nullptr;
}

int kp2d_attention_forward_train(const float* q, const float* kv, int N, int C, int H, int W, float* o, float* lse, void* stream) {
  int code;
  if (const char* why = attention_problem(N, C, H, W, &code)) return fail(code, "attention_forward_train: %s (N %d, C %d, H %d, W %d)", why, N, C, H, W);
  if (any_null(q, kv, o, lse)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(q, kv, o, lse)) return fail(KP2D_ERR_ARG, "attention_forward_train: float arrays must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(q, st);
  const int S = H * W, T = (H / 2) * (W / 2), hd = C / HEADS;
  const double scale = 1.0 / sqrt((double)hd);
  const dim3 grid((S + 15) / 16, HEADS, N);
  if (hd == 16) hipLaunchKernelGGL(att_fwd_kernel<16>, grid, dim3(64), 0, st, q, kv, o, lse, C, S, T, scale);
  else hipLaunchKernelGGL(att_fwd_kernel<12>, grid, dim3(64), 0, st, q, kv, o, lse, C, S, T, scale);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_attention_backward(const float* q, const float* kv, const float* o, const float* lse, const float* d_o, int N, int C, int H, int W,
                            float* dq, float* dkv, void* scratch, size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = attention_problem(N, C, H, W, &code)) return fail(code, "attention_backward: %s (N %d, C %d, H %d, W %d)", why, N, C, H, W);
  if (any_null(q, kv, o, lse, d_o, dq, dkv)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(q, kv, o, lse, d_o, dq, dkv)) return fail(KP2D_ERR_ARG, "attention_backward: float arrays must be 4-byte aligned");
  ATT_SCRATCH("attention_backward", N, H, W, C, C);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(q, st);
  const int S = H * W, T = (H / 2) * (W / 2), hd = C / HEADS;
  const double scale = 1.0 / sqrt((double)hd);
  const dim3 qgrid((S + 15) / 16, HEADS, N), kgrid((T + 15) / 16, HEADS, N);
  if (hd == 16) {
    hipLaunchKernelGGL(att_delta_kernel<16>, qgrid, dim3(64), 0, st, o, d_o, plan.delta, C, S);
    hipLaunchKernelGGL(att_dq_kernel<16>, qgrid, dim3(64), 0, st, q, kv, lse, plan.delta, d_o, dq, C, S, T, scale);
    hipLaunchKernelGGL(att_dkv_kernel<16>, kgrid, dim3(64), 0, st, q, kv, lse, plan.delta, d_o, dkv, C, S, T, scale);
  } else {
    hipLaunchKernelGGL(att_delta_kernel<12>, qgrid, dim3(64), 0, st, o, d_o, plan.delta, C, S);
    hipLaunchKernelGGL(att_dq_kernel<12>, qgrid, dim3(64), 0, st, q, kv, lse, plan.delta, d_o, dq, C, S, T, scale);
    hipLaunchKernelGGL(att_dkv_kernel<12>, kgrid, dim3(64), 0, st, q, kv, lse, plan.delta, d_o, dkv, C, S, T, scale);
  }
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

}  // extern "C"
