// Fine-tuning of the depth head on the device (include/kp2d.h): the loss of the reference's _compute_depth_loss
// (KeypointNetwithIOLoss.py:907-916), SILog (utils/losses.py:176-192) + Huber, taken from the logits before the sigmoid,
// with its gradient.  The head itself is the nine-layer stack of seg_train.hip / vpr_head_train.hip with one output channel.
//
//   kp2d_depth_loss     silog_weight SILog + huber_weight Huber over the valid pixels (gt finite and > 0, logit finite), two passes:
//     dl_sums_kernel    grid (runs <= 1024): a run walks a fixed stretch of 1024-pixel chunks; per chunk a thread forms g and
//                       the Huber term of its four pixels in fp32; the chunk's count and sum of g, then its sum of
//                       (g - chunk mean)^2 are float64 butterflies over the wave and the four waves in wave order; thread 0
//                       merges (count, mean, M2) into the run's by Chan's formula, chunk after chunk
//     dl_merge_kernel   one thread: the runs' (count, mean, M2) by Chan's formula in run order, the Huber sums in run order
//                       -> loss, parts, valid, stray and the four coefficients of the gradient
//     dl_grad_kernel    a thread per pixel (strided above 2^28 pixels): g and p again, dlogits; nothing of size [N, HW] is kept between the passes
// The variance is never formed from raw moments.  No float atomics; every cut depends on the shapes alone: bit-identical from
// run to run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "api_common.h"
#include "device_guard.h"
#include "train_common.h"

using namespace kp2d;

namespace {

constexpr int LP = 1024;            // pixels of a chunk: four per thread
constexpr int MAX_RUNS = 1024;
constexpr long long MAX_GRAD_BLOCKS = 1 << 20;      // pass 2 strides over the pixels beyond 2^28
constexpr float HUBER_DELTA = (float)KP2D_HUBER_DELTA;

struct DepthGeo {
  long long total, chunks, cpr;     // pixels, chunks, chunks per run
  int runs;
};

DepthGeo depth_geo(int N, int64_t HW) {
  DepthGeo g{};
  g.total = (long long)N * HW;
  g.chunks = (g.total + LP - 1) / LP;
  g.cpr = (g.chunks + MAX_RUNS - 1) / MAX_RUNS;
  g.runs = (int)((g.chunks + g.cpr - 1) / g.cpr);
  return g;
}

struct DepthPlan {
  long long* cnt;     // [runs][2]: valid, stray
  double* part;       // [runs][3]: mean of g, M2 of g, the Huber sum
  double* coef;       // [4]: mean; a, b of dSILog / dg = a (g - mean) + b (times silog_weight); huber_weight / M
  size_t total;
};

DepthPlan depth_plan(void* scratch, int N, int64_t HW) {
  DepthPlan p{};
  Carve c(scratch);
  const DepthGeo g = depth_geo(N, HW);
  p.cnt = c.take<long long>((size_t)g.runs * 2);
  p.part = c.take<double>((size_t)g.runs * 3);
  p.coef = c.take<double>(4);
  p.total = c.bytes();
  return p;
}

// 1: valid; 0: ignored (gt <= 0); -1: stray (gt or the logit is not finite)
__device__ __forceinline__ int pixel_kind(float z, float gt) {
  if (!isfinite(z) || !isfinite(gt)) return -1;
  return gt > 0.f ? 1 : 0;
}

// a valid pixel: g = log sigmoid(z) - log gt = -softplus(-z) - log gt, p = sigmoid(z), q = 1 - p; all finite for finite z
__device__ __forceinline__ void pixel_terms(float z, float gt, float* g, float* p, float* q) {
  const float e = expf(-fabsf(z));
  const float r = 1.f / (1.f + e);
  *p = z >= 0.f ? r : e * r;
  *q = z >= 0.f ? e * r : r;
  *g = -(fmaxf(-z, 0.f) + log1pf(e)) - logf(gt);
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// (n, mean, M2) <- (n, mean, M2) + (nb, mb, M2b), Chan et al.
__device__ __forceinline__ void chan_merge(long long* n, double* mean, double* m2, long long nb, double mb, double m2b) {
  if (nb == 0) return;
  if (*n == 0) { *n = nb; *mean = mb; *m2 = m2b; return; }
  const long long nt = *n + nb;
  const double delta = mb - *mean;
  *m2 += m2b + delta * delta * ((double)*n * (double)nb / (double)nt);
  *mean += delta * ((double)nb / (double)nt);
  *n = nt;
}

__global__ __launch_bounds__(256) void dl_sums_kernel(const float* __restrict__ z, const float* __restrict__ gt, DepthGeo geo,
                                                      double* __restrict__ part, long long* __restrict__ cnt) {
  __shared__ double s_sum[4], s_m2[4], s_h[4];
  __shared__ int s_n[4], s_stray[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double huber = 0.0;
  int stray = 0;
  long long run_n = 0;              // thread 0's: the run so far
  double run_mean = 0.0, run_m2 = 0.0;
  const long long q_end = ((long long)blockIdx.x + 1) * geo.cpr < geo.chunks ? ((long long)blockIdx.x + 1) * geo.cpr : geo.chunks;
  for (long long q = (long long)blockIdx.x * geo.cpr; q < q_end; ++q) {
    float g[LP / 256];
    bool ok[LP / 256];
    int n = 0;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < LP / 256; ++i) {
      const long long gp = q * LP + tid + 256 * i;
      g[i] = 0.f;
      ok[i] = false;
      if (gp < geo.total) {
        const float zi = z[gp], ti = gt[gp];
        const int kind = pixel_kind(zi, ti);
        if (kind < 0) ++stray;
        if (kind > 0) {
          float p, qq;
          pixel_terms(zi, ti, &g[i], &p, &qq);
          const float d = p - ti, ad = fabsf(d);
          huber += (double)(ad < HUBER_DELTA ? 0.5f * d * d : HUBER_DELTA * (ad - 0.5f * HUBER_DELTA));
          ok[i] = true;
          ++n;
          s += (double)g[i];
        }
      }
    }
    s = wave_sum(s);
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    __syncthreads();              // the previous chunk's sums have been read
    if (lane == 0) { s_sum[wave] = s; s_n[wave] = n; }
    __syncthreads();
    const int cn = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
    const double cmean = cn > 0 ? ((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3])) / (double)cn : 0.0;
    double m2 = 0.0;
#pragma unroll
    for (int i = 0; i < LP / 256; ++i) {
      const double dd = (double)g[i] - cmean;
      if (ok[i]) m2 += dd * dd;
    }
    m2 = wave_sum(m2);
    if (lane == 0) s_m2[wave] = m2;
    __syncthreads();
    if (tid == 0) chan_merge(&run_n, &run_mean, &run_m2, (long long)cn, cmean, (s_m2[0] + s_m2[1]) + (s_m2[2] + s_m2[3]));
  }
  huber = wave_sum(huber);
  for (int o = 32; o > 0; o >>= 1) stray += __shfl_xor(stray, o);
  __syncthreads();
  if (lane == 0) { s_h[wave] = huber; s_stray[wave] = stray; }
  __syncthreads();
  if (tid == 0) {
    part[(size_t)blockIdx.x * 3] = run_mean;
    part[(size_t)blockIdx.x * 3 + 1] = run_m2;
    part[(size_t)blockIdx.x * 3 + 2] = (s_h[0] + s_h[1]) + (s_h[2] + s_h[3]);
    cnt[(size_t)blockIdx.x * 2] = run_n;
    cnt[(size_t)blockIdx.x * 2 + 1] = (long long)s_stray[0] + s_stray[1] + s_stray[2] + s_stray[3];
  }
}

__global__ __launch_bounds__(64) void dl_merge_kernel(const double* __restrict__ part, const long long* __restrict__ cnt, int runs,
                                                      double ws, double wh, double* __restrict__ coef, float* __restrict__ loss,
                                                      float* __restrict__ parts, long long* __restrict__ valid_out,
                                                      long long* __restrict__ stray_out) {
  if (threadIdx.x != 0) return;
  long long M = 0, stray = 0;
  double mean = 0.0, m2 = 0.0, H = 0.0;
  for (int r = 0; r < runs; ++r) {
    chan_merge(&M, &mean, &m2, cnt[(size_t)r * 2], part[(size_t)r * 3], part[(size_t)r * 3 + 1]);
    H += part[(size_t)r * 3 + 2];
    stray += cnt[(size_t)r * 2 + 1];
  }
  const double Dg = M >= 2 ? m2 / (double)(M - 1) + KP2D_SILOG_LAMBDA * mean * mean : 0.0;
  const bool on = M >= 2 && Dg > 0.0;
  const double root = on ? sqrt(Dg) : 0.0;
  const double silog = KP2D_SILOG_SCALE * root, huber = M > 0 ? H / (double)M : 0.0;
  const double k = on ? ws * (0.5 * KP2D_SILOG_SCALE) / root : 0.0;      // d (10 sqrt(Dg)) / d Dg = 5 / sqrt(Dg)
  coef[0] = mean;
  coef[1] = on ? k * 2.0 / (double)(M - 1) : 0.0;
  coef[2] = on ? k * 2.0 * KP2D_SILOG_LAMBDA * mean / (double)M : 0.0;
  coef[3] = M > 0 ? wh / (double)M : 0.0;
  *loss = (float)(ws * silog + wh * huber);
  parts[0] = (float)silog;
  parts[1] = (float)huber;
  *valid_out = M;
  *stray_out = stray;
}

// dz = (a (g - mean) + b) (1 - p) + (huber_weight / M) clip(p - gt) p (1 - p) at a valid pixel, 0 elsewhere
__global__ __launch_bounds__(256) void dl_grad_kernel(const float* __restrict__ z, const float* __restrict__ gt, long long total,
                                                      const double* __restrict__ coef, float* __restrict__ dz) {
  const double mean = coef[0];
  const float a = (float)coef[1], b = (float)coef[2], h = (float)coef[3];
  for (long long gp = (long long)blockIdx.x * 256 + threadIdx.x; gp < total; gp += (long long)gridDim.x * 256) {
    const float zi = z[gp], ti = gt[gp];
    float out = 0.f;
    if (pixel_kind(zi, ti) > 0) {
      float g, p, q;
      pixel_terms(zi, ti, &g, &p, &q);
      const float dev = (float)((double)g - mean);
      const float d = p - ti;
      const float clip = fabsf(d) < HUBER_DELTA ? d : copysignf(HUBER_DELTA, d);
      out = fmaf(a, dev, b) * q + h * clip * (p * q);
    }
    dz[gp] = out;
  }
}

const char* depth_shape_problem(int N, int64_t HW, int* code) {
  *code = KP2D_ERR_ARG;
  if (N < 1 || N > 65535) return "N outside [1, 65535]";
  if (HW < 1) return "H * W must be at least 1";
  *code = KP2D_ERR_UNSUPPORTED;
  if (HW > ((int64_t)1 << 30)) return "H * W above 2^30";
  return nullptr;
}

}  // namespace

extern "C" {

size_t kp2d_depth_loss_scratch_bytes(int N, int64_t HW) {
  int code;
  if (depth_shape_problem(N, HW, &code)) return 0;
  return depth_plan(nullptr, N, HW).total;
}

int kp2d_depth_loss(const float* logits, const float* gt, int N, int64_t HW, double silog_weight, double huber_weight, float* loss,
                    float* parts, float* dlogits, int64_t* valid, int64_t* stray, void* scratch, size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = depth_shape_problem(N, HW, &code)) return fail(code, "depth_loss: %s (N %d, HW %lld)", why, N, (long long)HW);
  if (!(silog_weight >= 0.0 && silog_weight < INFINITY && huber_weight >= 0.0 && huber_weight < INFINITY))
    return fail(KP2D_ERR_ARG, "depth_loss: weights %g, %g must be finite and not negative", silog_weight, huber_weight);
  if (any_null(logits, gt, loss, parts, dlogits, valid, stray, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(logits, gt, loss, parts, dlogits) || misaligned(valid, 8) || misaligned(stray, 8) || misaligned(scratch, 16))
    return fail(KP2D_ERR_ARG, "depth_loss: misaligned argument");
  const DepthPlan p = depth_plan(scratch, N, HW);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_ARG, "depth_loss scratch %zu B < required %zu B (kp2d_depth_loss_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(logits, st);
  const DepthGeo g = depth_geo(N, HW);
  hipLaunchKernelGGL(dl_sums_kernel, dim3(g.runs), dim3(256), 0, st, logits, gt, g, p.part, p.cnt);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(dl_merge_kernel, dim3(1), dim3(64), 0, st, p.part, p.cnt, g.runs, silog_weight, huber_weight, p.coef, loss, parts,
                     (long long*)valid, (long long*)stray);
  HIP_TRY(hipGetLastError());
  const long long need = (g.total + 255) / 256, grad_blocks = need < MAX_GRAD_BLOCKS ? need : MAX_GRAD_BLOCKS;
  hipLaunchKernelGGL(dl_grad_kernel, dim3((unsigned)grad_blocks), dim3(256), 0, st, logits, gt, g.total, p.coef, dlogits);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

}  // extern "C"
