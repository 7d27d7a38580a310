// Scores of the two dense heads on the device (kp2d_seg_stats, kp2d_depth_sums: include/kp2d.h): the counts behind
// segmentation_models_pytorch's metrics and the sums behind the reference's nine depth metrics
// (src/evaluation/segmentation.py:42-57, src/evaluation/depth_estimation.py:58-83), so that a class map or a depth map never
// has to leave HBM to be scored.  Stateless like vpr.hip and kmeans.hip; plain vector code, integer atomics only.
//   seg_count_kernel    one workgroup per (image, chunk of SEG_CHUNK pixels): three class histograms in LDS (target,
//                       prediction, matched) filled with integer LDS atomics, flushed with one integer global add per
//                       non-zero bin: tp = matched, fp = prediction - matched, fn = target - matched.  The confusion
//                       matrix takes one of two forms: a C x C tile in LDS next to the histograms (C <= SEG_CONF_LDS_MAX,
//                       flushed the same way), or one integer global add per pixel (larger C: the tile no longer fits).
//   seg_tn_kernel       tn = (n - ignored - stray) - tp - fp - fn for every (image, class)
//   depth_part_kernel   one workgroup per (image, chunk of DEPTH_CHUNK pixels): thread t widens pixels t, t + 256, ... of the
//                       chunk to double and adds its terms in that order; lanes, then waves, are combined by a fixed tree
//                       -> one partial row per chunk
//   depth_final_kernel  one workgroup per image: thread t adds partial rows t, t + 256, ... in order, then the same tree
// Integer sums do not depend on their order; the double sums are formed in an order that n alone decides (no float
// atomics), and an image's rows never meet another image's: bit-identical from run to run and alone or inside a batch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "api_common.h"
#include "device_guard.h"

using namespace kp2d;

namespace {

constexpr int WG = 256;                     // threads of every kernel here
constexpr int SEG_CHUNK = 4096;             // pixels per workgroup of seg_count_kernel
constexpr int SEG_MAX_C = 1024;
constexpr int SEG_CONF_MAX_C = 256;
constexpr int SEG_CONF_LDS_MAX = 96;        // 96 * 96 + 3 * 96 ints = 38 016 B of LDS: four workgroups per compute unit
constexpr int DEPTH_CHUNK = 4096;           // pixels per workgroup of depth_part_kernel: 16 per thread
constexpr int NS = KP2D_DEPTH_NSUMS;
constexpr int MAX_B = 65535;                // images ride on gridDim.y

typedef unsigned long long u64;

enum { CONF_NONE = 0, CONF_LDS = 1, CONF_GLOBAL = 2 };

template <typename T, int MODE>
__global__ __launch_bounds__(WG) void seg_count_kernel(const int64_t* __restrict__ pred, const T* __restrict__ target, int64_t n,
                                                       int C, int64_t ignore, u64* __restrict__ stats, u64* __restrict__ conf,
                                                       u64* __restrict__ ignored, u64* __restrict__ stray) {
  extern __shared__ int lds[];               // hT [C], hP [C], hM [C], then the C x C tile (CONF_LDS)
  __shared__ int s_misc[2];                  // ignored, stray of this chunk
  int* hT = lds;
  int* hP = lds + C;
  int* hM = lds + 2 * C;
  int* tile = lds + 3 * C;
  const int t = threadIdx.x, b = blockIdx.y;
  const int cells = 3 * C + (MODE == CONF_LDS ? C * C : 0);
  for (int i = t; i < cells; i += WG) lds[i] = 0;
  if (t < 2) s_misc[t] = 0;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * SEG_CHUNK, i1 = min(n, i0 + SEG_CHUNK);
  const int64_t* prow = pred + (size_t)b * n;
  const T* trow = target + (size_t)b * n;
  u64* crow = MODE == CONF_NONE ? nullptr : conf + (size_t)b * C * C;
  int n_ign = 0, n_stray = 0;
  for (int64_t i = i0 + t; i < i1; i += WG) {
    const int64_t g = (int64_t)trow[i], p = prow[i];
    if (ignore != KP2D_SEG_NO_IGNORE && g == ignore) {
      ++n_ign;
    } else if (g < 0 || g >= C || p < 0 || p >= C) {
      ++n_stray;
    } else {
      atomicAdd(hT + (int)g, 1);
      atomicAdd(hP + (int)p, 1);
      if (g == p) atomicAdd(hM + (int)g, 1);
      if (MODE == CONF_LDS) atomicAdd(tile + (int)g * C + (int)p, 1);
      if (MODE == CONF_GLOBAL) atomicAdd(crow + (size_t)g * C + (size_t)p, (u64)1);
    }
  }
  if (n_ign) atomicAdd(s_misc + 0, n_ign);
  if (n_stray) atomicAdd(s_misc + 1, n_stray);
  __syncthreads();
  u64* srow = stats + (size_t)b * C * 4;
  for (int c = t; c < C; c += WG) {
    const int m = hM[c], fp = hP[c] - m, fn = hT[c] - m;
    if (m) atomicAdd(srow + (size_t)c * 4 + 0, (u64)m);
    if (fp) atomicAdd(srow + (size_t)c * 4 + 1, (u64)fp);
    if (fn) atomicAdd(srow + (size_t)c * 4 + 2, (u64)fn);
  }
  if (MODE == CONF_LDS)
    for (int i = t; i < C * C; i += WG) {
      const int v = tile[i];
      if (v) atomicAdd(crow + i, (u64)v);
    }
  if (t == 0 && s_misc[0]) atomicAdd(ignored + b, (u64)s_misc[0]);
  if (t == 1 && s_misc[1]) atomicAdd(stray + b, (u64)s_misc[1]);
}

__global__ __launch_bounds__(WG) void seg_tn_kernel(int64_t* __restrict__ stats, const int64_t* __restrict__ ignored,
                                                    const int64_t* __restrict__ stray, int64_t n, int C) {
  const int c = blockIdx.x * WG + threadIdx.x, b = blockIdx.y;
  if (c >= C) return;
  int64_t* s = stats + ((size_t)b * C + c) * 4;
  s[3] = n - ignored[b] - stray[b] - s[0] - s[1] - s[2];
}

template <typename T, int MODE>
int launch_seg(const int64_t* pred, const void* target, int B, int64_t n, int C, int64_t ignore, int64_t* stats,
               int64_t* conf, int64_t* ignored, int64_t* stray, hipStream_t st) {
  const unsigned chunks = (unsigned)((n + SEG_CHUNK - 1) / SEG_CHUNK);
  const size_t lds = (size_t)(3 * C + (MODE == CONF_LDS ? C * C : 0)) * sizeof(int);
  hipLaunchKernelGGL((seg_count_kernel<T, MODE>), dim3(chunks, B), dim3(WG), lds, st, pred, reinterpret_cast<const T*>(target), n,
                     C, ignore, reinterpret_cast<u64*>(stats), reinterpret_cast<u64*>(conf), reinterpret_cast<u64*>(ignored),
                     reinterpret_cast<u64*>(stray));
  return (int)hipGetLastError();
}

template <typename T>
int launch_seg_mode(int mode, const int64_t* pred, const void* target, int B, int64_t n, int C, int64_t ignore, int64_t* stats,
                    int64_t* conf, int64_t* ignored, int64_t* stray, hipStream_t st) {
  switch (mode) {
    case CONF_NONE: return launch_seg<T, CONF_NONE>(pred, target, B, n, C, ignore, stats, conf, ignored, stray, st);
    case CONF_LDS: return launch_seg<T, CONF_LDS>(pred, target, B, n, C, ignore, stats, conf, ignored, stray, st);
    default: return launch_seg<T, CONF_GLOBAL>(pred, target, B, n, C, ignore, stats, conf, ignored, stray, st);
  }
}

// lanes of a wave by a butterfly (every lane ends with the same sum), then the four waves in wave order
__device__ inline void block_sum(double (&acc)[NS], double (*s_wave)[NS]) {
#pragma unroll
  for (int k = 0; k < NS; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
  const int t = threadIdx.x;
  if ((t & 63) == 0)
#pragma unroll
    for (int k = 0; k < NS; ++k) s_wave[t >> 6][k] = acc[k];
  __syncthreads();
}

__global__ __launch_bounds__(WG) void depth_part_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                        const uint8_t* __restrict__ valid, int64_t n, int nchunk, double lo,
                                                        double hi, double* __restrict__ part) {
  __shared__ double s_wave[WG / 64][NS];
  const int t = threadIdx.x, b = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * DEPTH_CHUNK, i1 = min(n, i0 + DEPTH_CHUNK);
  const float* grow = gt + (size_t)b * n;
  const float* prow = pred + (size_t)b * n;
  const uint8_t* vrow = valid ? valid + (size_t)b * n : nullptr;
  double acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.0;
  for (int64_t i = i0 + t; i < i1; i += WG) {
    const double g = (double)grow[i], p = (double)prow[i];
    // finite and positive (a NaN fails both comparisons), inside the limits (a NaN limit fails neither), not masked out
    const bool ok = g > 0.0 && g < INFINITY && p > 0.0 && p < INFINITY && !(g < lo) && !(g > hi) && (!vrow || vrow[i] != 0);
    if (!ok) {
      acc[10] += 1.0;
      continue;
    }
    const double d = g - p, r = fmax(g / p, p / g);
    const double lg = log(g), lp = log(p), dl = lg - lp;
    acc[0] += 1.0;
    acc[1] += r < 1.25 ? 1.0 : 0.0;
    acc[2] += r < 1.5625 ? 1.0 : 0.0;
    acc[3] += r < 1.953125 ? 1.0 : 0.0;
    acc[4] += fabs(d) / g;
    acc[5] += d * d / g;
    acc[6] += d * d;
    acc[7] += dl * dl;
    acc[8] += lp - lg;
    acc[9] += fabs(log10(g) - log10(p));
  }
  block_sum(acc, s_wave);
  if (t < NS) part[((size_t)b * nchunk + blockIdx.x) * NS + t] = ((s_wave[0][t] + s_wave[1][t]) + s_wave[2][t]) + s_wave[3][t];
}

__global__ __launch_bounds__(WG) void depth_final_kernel(const double* __restrict__ part, int nchunk, double* __restrict__ sums) {
  __shared__ double s_wave[WG / 64][NS];
  const int t = threadIdx.x, b = blockIdx.x;
  const double* rows = part + (size_t)b * nchunk * NS;
  double acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.0;
  for (int ch = t; ch < nchunk; ch += WG)
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] += rows[(size_t)ch * NS + k];
  block_sum(acc, s_wave);
  if (t < NS) sums[(size_t)b * NS + t] = ((s_wave[0][t] + s_wave[1][t]) + s_wave[2][t]) + s_wave[3][t];
}

int check_batch(const char* who, int B, int64_t n, int64_t chunk) {
  if (B < 1 || B > MAX_B) return fail(KP2D_ERR_ARG, "%s: B = %d outside [1, %d]", who, B, MAX_B);
  if (n < 1) return fail(KP2D_ERR_ARG, "%s: n = %lld elements per image", who, (long long)n);
  if ((n + chunk - 1) / chunk > INT32_MAX) return fail(KP2D_ERR_UNSUPPORTED, "%s: n = %lld: more than 2^31 - 1 chunks", who, (long long)n);
  return KP2D_OK;
}

size_t depth_scratch(int B, int64_t n) { return (size_t)B * (size_t)((n + DEPTH_CHUNK - 1) / DEPTH_CHUNK) * NS * sizeof(double); }

}  // namespace

extern "C" {

int kp2d_seg_conf_lds_max(void) { return SEG_CONF_LDS_MAX; }

int kp2d_seg_stats(const int64_t* pred, const void* target, int target_dtype, int B, int64_t n, int num_classes,
                   int64_t ignore_index, int64_t* stats, int64_t* confusion, int64_t* ignored, int64_t* stray, void* stream) {
  if (int e = check_batch("seg_stats", B, n, SEG_CHUNK)) return e;
  const int C = num_classes;
  if (C < 1 || C > SEG_MAX_C) return fail(KP2D_ERR_ARG, "seg_stats: num_classes = %d outside [1, %d]", C, SEG_MAX_C);
  if (target_dtype != KP2D_SEG_U8 && target_dtype != KP2D_SEG_I32 && target_dtype != KP2D_SEG_I64)
    return fail(KP2D_ERR_ARG, "seg_stats: target_dtype = %d (KP2D_SEG_U8, KP2D_SEG_I32 or KP2D_SEG_I64)", target_dtype);
  if (!pred || !target || !stats || !ignored || !stray) return fail(KP2D_ERR_ARG, "seg_stats: null argument");
  if (confusion && C > SEG_CONF_MAX_C)
    return fail(KP2D_ERR_UNSUPPORTED, "seg_stats: confusion matrix for num_classes = %d (at most %d)", C, SEG_CONF_MAX_C);
  if ((uintptr_t)pred % 8 || (uintptr_t)stats % 8 || (uintptr_t)confusion % 8 || (uintptr_t)ignored % 8 || (uintptr_t)stray % 8 ||
      (target_dtype == KP2D_SEG_I64 && (uintptr_t)target % 8) || (target_dtype == KP2D_SEG_I32 && (uintptr_t)target % 4))
    return fail(KP2D_ERR_ARG, "seg_stats: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(pred, st);
  HIP_TRY(hipMemsetAsync(stats, 0, (size_t)B * C * 4 * sizeof(int64_t), st));
  HIP_TRY(hipMemsetAsync(ignored, 0, (size_t)B * sizeof(int64_t), st));
  HIP_TRY(hipMemsetAsync(stray, 0, (size_t)B * sizeof(int64_t), st));
  if (confusion) HIP_TRY(hipMemsetAsync(confusion, 0, (size_t)B * C * C * sizeof(int64_t), st));
  const int mode = !confusion ? CONF_NONE : C <= SEG_CONF_LDS_MAX ? CONF_LDS : CONF_GLOBAL;
  int e;
  if (target_dtype == KP2D_SEG_U8)
    e = launch_seg_mode<uint8_t>(mode, pred, target, B, n, C, ignore_index, stats, confusion, ignored, stray, st);
  else if (target_dtype == KP2D_SEG_I32)
    e = launch_seg_mode<int32_t>(mode, pred, target, B, n, C, ignore_index, stats, confusion, ignored, stray, st);
  else
    e = launch_seg_mode<int64_t>(mode, pred, target, B, n, C, ignore_index, stats, confusion, ignored, stray, st);
  if (e) return fail(KP2D_ERR_HIP, "seg_stats: count kernel: %d", e);
  hipLaunchKernelGGL(seg_tn_kernel, dim3((C + WG - 1) / WG, B), dim3(WG), 0, st, stats, ignored, stray, n, C);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

size_t kp2d_depth_scratch_bytes(int B, int64_t n) {
  if (B < 1 || B > MAX_B || n < 1 || (n + DEPTH_CHUNK - 1) / DEPTH_CHUNK > INT32_MAX) return 0;
  return depth_scratch(B, n);
}

int kp2d_depth_sums(const float* gt, const float* pred, const uint8_t* valid, int B, int64_t n, double min_depth,
                    double max_depth, double* sums, void* scratch, size_t scratch_bytes, void* stream) {
  if (int e = check_batch("depth_sums", B, n, DEPTH_CHUNK)) return e;
  if (!gt || !pred || !sums || !scratch) return fail(KP2D_ERR_ARG, "depth_sums: null argument");
  if ((uintptr_t)gt % 4 || (uintptr_t)pred % 4 || (uintptr_t)sums % 8 || (uintptr_t)scratch % 8)
    return fail(KP2D_ERR_ARG, "depth_sums: misaligned pointer");
  const size_t need = depth_scratch(B, n);
  if (scratch_bytes < need)
    return fail(KP2D_ERR_ARG, "depth_sums: scratch %zu B < required %zu B (kp2d_depth_scratch_bytes)", scratch_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(gt, st);
  const int nchunk = (int)((n + DEPTH_CHUNK - 1) / DEPTH_CHUNK);
  double* part = reinterpret_cast<double*>(scratch);
  hipLaunchKernelGGL(depth_part_kernel, dim3(nchunk, B), dim3(WG), 0, st, gt, pred, valid, n, nchunk, min_depth, max_depth, part);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(depth_final_kernel, dim3(B), dim3(WG), 0, st, part, nchunk, sums);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

}  // extern "C"
