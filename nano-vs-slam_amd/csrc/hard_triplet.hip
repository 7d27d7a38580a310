// The multitask place-recognition loss on the device (kp2d_hard_triplet_loss, include/kp2d.h): the reference's HardTripletLoss
// (src/kp2dtiny/utils/losses.py:9-152) on a batch of M embeddings with integer labels, forward and gradient, three launches.
//   ht_dist_kernel          a workgroup per 16 x 16 tile of the upper triangle of the distance matrix (a triangular
//                           launch), dim walked in chunks of 128 through LDS; a thread owns one pair and adds the squares of the widened differences in
//                           float64 in ascending order of the dimension, so (i, j) and (j, i) are one number, written to both
//                           places, and two bitwise-equal rows are at distance exactly 0
//   ht_mine_kernel<HARDEST> a workgroup per anchor with the anchor's row of distances and the labels in LDS.  HARDEST: wave 0
//                           finds the three arg-extrema (lowest index among equal values) and the hinge.  Batch-all: a thread
//                           per column counts the active triplets the column takes part in, as the negative (over the
//                           positives in ascending order, adding the hinges in float64) or as the positive (over the
//                           negatives).  Either way the anchor's row of the INTEGER coefficient matrix c is written in full:
//                           d loss / d d_aj = scale * c_aj, with scale = weight / M or weight / (hard triplets + 1e-16).
//   ht_grad_kernel          a workgroup per row i gathers demb_i = sum_j s_ij (x_i - x_j) over j ascending in fp32 from the
//                           columns with c_ij + c_ji != 0 and d_ij > 0 (the receiving row scans; no atomics); the extra last
//                           workgroup adds the anchors' hinge sums and counts and writes loss and stats.
// Counts are integers, so their sums are exact in any order; every float sum has a fixed order: bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "api_common.h"
#include "device_guard.h"
#include "train_common.h"

using namespace kp2d;

namespace {

constexpr int HT_MAX_M = 512;
constexpr int HT_TILE = 16;       // pairs per tile side
constexpr int HT_KC = 128;        // dimensions per LDS chunk

struct HtPlan {
  float* dist;        // [M, M]
  int32_t* coef;      // [M, M]
  double* hsum;       // [M] an anchor's hinge sum
  int64_t* hcnt;      // [M] an anchor's active hinges (HARDEST: 0 or 1; batch-all: its hard triplets, h > 1e-16)
  int32_t* flags;     // [M, 3] no positive, no negative, zero off-diagonal entries of the row
  size_t total;
};

HtPlan ht_plan(void* scratch, int M) {
  HtPlan p{};
  Carve c(scratch);
  p.dist = c.take<float>((size_t)M * M);
  p.coef = c.take<int32_t>((size_t)M * M);
  p.hsum = c.take<double>(M);
  p.hcnt = c.take<int64_t>(M);
  p.flags = c.take<int32_t>((size_t)M * 3);
  p.total = c.bytes();
  return p;
}

__global__ __launch_bounds__(256) void ht_dist_kernel(const float* __restrict__ x, int M, int dim, int squared, float* __restrict__ dist) {
  int bi = 0, bj = blockIdx.x;                        // the upper triangle of tiles, row by row: row bi holds tiles bi ... T - 1
  for (int T = (M + HT_TILE - 1) / HT_TILE; bj >= T - bi; ++bi) bj -= T - bi;
  bj += bi;                                           // (the mirror image is written from here)
  __shared__ float s_a[HT_TILE][HT_KC + 1], s_b[HT_TILE][HT_KC + 1];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int i = bi * HT_TILE + ti, j = bj * HT_TILE + tj;
  double acc = 0.0;
  for (int k0 = 0; k0 < dim; k0 += HT_KC) {
    __syncthreads();
    for (int e = tid; e < HT_TILE * HT_KC; e += 256) {
      const int r = e / HT_KC, c = e % HT_KC, gk = k0 + c;
      const int ga = bi * HT_TILE + r, gb = bj * HT_TILE + r;
      s_a[r][c] = (ga < M && gk < dim) ? x[(size_t)ga * dim + gk] : 0.f;      // past the end: zeros, whose difference adds 0
      s_b[r][c] = (gb < M && gk < dim) ? x[(size_t)gb * dim + gk] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int c = 0; c < HT_KC; ++c) {
      const double d = (double)s_a[ti][c] - (double)s_b[tj][c];               // exact; (a - b)^2 and (b - a)^2 are one number
      acc = fma(d, d, acc);
    }
  }
  if (i >= M || j >= M || (bi == bj && j < i)) return;
  const float v = i == j ? 0.f : squared ? (float)acc : (float)sqrt(acc);
  dist[(size_t)i * M + j] = v;
  dist[(size_t)j * M + i] = v;
}

// (value, index) with the lowest index among equal values; MAX: the larger value wins, else the smaller
template <bool MAX>
__device__ __forceinline__ void better(float& v, int& j, float ov, int oj) {
  const bool take = MAX ? (ov > v || (ov == v && oj < j)) : (ov < v || (ov == v && oj < j));
  if (take) { v = ov; j = oj; }
}
template <bool MAX>
__device__ __forceinline__ void wave_arg(float& v, int& j) {
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oj = __shfl_xor(j, o);
    better<MAX>(v, j, ov, oj);
  }
}
__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// block sums in a fixed order: lanes by butterfly, the four waves as (0 + 1) + (2 + 3); every thread calls and gets the sum
template <typename T>
__device__ __forceinline__ T ht_block_sum(T v, T* s_w) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

template <bool HARDEST>
__global__ __launch_bounds__(256) void ht_mine_kernel(const float* __restrict__ dist, const int32_t* __restrict__ labels, int M, float margin,
                                                      int32_t* __restrict__ coef, double* __restrict__ hsum, int64_t* __restrict__ hcnt,
                                                      int32_t* __restrict__ flags) {
  __shared__ float s_d[HT_MAX_M];
  __shared__ int s_l[HT_MAX_M], s_c[HT_MAX_M];
  __shared__ double s_wd[4];
  __shared__ int s_wi[4];
  const int a = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < M; j += 256) {
    s_d[j] = dist[(size_t)a * M + j];
    s_l[j] = labels[j];
    s_c[j] = 0;
  }
  __syncthreads();
  const int la = s_l[a];
  int npos = 0, nneg = 0, nzero = 0;
  for (int j = tid; j < M; j += 256) {
    if (j != a && s_l[j] == la) ++npos;
    if (s_l[j] != la) ++nneg;
    if (j != a && s_d[j] == 0.f) ++nzero;
  }
  npos = ht_block_sum(npos, s_wi);
  nneg = ht_block_sum(nneg, s_wi);
  nzero = ht_block_sum(nzero, s_wi);
  if (tid == 0) {
    flags[3 * a] = npos == 0;
    flags[3 * a + 1] = nneg == 0;
    flags[3 * a + 2] = nzero;
  }
  if (HARDEST) {
    if (tid < 64) {
      // hp = max_j d_aj [j != a, same label]; rowmax = max_j d_aj
      float hp = -1.f, rm = -1.f;
      int jp = M, jm = M;
      for (int j = tid; j < M; j += 64) {
        better<true>(hp, jp, (j != a && s_l[j] == la) ? s_d[j] : 0.f, j);
        better<true>(rm, jm, s_d[j], j);
      }
      wave_arg<true>(hp, jp);
      wave_arg<true>(rm, jm);
      // hn = min_j (d_aj + rowmax [same label]): a same-label column passes its gradient to d_aj and to the row maximum
      float hn = INFINITY;
      int jn = M;
      for (int j = tid; j < M; j += 64) better<false>(hn, jn, s_l[j] == la ? s_d[j] + rm : s_d[j], j);
      wave_arg<false>(hn, jn);
      if (tid == 0) {
        const float h = (hp - hn) + margin;
        const bool on = h > 0.f;
        hsum[a] = on ? (double)h : 0.0;
        hcnt[a] = on;
        if (on) {
          if (jp != a && s_l[jp] == la) s_c[jp] += 1;      // a maximum of 0 on a masked column: the mask's factor is 0
          s_c[jn] -= 1;
          if (s_l[jn] == la) s_c[jm] -= 1;
        }
      }
    }
  } else {
    double sum = 0.0;
    int hard = 0;
    for (int j = tid; j < M; j += 256) {
      const float dj = s_d[j];
      int c = 0;
      if (s_l[j] != la) {                             // the negative of (a, p, j) for every positive p
        for (int p = 0; p < M; ++p) {
          if (p == a || s_l[p] != la) continue;
          const float h = (s_d[p] - dj) + margin;
          if (h > 0.f) { --c; sum += (double)h; }
          if (h > 1e-16f) ++hard;
        }
      } else if (j != a) {                            // the positive of (a, j, n) for every negative n
        for (int n = 0; n < M; ++n) {
          if (s_l[n] == la) continue;
          if ((dj - s_d[n]) + margin > 0.f) ++c;
        }
      }
      s_c[j] = c;
    }
    sum = ht_block_sum(sum, s_wd);
    hard = ht_block_sum(hard, s_wi);
    if (tid == 0) { hsum[a] = sum; hcnt[a] = hard; }
  }
  __syncthreads();
  for (int j = tid; j < M; j += 256) coef[(size_t)a * M + j] = s_c[j];
}

template <bool HARDEST>
__global__ __launch_bounds__(256) void ht_grad_kernel(const float* __restrict__ x, int M, int dim, int squared, double weight,
                                                      const float* __restrict__ dist, const int32_t* __restrict__ coef,
                                                      const double* __restrict__ hsum, const int64_t* __restrict__ hcnt,
                                                      const int32_t* __restrict__ flags, float* __restrict__ loss, float* __restrict__ demb,
                                                      int64_t* __restrict__ stats) {
  __shared__ float s_s[HT_MAX_M], s_val[HT_MAX_M];
  __shared__ int s_idx[HT_MAX_M];
  __shared__ int s_n;
  __shared__ double s_wd[4];
  __shared__ long long s_wl[4];
  __shared__ int s_wi[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  long long cnt = 0;
  if (!HARDEST || i == M) {
    for (int a = tid; a < M; a += 256) cnt += hcnt[a];
    cnt = ht_block_sum(cnt, s_wl);
  }
  const double denom = HARDEST ? (double)M : (double)cnt + 1e-16;
  if (i == M) {                                       // loss and stats: the anchors' sums, thread t taking t and t + 256
    double sum = 0.0;
    int f0 = 0, f1 = 0, f2 = 0;
    for (int a = tid; a < M; a += 256) {
      sum += hsum[a];
      f0 += flags[3 * a]; f1 += flags[3 * a + 1]; f2 += flags[3 * a + 2];
    }
    sum = ht_block_sum(sum, s_wd);
    f0 = ht_block_sum(f0, s_wi);
    f1 = ht_block_sum(f1, s_wi);
    f2 = ht_block_sum(f2, s_wi);
    if (tid == 0) {
      loss[0] = (float)(weight * sum / denom);
      stats[0] = cnt; stats[1] = f0; stats[2] = f1; stats[3] = f2;
    }
    return;
  }
  const float scale = (float)(weight / denom);
  for (int j = tid; j < M; j += 256) {
    const int c = coef[(size_t)i * M + j] + coef[(size_t)j * M + i];
    const float d = dist[(size_t)i * M + j];
    float s = 0.f;
    if (c != 0 && d > 0.f) s = squared ? 2.f * (scale * (float)c) : (scale * (float)c) / d;      // a zero entry passes nothing
    s_s[j] = s;
  }
  __syncthreads();
  if (tid < 64) {                                     // the columns with s != 0, ascending
    int n = 0;
    for (int base = 0; base < M; base += 64) {
      const int j = base + tid;
      const bool on = j < M && s_s[j] != 0.f;
      const unsigned long long m = __ballot(on);
      if (on) {
        const int at = n + __popcll(m & ((1ull << tid) - 1ull));
        s_idx[at] = j;
        s_val[at] = s_s[j];
      }
      n += __popcll(m);
    }
    if (tid == 0) s_n = n;
  }
  __syncthreads();
  const int n = s_n;
  const float* xi = x + (size_t)i * dim;
  float* out = demb + (size_t)i * dim;
  for (int e = tid; e < dim; e += 256) {
    const float v = xi[e];
    float acc = 0.f;
    for (int q = 0; q < n; ++q) acc = fmaf(s_val[q], v - x[(size_t)s_idx[q] * dim + e], acc);
    out[e] = acc;
  }
}

const char* ht_shape_problem(int M, int dim, int* code) {
  *code = KP2D_ERR_ARG;
  if (M < 1) return "M < 1";
  if (dim < 1) return "dim < 1";
  *code = KP2D_ERR_UNSUPPORTED;
  if (M > HT_MAX_M) return "M > 512";
  return nullptr;
}

}  // namespace

extern "C" {

size_t kp2d_hard_triplet_scratch_bytes(int M, int dim) {
  int code;
  if (ht_shape_problem(M, dim, &code)) return 0;
  return ht_plan(nullptr, M).total;
}

int kp2d_hard_triplet_loss(const float* emb, const int32_t* labels, int M, int dim, double margin, uint32_t flags, double weight,
                           float* loss, float* demb, int64_t* stats, void* scratch, size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = ht_shape_problem(M, dim, &code)) return fail(code, "hard_triplet_loss: %s (M %d, dim %d)", why, M, dim);
  if (!std::isfinite(margin) || margin < 0.0 || !std::isfinite(weight))
    return fail(KP2D_ERR_ARG, "hard_triplet_loss: margin %g (finite, >= 0), weight %g (finite)", margin, weight);
  if (flags & ~(uint32_t)(KP2D_HT_HARDEST | KP2D_HT_SQUARED)) return fail(KP2D_ERR_ARG, "hard_triplet_loss: unknown flags 0x%x", flags);
  if (any_null(emb, labels, loss, demb, stats, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(emb, labels, loss, demb) || misaligned(stats, 8) || misaligned(scratch, 16))
    return fail(KP2D_ERR_ARG, "hard_triplet_loss: float and int32 arrays must be 4-byte aligned, stats 8-byte, scratch 16-byte");
  const HtPlan p = ht_plan(scratch, M);
  if (scratch_bytes < p.total)
    return fail(KP2D_ERR_ARG, "hard_triplet_loss scratch %zu B < required %zu B (kp2d_hard_triplet_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(emb, st);
  const int squared = (flags & KP2D_HT_SQUARED) != 0;
  const int T = (M + HT_TILE - 1) / HT_TILE;
  hipLaunchKernelGGL(ht_dist_kernel, dim3(T * (T + 1) / 2), dim3(256), 0, st, emb, M, dim, squared, p.dist);
  HIP_TRY(hipGetLastError());
  if (flags & KP2D_HT_HARDEST) {
    hipLaunchKernelGGL(ht_mine_kernel<true>, dim3(M), dim3(256), 0, st, p.dist, labels, M, (float)margin, p.coef, p.hsum, p.hcnt, p.flags);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ht_grad_kernel<true>, dim3(M + 1), dim3(256), 0, st, emb, M, dim, squared, weight, p.dist, p.coef, p.hsum, p.hcnt,
                       p.flags, loss, demb, stats);
  } else {
    hipLaunchKernelGGL(ht_mine_kernel<false>, dim3(M), dim3(256), 0, st, p.dist, labels, M, (float)margin, p.coef, p.hsum, p.hcnt, p.flags);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ht_grad_kernel<false>, dim3(M + 1), dim3(256), 0, st, emb, M, dim, squared, weight, p.dist, p.coef, p.hsum, p.hcnt,
                       p.flags, loss, demb, stats);
  }
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

}  // extern "C"
