// Keypoint scores on the device (kp2d_kp_repeatability, kp2d_kp_matching_score: include/kp2d.h): the counts and sums behind
// the reference's repeatability / localisation error (src/evaluation/detector.py:67-113) and matching score
// (src/evaluation/descriptor.py:112-170), for batches of image pairs, so that no keypoint, probability or descriptor has to
// leave HBM to be scored.  Stateless like dense_metrics.hip; plain vector code, all geometry in float64 (the reference's
// numpy code is float64: warp_keypoints concatenates the fp32 rows with a float64 column of ones), no float atomics.
//   kp_filter_kernel   one thread per (pair, set, row): warp the point, test the box (repeatability only), write the row's
//                      selection key (0: row is out) and the point that goes on (set 0 of repeatability: the WARPED point)
//   kp_rank_kernel     one thread per (pair, set, row): rank = number of rows with a greater key (keys staged through LDS
//                      256 at a time); rows with rank < keep_k are written to compact slot `rank`: most probable first
//   kp_nearest_kernel  one workgroup per (pair, direction): the other set's compact points staged in LDS, every query row's
//                      squared distance to its nearest row; thread t adds rows t, t + 256, ... in that order, then a fixed tree
//   kp_gather_kernel   descriptors of the selected rows -> compact [B,kk,C] (rows past the selection: zeros)
//   kp_score_kernel    one workgroup per (pair, direction): every query's match (nn_idx of kp2d_match_descriptors_ex) warped
//                      back, visibility and `norm < 3` counted
// The key is (probability as an order-preserving uint32) << 32 | (2^32 - 1 - row): distinct per row, so ranks are a
// permutation and among equal probabilities the LOWER row ranks first (the library's tie rule; numpy's argsort, which the
// reference uses, defines none).  The inverse homography is the adjugate over the determinant in float64; the reference calls
// np.linalg.inv, and the two agree to rounding.  The box test compares x with b0 and y with b1 and the reference passes
// (H, W): x is held against the HEIGHT.  That is the reference's quirk (detector.py:41-46, keypoints.py:133), kept as is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "api_common.h"
#include "device_guard.h"

using namespace kp2d;

namespace {

constexpr int WG = 256;                     // threads of every kernel here
constexpr int NEAR_TILE = 1024;             // rows of the other set per LDS tile of kp_nearest_kernel: 16 KB
constexpr int MAX_B = 65535;                // pairs ride on gridDim.y
constexpr int MAX_K = 65536;                // rows per set: ranking is O(k^2)

typedef unsigned long long u64;

struct Hom { double h[9]; };

__device__ inline Hom load_hom(const double* __restrict__ p) {
  Hom m;
#pragma unroll
  for (int i = 0; i < 9; ++i) m.h[i] = p[i];
  return m;
}

// adjugate / determinant
__device__ inline Hom inverse(const Hom& m) {
  const double* h = m.h;
  Hom a;
  a.h[0] = h[4] * h[8] - h[5] * h[7];
  a.h[1] = h[2] * h[7] - h[1] * h[8];
  a.h[2] = h[1] * h[5] - h[2] * h[4];
  a.h[3] = h[5] * h[6] - h[3] * h[8];
  a.h[4] = h[0] * h[8] - h[2] * h[6];
  a.h[5] = h[2] * h[3] - h[0] * h[5];
  a.h[6] = h[3] * h[7] - h[4] * h[6];
  a.h[7] = h[1] * h[6] - h[0] * h[7];
  a.h[8] = h[0] * h[4] - h[1] * h[3];
  const double det = h[0] * a.h[0] + h[1] * a.h[3] + h[2] * a.h[6];
#pragma unroll
  for (int i = 0; i < 9; ++i) a.h[i] /= det;
  return a;
}

// warp_keypoints (utils/keypoints.py:7-25) for one point
__device__ inline double2 warp(const Hom& m, double x, double y) {
  const double w0 = m.h[0] * x + m.h[1] * y + m.h[2];
  const double w1 = m.h[3] * x + m.h[4] * y + m.h[5];
  const double w2 = m.h[6] * x + m.h[7] * y + m.h[8];
  return make_double2(w0 / w2, w1 / w2);
}

__device__ inline u64 make_key(float prob, int row) {
  uint32_t u = __float_as_uint(prob + 0.0f);                 // -0 -> +0: the two compare equal in the reference
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);           // float order -> unsigned order
  return ((u64)u << 32) | (u64)(0xFFFFFFFFu - (uint32_t)row);
}

struct KpSets {               // both sets of every pair; index 0 / 1 = set
  const float* pts[2];        // [B,k,3] (x, y, prob)
  const int32_t* cnt[2];      // [B]
  int k[2], kk[2];            // rows per pair, compact rows per pair (min(keep_k, k))
  u64* keys[2];               // [B,k]
  double2* wp[2];             // [B,k]  the point a selected row contributes
  double2* cp[2];             // [B,kk] compact points, most probable first
  int32_t* src[2];            // [B,kk] their rows (null: not wanted)
  int32_t* nsel;              // [2,B]  rows selected
  const double* hom;          // [B,9]
  int B;
  double b0, b1;
};

__device__ inline int valid_rows(const KpSets& a, int s, int b) { return min(max(a.cnt[s][b], 0), a.k[s]); }

// grid (ceil(max k / WG), B, 2)
template <bool BOX>
__global__ __launch_bounds__(WG) void kp_filter_kernel(const KpSets a) {
  const int s = blockIdx.z, b = blockIdx.y, i = blockIdx.x * WG + threadIdx.x;
  if (i >= a.k[s]) return;
  const size_t o = (size_t)b * a.k[s] + i;
  u64 key = 0;
  double2 p = make_double2(0.0, 0.0);
  if (i < valid_rows(a, s, b)) {
    const float* row = a.pts[s] + o * 3;
    p = make_double2((double)row[0], (double)row[1]);
    bool in = true;
    if (BOX) {
      const Hom h = load_hom(a.hom + (size_t)b * 9);
      const double2 w = warp(s == 0 ? h : inverse(h), p.x, p.y);
      in = w.x >= 0.0 && w.x < a.b0 && w.y >= 0.0 && w.y < a.b1;     // a NaN fails
      if (s == 0) p = w;
    }
    if (in) key = make_key(row[2], i);
  }
  a.keys[s][o] = key;
  a.wp[s][o] = p;
}

// grid (max(1, ceil(max k / WG)), B, 2): every thread walks all keys of its (pair, set), so block 0 also knows the total
__global__ __launch_bounds__(WG) void kp_rank_kernel(const KpSets a) {
  __shared__ u64 s_keys[WG];
  const int s = blockIdx.z, b = blockIdx.y, t = threadIdx.x, i = blockIdx.x * WG + t;
  const int k = a.k[s];
  if (blockIdx.x * WG >= k && blockIdx.x != 0) return;               // (uniform)
  const u64* keys = a.keys[s] + (size_t)b * k;
  const u64 mine = i < k ? keys[i] : 0;
  int rank = 0, total = 0;
  for (int j0 = 0; j0 < k; j0 += WG) {
    __syncthreads();
    s_keys[t] = j0 + t < k ? keys[j0 + t] : 0;
    __syncthreads();
    const int n = min(WG, k - j0);
    for (int j = 0; j < n; ++j) {
      const u64 other = s_keys[j];
      rank += other > mine ? 1 : 0;
      total += other != 0 ? 1 : 0;
    }
  }
  if (mine != 0 && rank < a.kk[s]) {
    const size_t o = (size_t)b * a.kk[s] + rank;
    a.cp[s][o] = a.wp[s][(size_t)b * k + i];
    if (a.src[s]) a.src[s][o] = i;
  }
  if (i == 0) a.nsel[s * a.B + b] = min(total, a.kk[s]);
}

__device__ inline double block_sum(double v, double* s_d) {
  const int t = threadIdx.x;
  __syncthreads();
  s_d[t] = v;
  __syncthreads();
  for (int o = WG / 2; o > 0; o >>= 1) {
    if (t < o) s_d[t] += s_d[t + o];
    __syncthreads();
  }
  return s_d[0];
}

__device__ inline int block_sum(int v, int* s_i) {
  const int t = threadIdx.x;
  __syncthreads();
  s_i[t] = v;
  __syncthreads();
  for (int o = WG / 2; o > 0; o >>= 1) {
    if (t < o) s_i[t] += s_i[t + o];
    __syncthreads();
  }
  return s_i[0];
}

// grid (B, 2).  Direction d: query rows = set d, the rows searched = set 1 - d.
// counts [B,4] = (N1, N2, count1, count2), le [B,2] = (le1, le2)
__global__ __launch_bounds__(WG) void kp_nearest_kernel(const KpSets a, double thresh, int64_t* __restrict__ counts,
                                                        double* __restrict__ le) {
  __shared__ double2 s_pts[NEAR_TILE];
  __shared__ double s_d[WG];
  __shared__ int s_i[WG];
  const int b = blockIdx.x, d = blockIdx.y, t = threadIdx.x;
  const int nq = a.nsel[d * a.B + b], nt = a.nsel[(1 - d) * a.B + b];
  const double2* q = a.cp[d] + (size_t)b * a.kk[d];
  const double2* o = a.cp[1 - d] + (size_t)b * a.kk[1 - d];
  int count = 0;
  double sum = 0.0;
  if (nt > 0)
    for (int q0 = 0; q0 < nq; q0 += WG) {                            // (uniform trip count: the barriers below are safe)
      const bool on = q0 + t < nq;
      const double2 p = on ? q[q0 + t] : make_double2(0.0, 0.0);
      double best = INFINITY;
      for (int t0 = 0; t0 < nt; t0 += NEAR_TILE) {
        const int n = min(NEAR_TILE, nt - t0);
        __syncthreads();
        for (int e = t; e < n; e += WG) s_pts[e] = o[t0 + e];
        __syncthreads();
        for (int j = 0; j < n; ++j) {
          const double dx = p.x - s_pts[j].x, dy = p.y - s_pts[j].y;
          const double d2 = dx * dx + dy * dy;
          best = d2 < best ? d2 : best;                              // a NaN never wins
        }
      }
      const double dist = sqrt(best);                                // sqrt is monotone: min of the norms = norm of the min
      if (on && dist <= thresh) {
        ++count;
        sum += dist;
      }
    }
  const int c = block_sum(count, s_i);
  const double l = block_sum(sum, s_d);
  if (t == 0) {
    counts[(size_t)b * 4 + d] = nq;
    counts[(size_t)b * 4 + 2 + d] = c;
    le[(size_t)b * 2 + d] = l;
  }
}

struct KpGather {
  const float* desc[2];       // [B,k,C]
  float* out[2];              // [B,kk,C]
  int C;
};

// grid (ceil(max kk * C / 4 / WG), B, 2): one float4 per thread
__global__ __launch_bounds__(WG) void kp_gather_kernel(const KpSets a, const KpGather g) {
  const int s = blockIdx.z, b = blockIdx.y, e = blockIdx.x * WG + threadIdx.x;
  const int c4n = g.C / 4, row = e / c4n, c4 = e - row * c4n;
  if (row >= a.kk[s]) return;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row < a.nsel[s * a.B + b]) {
    const int src = a.src[s][(size_t)b * a.kk[s] + row];
    v = reinterpret_cast<const float4*>(g.desc[s] + ((size_t)b * a.k[s] + src) * g.C)[c4];
  }
  reinterpret_cast<float4*>(g.out[s] + ((size_t)b * a.kk[s] + row) * g.C)[c4] = v;
}

// grid (B, 2).  Direction 0: queries = set 0, their matches in set 1 warped back by inv(H) (descriptor.py:134-152);
// direction 1: queries = set 1, their matches in set 0 warped by H (:154-168).  counts [B,4] = (vis1, hit1, vis2, hit2)
__global__ __launch_bounds__(WG) void kp_score_kernel(const KpSets a, const int32_t* __restrict__ nn01,
                                                      const int32_t* __restrict__ nn10, int64_t* __restrict__ counts) {
  __shared__ int s_i[WG];
  const int b = blockIdx.x, d = blockIdx.y, t = threadIdx.x;
  const int nq = a.nsel[d * a.B + b], nt = a.nsel[(1 - d) * a.B + b];
  const double2* q = a.cp[d] + (size_t)b * a.kk[d];
  const double2* o = a.cp[1 - d] + (size_t)b * a.kk[1 - d];
  const int32_t* nn = (d == 0 ? nn01 : nn10) + (size_t)b * a.kk[d];
  const Hom h = load_hom(a.hom + (size_t)b * 9);
  const Hom m = d == 0 ? inverse(h) : h;
  int vis = 0, hit = 0;
  if (nt > 0)
    for (int i = t; i < nq; i += WG) {
      const int j = nn[i];
      if (j < 0 || j >= nt) continue;                                // no neighbour
      const double2 w = warp(m, o[j].x, o[j].y);
      const bool v = w.x >= 0.0 && w.x <= a.b0 - 1.0 && w.y >= 0.0 && w.y <= a.b1 - 1.0;
      const double dx = w.x - q[i].x, dy = w.y - q[i].y;
      const bool c = sqrt(dx * dx + dy * dy) < 3.0;
      vis += v ? 1 : 0;
      hit += (v && c) ? 1 : 0;
    }
  const int nv = block_sum(vis, s_i);
  const int nh = block_sum(hit, s_i);
  if (t == 0) {
    counts[(size_t)b * 4 + 2 * d] = nv;
    counts[(size_t)b * 4 + 2 * d + 1] = nh;
  }
}

// scratch layout, every piece on an ALIGN boundary: one walk fills the selection's buffers (a.keys / wp / cp / nsel, kk) and,
// for the matching score (C > 0), the compact rows, the descriptors gathered by them and the matcher's outputs and scratch.
// C = 0: repeatability only.
struct KpScratch {
  int32_t* nn[2];             // [B,kk] nearest row of the other set, per direction
  float* nd; float* nd2; int32_t* mq; float* md;      // the matcher's other outputs (not read): [B, max kk]
  void* match; size_t match_bytes;                     // its scratch, for the larger direction
  size_t bytes;
};

KpScratch kp_layout(void* scratch, int B, int k0, int k1, int C, int keep_k, KpSets& a, KpGather& g) {
  Carve c(scratch);
  KpScratch w{};
  a.B = B;
  a.k[0] = k0; a.k[1] = k1;
  for (int s = 0; s < 2; ++s) {
    a.kk[s] = std::min(keep_k, a.k[s]);
    a.keys[s] = c.take<u64>((size_t)B * a.k[s]);
    a.wp[s] = c.take<double2>((size_t)B * a.k[s]);
    a.cp[s] = c.take<double2>((size_t)B * a.kk[s]);
  }
  a.nsel = c.take<int32_t>((size_t)2 * B);
  if (C > 0) {
    const size_t km = (size_t)std::max(a.kk[0], a.kk[1]);
    g.C = C;
    for (int s = 0; s < 2; ++s) {
      a.src[s] = c.take<int32_t>((size_t)B * a.kk[s]);
      g.out[s] = c.take<float>((size_t)B * a.kk[s] * C);
      w.nn[s] = c.take<int32_t>((size_t)B * a.kk[s]);
    }
    w.nd = c.take<float>(B * km);
    w.nd2 = c.take<float>(B * km);
    w.mq = c.take<int32_t>(B * km);
    w.md = c.take<float>(B * km);
    w.match_bytes = std::max(kp2d_match_scratch_bytes(B, a.kk[0], a.kk[1]), kp2d_match_scratch_bytes(B, a.kk[1], a.kk[0]));
    w.match = c.take<char>(w.match_bytes);
  }
  w.bytes = std::max(c.bytes(), ALIGN);
  return w;
}

int check_shape(const char* who, int B, int k0, int k1, int keep_k) {
  if (B < 1 || B > MAX_B) return fail(KP2D_ERR_ARG, "%s: B = %d outside [1, %d]", who, B, MAX_B);
  if (k0 < 0 || k0 > MAX_K || k1 < 0 || k1 > MAX_K)
    return fail(KP2D_ERR_ARG, "%s: k0 = %d, k1 = %d rows per set outside [0, %d]", who, k0, k1, MAX_K);
  if (keep_k < 1) return fail(KP2D_ERR_ARG, "%s: keep_k = %d must be >= 1", who, keep_k);
  return KP2D_OK;
}

int check_common(const char* who, const float* pts0, const int32_t* cnt0, const float* pts1, const int32_t* cnt1,
                 const double* hom, int k0, int k1, double b0, double b1, const void* out, void* scratch, size_t scratch_bytes,
                 size_t need) {
  if ((k0 > 0 && !pts0) || (k1 > 0 && !pts1) || !cnt0 || !cnt1 || !hom || !out || !scratch)
    return fail(KP2D_ERR_ARG, "%s: null argument", who);
  if (std::isnan(b0) || std::isnan(b1)) return fail(KP2D_ERR_ARG, "%s: bounds (%g, %g)", who, b0, b1);
  if ((uintptr_t)pts0 % 4 || (uintptr_t)pts1 % 4 || (uintptr_t)cnt0 % 4 || (uintptr_t)cnt1 % 4 || (uintptr_t)hom % 8 ||
      (uintptr_t)out % 8 || (uintptr_t)scratch % 16)
    return fail(KP2D_ERR_ARG, "%s: misaligned pointer", who);
  if (scratch_bytes < need)
    return fail(KP2D_ERR_ARG, "%s: scratch %zu B < required %zu B (kp2d_kp_scratch_bytes)", who, scratch_bytes, need);
  return KP2D_OK;
}

template <bool BOX>
int launch_select(const KpSets& a, hipStream_t st) {
  const unsigned gx = (unsigned)std::max(1, (std::max(a.k[0], a.k[1]) + WG - 1) / WG);
  hipLaunchKernelGGL(kp_filter_kernel<BOX>, dim3(gx, a.B, 2), dim3(WG), 0, st, a);
  hipLaunchKernelGGL(kp_rank_kernel, dim3(gx, a.B, 2), dim3(WG), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t kp2d_kp_scratch_bytes(int B, int k0, int k1, int C, int keep_k) {
  if (B < 1 || B > MAX_B || k0 < 0 || k0 > MAX_K || k1 < 0 || k1 > MAX_K || keep_k < 1) return 0;
  if (C != 0 && C != 32 && C != 64 && C != 128) return 0;
  KpSets a{};
  KpGather g{};
  return kp_layout(nullptr, B, k0, k1, C, keep_k, a, g).bytes;
}

int kp2d_kp_repeatability(const float* pts0, const int32_t* cnt0, const float* pts1, const int32_t* cnt1, const double* hom,
                          int B, int k0, int k1, double b0, double b1, int keep_k, double distance_thresh, int64_t* counts,
                          double* le, void* scratch, size_t scratch_bytes, void* stream) {
  if (int e = check_shape("kp_repeatability", B, k0, k1, keep_k)) return e;
  if (std::isnan(distance_thresh)) return fail(KP2D_ERR_ARG, "kp_repeatability: distance_thresh is NaN");
  KpSets a{{pts0, pts1}, {cnt0, cnt1}};
  a.hom = hom; a.b0 = b0; a.b1 = b1;
  KpGather g{};
  const KpScratch w = kp_layout(scratch, B, k0, k1, 0, keep_k, a, g);
  if (int e = check_common("kp_repeatability", pts0, cnt0, pts1, cnt1, hom, k0, k1, b0, b1, counts, scratch, scratch_bytes, w.bytes))
    return e;
  if (!le || (uintptr_t)le % 8) return fail(KP2D_ERR_ARG, "kp_repeatability: le is null or misaligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(hom, st);
  if (int e = launch_select<true>(a, st)) return fail(KP2D_ERR_HIP, "kp_repeatability: selection kernels: %d", e);
  hipLaunchKernelGGL(kp_nearest_kernel, dim3(B, 2), dim3(WG), 0, st, a, distance_thresh, counts, le);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_kp_matching_score(const float* pts0, const int32_t* cnt0, const float* desc0, const float* pts1, const int32_t* cnt1,
                           const float* desc1, const double* hom, int B, int k0, int k1, int C, double b0, double b1,
                           int keep_k, int64_t* counts, void* scratch, size_t scratch_bytes, void* stream) {
  if (int e = check_shape("kp_matching_score", B, k0, k1, keep_k)) return e;
  if (C != 32 && C != 64 && C != 128) return fail(KP2D_ERR_ARG, "kp_matching_score: descriptor width %d (32, 64 or 128)", C);
  KpSets a{{pts0, pts1}, {cnt0, cnt1}};
  a.hom = hom; a.b0 = b0; a.b1 = b1;
  KpGather g{};
  g.desc[0] = desc0; g.desc[1] = desc1;
  const KpScratch w = kp_layout(scratch, B, k0, k1, C, keep_k, a, g);
  if (int e = check_common("kp_matching_score", pts0, cnt0, pts1, cnt1, hom, k0, k1, b0, b1, counts, scratch, scratch_bytes, w.bytes))
    return e;
  if ((k0 > 0 && !desc0) || (k1 > 0 && !desc1)) return fail(KP2D_ERR_ARG, "kp_matching_score: null descriptors");
  if ((uintptr_t)desc0 % 16 || (uintptr_t)desc1 % 16) return fail(KP2D_ERR_ARG, "kp_matching_score: descriptors must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(hom, st);
  if (k0 == 0 || k1 == 0) {                    // the reference's `if not matches: return 0`
    HIP_TRY(hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(int64_t), st));
    return KP2D_OK;
  }
  if (int e = launch_select<false>(a, st)) return fail(KP2D_ERR_HIP, "kp_matching_score: selection kernels: %d", e);
  const int kmax = std::max(a.kk[0], a.kk[1]);
  hipLaunchKernelGGL(kp_gather_kernel, dim3((unsigned)(((size_t)kmax * (C / 4) + WG - 1) / WG), B, 2), dim3(WG), 0, st, a, g);
  HIP_TRY(hipGetLastError());
  // cv2.BFMatcher(NORM_L2, crossCheck=False).match in both directions: nn_idx is all that is read
  for (int d = 0; d < 2; ++d)
    if (int e = kp2d_match_descriptors_ex(g.out[d], a.nsel + d * B, g.out[1 - d], a.nsel + (1 - d) * B, B, a.kk[d], a.kk[1 - d], C,
                                          0.7f, nullptr, nullptr, 0u, w.nn[d], w.nd, w.nd2, w.mq, w.md, w.match, w.match_bytes, stream))
      return e;
  hipLaunchKernelGGL(kp_score_kernel, dim3(B, 2), dim3(WG), 0, st, a, w.nn[0], w.nn[1], counts);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

}  // extern "C"
