// k-means on the device (kp2d_kmeans_*, include/kp2d.h): Lloyd iterations with faiss.Kmeans' conventions, the fit behind
// NetVLAD's centroids (reference utils/netvlad_utils.py:83-88) and the building block of later retrieval structures.
// The assignment IS kp2d_vpr_search with the centroids as the database (vpr.hip, k = 1, fixed query chunks); this file
// adds what faiss does around the search, with every sum in a fixed order and no float atomics:
//   km_hist_kernel      per-slab histograms of `assign` (integer global atomics; a slab is a fixed run of rows)
//   km_colscan_kernel   per cluster: the slabs' histograms -> running offsets inside the cluster's list, and its count
//   km_scan_kernel      one workgroup: exclusive scans over clusters (list starts, chunk starts, the empty clusters in
//                       ascending order) and the objective, sum of dist accumulated in double in a fixed order
//   km_scatter_kernel   one wave per slab walks its rows in order and writes row numbers into the inverted index: a
//                       stable counting sort, every list keeps ascending point order
//   km_sum_kernel       one wave per (cluster, chunk of CHUNK = 512 rows): rows gathered by index with 16-byte loads
//                       (register staging).  Lane = (row group g, float4 column); group g takes rows g, g + G, ... of
//                       the chunk into UNR = 8 accumulators round-robin, so no sequential run exceeds CHUNK / (8 G)
//                       rows; accumulators and then groups are combined by fixed trees.  G depends on dim alone.
//   km_update_kernel    per cluster: chunk partials added in chunk order, times 1 / count (fp32); empty: input centroid
//   km_split_kernel     one workgroup: faiss's split_clusters for the empty clusters in ascending order (below)
//   km_normalize_kernel KP2D_KMEANS_SPHERICAL: every centroid divided by its norm
// Slab, chunk and group sizes are constants or functions of (n, k, dim): nothing depends on the device, the occupancy
// or the environment, so a result is bit-identical from run to run and however the work is sliced.
// Split rule (faiss's algorithm, not faiss's random stream): for every empty cluster ci in ascending order, a donor cj
// is drawn with probability proportional to max(count_j - 1, 0) over the RUNNING counts; c[ci] = c[cj], then component
// j of c[ci] is multiplied by 1 + 1/1024 and of c[cj] by 1 - 1/1024 for even j (swapped for odd j), and the donor's
// running count is halved between the two (ci gets count_j / 2).  The draw is a counter-based hash of
// (seed, iteration, ci): r = mix(seed, iteration, ci) mod sum_j max(count_j - 1, 0), cj = the cluster whose cumulated
// weight interval holds r.  No state, no host round trip.
// Rows the search cannot place (a non-finite element: assign = -1) belong to no cluster and do not enter the objective.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "api_common.h"
#include "device_guard.h"
#include "kp2d_kernels.h"
#include "mix64.h"

using namespace kp2d;

namespace {

constexpr int QCHUNK = 16384;               // queries per search call: scratch does not grow with n
constexpr int CHUNK = 512;                  // rows of a list one wave sums
constexpr int UNR = 8;                      // accumulators per lane
constexpr int SB = 1024;                    // threads of the single-workgroup kernels
constexpr int MIN_SLAB = 256;               // rows per slab at least
constexpr int64_t HIST_CELLS = 1 << 22;     // slabs x k at most (16 MB of histograms), unless k alone exceeds it
constexpr float SPLIT_EPS = 1.f / 1024.f;

// the slicing of a step and its scratch (with the two centroid buffers kp2d_kmeans_train alternates between), as one walk:
// every piece on an ALIGN boundary.  scratch == nullptr: the sizing pass
struct KmPlan {
  int nslab;
  int64_t slab, nwork;
  unsigned char *cpack, *vpr;      // the centroids packed as a vpr database; the search's own scratch
  int *hist, *start, *cstart, *rcount, *elist, *meta, *order;
  float *part, *c0, *c1;
  size_t total;
};

KmPlan km_plan(void* scratch, int64_t n, int dim, int k) {
  KmPlan p{};
  const int64_t by_rows = (n + MIN_SLAB - 1) / MIN_SLAB, by_cells = std::max<int64_t>(1, HIST_CELLS / k);
  p.nslab = (int)std::max<int64_t>(1, std::min(by_rows, by_cells));
  p.slab = (n + p.nslab - 1) / p.nslab;
  p.nslab = (int)((n + p.slab - 1) / p.slab);
  p.nwork = (n + CHUNK - 1) / CHUNK + k;    // sum_c ceil(count_c / CHUNK) never exceeds it
  const int64_t q0 = std::min<int64_t>(n, QCHUNK), q1 = n % QCHUNK;
  size_t vs = kp2d_vpr_scratch_bytes((int)q0, k, dim, 1);
  if (q1 > 0) vs = std::max(vs, kp2d_vpr_scratch_bytes((int)q1, k, dim, 1));
  Carve c(scratch);
  p.cpack = c.take<unsigned char>(kp2d_vpr_packed_bytes(k, dim));
  p.vpr = c.take<unsigned char>(vs);
  p.hist = c.take<int>((size_t)p.nslab * k);
  p.start = c.take<int>((size_t)k + 1);
  p.cstart = c.take<int>((size_t)k + 1);
  p.rcount = c.take<int>(k);
  p.elist = c.take<int>(k);
  p.meta = c.take<int>(4);
  p.order = c.take<int>(n);
  p.part = c.take<float>((size_t)p.nwork * dim);
  p.c0 = c.take<float>((size_t)k * dim);
  p.c1 = c.take<float>((size_t)k * dim);
  p.total = c.bytes();
  return p;
}

__global__ __launch_bounds__(256) void km_hist_kernel(const int64_t* __restrict__ assign, int64_t n, int64_t slab, int k,
                                                      int* __restrict__ hist) {
  const int64_t r0 = (int64_t)blockIdx.x * slab, r1 = min(n, r0 + slab);
  int* h = hist + (size_t)blockIdx.x * k;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
    const int64_t a = assign[r];
    if (a >= 0 && a < k) atomicAdd(h + a, 1);
  }
}

__global__ __launch_bounds__(256) void km_colscan_kernel(int* __restrict__ hist, int nslab, int k, int* __restrict__ rcount,
                                                         int64_t* __restrict__ counts) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= k) return;
  int run = 0;
  for (int s = 0; s < nslab; ++s) {
    const int v = hist[(size_t)s * k + c];
    hist[(size_t)s * k + c] = run;
    run += v;
  }
  rcount[c] = run;
  counts[c] = run;
}

// exclusive scan of one int per thread over the SB threads of the workgroup; *total = the sum
__device__ inline int block_excl_scan(int v, int* s, int* total) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
  for (int o = 1; o < SB; o <<= 1) {
    const int add = t >= o ? s[t - o] : 0;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  *total = s[SB - 1];
  return s[t] - v;
}

__global__ __launch_bounds__(SB) void km_scan_kernel(const int* __restrict__ rcount, int k, int* __restrict__ start,
                                                     int* __restrict__ cstart, int* __restrict__ elist, int* __restrict__ meta,
                                                     const float* __restrict__ dist, const int64_t* __restrict__ assign, int64_t n,
                                                     float* __restrict__ obj) {
  __shared__ int s[SB];
  __shared__ double sd[SB];
  const int t = threadIdx.x;
  const int seg = (k + SB - 1) / SB, c0 = min(k, t * seg), c1 = min(k, c0 + seg);
  int rows = 0, chunks = 0, empties = 0;
  for (int c = c0; c < c1; ++c) {
    const int m = rcount[c];
    rows += m;
    chunks += (m + CHUNK - 1) / CHUNK;
    empties += m == 0;
  }
  int trows, tchunks, tempty;
  int r = block_excl_scan(rows, s, &trows);
  int ch = block_excl_scan(chunks, s, &tchunks);
  int e = block_excl_scan(empties, s, &tempty);
  for (int c = c0; c < c1; ++c) {
    const int m = rcount[c];
    start[c] = r;
    cstart[c] = ch;
    if (m == 0) elist[e++] = c;
    r += m;
    ch += (m + CHUNK - 1) / CHUNK;
  }
  if (t == 0) {
    start[k] = trows;
    cstart[k] = tchunks;
    meta[0] = tempty;
  }
  // the objective: thread t adds rows t, t + SB, ... in order, then a fixed tree; double, so the order costs no accuracy
  double acc = 0.0;
  for (int64_t i = t; i < n; i += SB)
    if (assign[i] >= 0) acc += (double)dist[i];
  sd[t] = acc;
  __syncthreads();
  for (int o = SB / 2; o > 0; o >>= 1) {
    if (t < o) sd[t] += sd[t + o];
    __syncthreads();
  }
  if (t == 0) obj[0] = (float)sd[0];
}

__global__ __launch_bounds__(64) void km_scatter_kernel(const int64_t* __restrict__ assign, int64_t n, int64_t slab, int k,
                                                        int* __restrict__ hist, const int* __restrict__ start,
                                                        int* __restrict__ order) {
  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * slab, r1 = min(n, r0 + slab);
  int* cursor = hist + (size_t)blockIdx.x * k;        // this slab's running offsets: touched by this wave alone
  for (int64_t base = r0; base < r1; base += 64) {
    const int64_t row = base + lane;
    int key = -1;
    if (row < r1) {
      const int64_t a = assign[row];
      if (a >= 0 && a < k) key = (int)a;
    }
    int rank = 0, same = 0, lead = 64;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
      const int kj = __builtin_amdgcn_readlane(key, j);
      const bool eq = kj == key;
      rank += (eq && j < lane) ? 1 : 0;
      same += eq ? 1 : 0;
      lead = (eq && j < lead) ? j : lead;
    }
    int pos = 0;
    if (key >= 0 && lead == lane) pos = start[key] + atomicAdd(cursor + key, same);
    pos = __shfl(pos, lead & 63);
    const int64_t at = (int64_t)pos + rank;
    if (key >= 0 && at < n) order[at] = (int)row;
  }
}

__device__ inline float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

__global__ __launch_bounds__(64) void km_sum_kernel(const float* __restrict__ x, int dim, int k, const int* __restrict__ start,
                                                    const int* __restrict__ cstart, const int* __restrict__ order,
                                                    float* __restrict__ part) {
  const int w = blockIdx.x, lane = threadIdx.x;
  if (w >= cstart[k]) return;
  int lo = 0, hi = k;                                  // the cluster of work item w: cstart[lo] <= w < cstart[lo + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cstart[mid] <= w) lo = mid; else hi = mid;
  }
  const int c = lo;
  const int r0 = start[c] + (w - cstart[c]) * CHUNK;
  const int cnt = min(CHUNK, start[c + 1] - r0);
  const int ncol = dim >> 2;                           // float4 columns of a row
  int cw = 4;                                          // lanes per row group: the power of two >= min(ncol, 64)
  while (cw < ncol && cw < 64) cw <<= 1;
  const int G = 64 / cw, g = lane / cw, cl = lane - g * cw;
  const int* ord = order + r0;
  for (int cb = 0; cb < ncol; cb += cw) {
    const int col = cb + cl;
    const bool live = col < ncol;
    float4 acc[UNR];
#pragma unroll
    for (int a = 0; a < UNR; ++a) acc[a] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live)
      for (int j0 = 0; g + G * j0 < cnt; j0 += UNR) {
#pragma unroll
        for (int a = 0; a < UNR; ++a) {
          const int r = g + G * (j0 + a);
          if (r < cnt) acc[a] = add4(acc[a], *reinterpret_cast<const float4*>(x + (size_t)ord[r] * dim + (size_t)col * 4));
        }
      }
    float4 s = add4(add4(add4(acc[0], acc[1]), add4(acc[2], acc[3])), add4(add4(acc[4], acc[5]), add4(acc[6], acc[7])));
    for (int o = cw; o < 64; o <<= 1) {                // groups g and g ^ (o / cw): both lanes get the same sum
      s.x += __shfl_xor(s.x, o);
      s.y += __shfl_xor(s.y, o);
      s.z += __shfl_xor(s.z, o);
      s.w += __shfl_xor(s.w, o);
    }
    if (live && g == 0) *reinterpret_cast<float4*>(part + (size_t)w * dim + (size_t)col * 4) = s;
  }
}

__global__ __launch_bounds__(64) void km_update_kernel(const float* __restrict__ part, const float* __restrict__ cin, int dim,
                                                       const int* __restrict__ start, const int* __restrict__ cstart,
                                                       float* __restrict__ cout) {
  const int c = blockIdx.x;
  const int m = start[c + 1] - start[c];
  const int w0 = cstart[c], nch = cstart[c + 1] - w0;
  const float inv = m > 0 ? 1.f / (float)m : 0.f;
  for (int col = threadIdx.x; col < (dim >> 2); col += 64) {
    const size_t at = (size_t)col * 4;
    float4 v;
    if (m == 0) {
      v = *reinterpret_cast<const float4*>(cin + (size_t)c * dim + at);
    } else {
      float4 s = *reinterpret_cast<const float4*>(part + (size_t)w0 * dim + at);
      for (int i = 1; i < nch; ++i) s = add4(s, *reinterpret_cast<const float4*>(part + (size_t)(w0 + i) * dim + at));
      v = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
    }
    *reinterpret_cast<float4*>(cout + (size_t)c * dim + at) = v;
  }
}

__host__ __device__ inline uint64_t km_draw(uint64_t seed, int iteration, int ci) {
  return km_mix(km_mix(seed + 0x9E3779B97F4A7C15ull) ^ (((uint64_t)(uint32_t)iteration << 32) | (uint32_t)ci));
}

__global__ __launch_bounds__(SB) void km_split_kernel(float* __restrict__ cout, int dim, int k, int* __restrict__ rcount,
                                                      const int* __restrict__ elist, const int* __restrict__ meta, uint64_t seed,
                                                      int iteration) {
  __shared__ int s[SB];
  __shared__ int s_cj;
  const int t = threadIdx.x;
  const int nempty = meta[0];
  if (nempty == 0) return;
  const int seg = (k + SB - 1) / SB, c0 = min(k, t * seg), c1 = min(k, c0 + seg);
  for (int e = 0; e < nempty; ++e) {
    const int ci = elist[e];
    int wsum = 0;                                      // this thread's share of sum_j max(count_j - 1, 0)
    for (int c = c0; c < c1; ++c) wsum += max(rcount[c] - 1, 0);
    int total;
    const int before = block_excl_scan(wsum, s, &total);
    if (total <= 0) return;                            // no cluster has two points left to give: the rest keep their input
    const int r = (int)(km_draw(seed, iteration, ci) % (uint64_t)total);
    if (r >= before && r < before + wsum) {
      int run = before, cj = c0;
      for (int c = c0; c < c1; ++c) {
        const int wgt = max(rcount[c] - 1, 0);
        if (r < run + wgt) { cj = c; break; }
        run += wgt;
      }
      s_cj = cj;
    }
    __syncthreads();
    const int cj = s_cj;
    for (int j = t; j < dim; j += SB) {
      const float v = cout[(size_t)cj * dim + j];
      const float up = v * (1.f + SPLIT_EPS), dn = v * (1.f - SPLIT_EPS);
      cout[(size_t)ci * dim + j] = (j & 1) ? dn : up;
      cout[(size_t)cj * dim + j] = (j & 1) ? up : dn;
    }
    if (t == 0) {
      const int half = rcount[cj] / 2;
      rcount[ci] = half;
      rcount[cj] -= half;
    }
    __syncthreads();                                   // centroids and running counts are written: the next empty cluster may read
  }
}

__global__ __launch_bounds__(64) void km_normalize_kernel(float* __restrict__ c, int dim) {
  float* row = c + (size_t)blockIdx.x * dim;
  float acc = 0.f;
  for (int j = threadIdx.x; j < dim; j += 64) acc = fmaf(row[j], row[j], acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  const float nrm = sqrtf(acc);
  if (nrm > 0.f) {
    const float inv = 1.f / nrm;
    for (int j = threadIdx.x; j < dim; j += 64) row[j] *= inv;
  }
}

int check_shape(const char* who, int64_t n, int dim, int k) {
  if (dim < 16 || dim > 16384 || dim % 16) return fail(KP2D_ERR_UNSUPPORTED, "%s: dim %d (needs dim %% 16 == 0, 16 <= dim <= 16384)", who, dim);
  if (k < 1 || k > 65536) return fail(KP2D_ERR_ARG, "%s: k = %d outside [1, 65536]", who, k);
  if (n < k) return fail(KP2D_ERR_ARG, "%s: n = %lld points for k = %d centroids", who, (long long)n, k);
  if (n > INT32_MAX) return fail(KP2D_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 points", who);
  return KP2D_OK;
}

// one Lloyd iteration, enqueued on st; arguments are checked by the callers
int step(const float* x, int64_t n, int dim, const float* cin, int k, uint32_t flags, uint64_t seed, int iteration, float* cout,
         int64_t* assign, float* dist, int64_t* counts, float* obj, const KmPlan& p, hipStream_t st) {
  // a. assign: the flat index's own search, k = 1, the centroids as the database
  if (int e = launch_vpr_pack(cin, k, dim, p.cpack, st)) return fail(KP2D_ERR_HIP, "kmeans: pack kernel: %d", e);
  for (int64_t q0 = 0; q0 < n; q0 += QCHUNK) {
    VprSearchArgs a{};
    a.dbp = p.cpack;
    a.db = cin;
    a.q = x + q0 * dim;
    a.limit = nullptr;
    a.ndb = k;
    a.dim = dim;
    a.nq = (int)std::min<int64_t>(QCHUNK, n - q0);
    a.k = 1;
    a.fp32 = (flags & KP2D_VPR_FP32) ? 1 : 0;
    if (int e = launch_vpr_search(a, p.vpr, dist + q0, assign + q0, st)) return fail(KP2D_ERR_HIP, "kmeans: search kernels: %d", e);
  }
  // b. inverted index by a stable counting sort, then the per-cluster sums
  HIP_TRY(hipMemsetAsync(p.hist, 0, (size_t)p.nslab * k * 4, st));
  hipLaunchKernelGGL(km_hist_kernel, dim3(p.nslab), dim3(256), 0, st, assign, n, p.slab, k, p.hist);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(km_colscan_kernel, dim3((k + 255) / 256), dim3(256), 0, st, p.hist, p.nslab, k, p.rcount, counts);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(SB), 0, st, p.rcount, k, p.start, p.cstart, p.elist, p.meta, dist, assign, n, obj);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(km_scatter_kernel, dim3(p.nslab), dim3(64), 0, st, assign, n, p.slab, k, p.hist, p.start, p.order);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(km_sum_kernel, dim3((unsigned)p.nwork), dim3(64), 0, st, x, dim, k, p.start, p.cstart, p.order, p.part);
  HIP_TRY(hipGetLastError());
  // c. update
  hipLaunchKernelGGL(km_update_kernel, dim3(k), dim3(64), 0, st, p.part, cin, dim, p.start, p.cstart, cout);
  HIP_TRY(hipGetLastError());
  if (!(flags & KP2D_KMEANS_NO_SPLIT)) {
    hipLaunchKernelGGL(km_split_kernel, dim3(1), dim3(SB), 0, st, cout, dim, k, p.rcount, p.elist, p.meta, seed, iteration);
    HIP_TRY(hipGetLastError());
  }
  if (flags & KP2D_KMEANS_SPHERICAL) {
    hipLaunchKernelGGL(km_normalize_kernel, dim3(k), dim3(64), 0, st, cout, dim);
    HIP_TRY(hipGetLastError());
  }
  return KP2D_OK;
}

constexpr uint32_t KNOWN_FLAGS = KP2D_VPR_FP32 | KP2D_KMEANS_SPHERICAL | KP2D_KMEANS_NO_SPLIT;

}  // namespace

extern "C" {

size_t kp2d_kmeans_scratch_bytes(int64_t n, int dim, int k) {
  if (dim < 16 || dim > 16384 || dim % 16 || k < 1 || k > 65536 || n < k || n > INT32_MAX) return 0;
  return km_plan(nullptr, n, dim, k).total;
}

int kp2d_kmeans_step(const float* x, int64_t n, int dim, const float* centroids_in, int k, uint32_t flags, uint64_t seed,
                     int iteration, float* centroids_out, int64_t* assign, float* dist, int64_t* counts, float* obj,
                     void* scratch, size_t scratch_bytes, void* stream) {
  if (int e = check_shape("kmeans_step", n, dim, k)) return e;
  if (flags & ~KNOWN_FLAGS) return fail(KP2D_ERR_ARG, "unknown kmeans flags 0x%x", flags);
  if (iteration < 0) return fail(KP2D_ERR_ARG, "kmeans_step: iteration %d", iteration);
  if (!x || !centroids_in || !centroids_out || !assign || !dist || !counts || !obj || !scratch) return fail(KP2D_ERR_ARG, "null argument");
  if (centroids_in == centroids_out) return fail(KP2D_ERR_ARG, "kmeans_step: centroids_in and centroids_out must differ");
  if ((uintptr_t)x % 16 || (uintptr_t)centroids_in % 16 || (uintptr_t)centroids_out % 16 || (uintptr_t)scratch % 16)
    return fail(KP2D_ERR_ARG, "kmeans_step: x, centroids and scratch must be 16-byte aligned");
  const KmPlan p = km_plan(scratch, n, dim, k);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_WORKSPACE, "kmeans scratch %zu B < required %zu B (kp2d_kmeans_scratch_bytes)", scratch_bytes, p.total);
  DeviceGuard guard(x, (hipStream_t)stream);
  return step(x, n, dim, centroids_in, k, flags, seed, iteration, centroids_out, assign, dist, counts, obj, p, (hipStream_t)stream);
}

int kp2d_kmeans_train(const float* x, int64_t n, int dim, float* centroids, int k, int niter, uint32_t flags, uint64_t seed,
                      float* obj, int64_t* assign, float* dist, int64_t* counts, void* scratch, size_t scratch_bytes,
                      void* stream) {
  if (int e = check_shape("kmeans_train", n, dim, k)) return e;
  if (niter < 1) return fail(KP2D_ERR_ARG, "kmeans_train: niter = %d", niter);
  if (flags & ~KNOWN_FLAGS) return fail(KP2D_ERR_ARG, "unknown kmeans flags 0x%x", flags);
  if (!x || !centroids || !assign || !dist || !counts || !obj || !scratch) return fail(KP2D_ERR_ARG, "null argument");
  if ((uintptr_t)x % 16 || (uintptr_t)centroids % 16 || (uintptr_t)scratch % 16)
    return fail(KP2D_ERR_ARG, "kmeans_train: x, centroids and scratch must be 16-byte aligned");
  const KmPlan p = km_plan(scratch, n, dim, k);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_WORKSPACE, "kmeans scratch %zu B < required %zu B (kp2d_kmeans_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  float* buf[2] = {p.c0, p.c1};
  const float* cur = centroids;                        // iteration i: cur -> buf[i & 1]
  for (int i = 0; i < niter; ++i) {
    if (int e = step(x, n, dim, cur, k, flags, seed, i, buf[i & 1], assign, dist, counts, obj + i, p, st)) return e;
    cur = buf[i & 1];
  }
  HIP_TRY(hipMemcpyAsync(centroids, cur, (size_t)k * dim * 4, hipMemcpyDeviceToDevice, st));
  return KP2D_OK;
}

}  // extern "C"
