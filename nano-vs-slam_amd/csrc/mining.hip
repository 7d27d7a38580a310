// Triplet mining on the device (kp2d_geo_radius_mask, kp2d_mask_lists, kp2d_vpr_mine; include/kp2d.h): what the
// reference's dataset classes do with sklearn.neighbors.NearestNeighbors on the host (src/data/pittsburgh.py:189-200,
// :258-333) for descriptors this library has just computed.  Both jobs are searches over a per-query subset of the
// database rows, so everything here is built on row masks (uint32 words, [nq, W], W = ceil(ndb / 32), row r = bit r & 31
// of word r >> 5) and on the masked instantiation of the flat index's search (vpr.hip).
// Kernels:
//   geo_mask_kernel     one workgroup per query walks the database positions 256 rows at a time; a wave's 64-bit ballot
//                       is two mask words, written by its lane 0 (one writer per word, no atomics); float64, no FMA
//   mask_lists_kernel   one wave per query: popcounts of 64 words, a wave scan, every lane writes the rows of its word
//   mine_cand_kernel    one workgroup per query: cache rows and the n_sample counter-based draws -> candidate mask.
//                       Popcount prefix sums over groups of G words in LDS (G = 1 up to 131072 rows), a binary search
//                       over the prefix, then the rank-th set bit inside the group; bits set with integer atomicOr
//   mine_select_kernel  one thread per query: the violators (a prefix of the ascending list) in float64
// The two searches of a round are launch_vpr_search with a mask (k = 1 over the positives, k = n_neg n_neg_factor over
// the candidates) on one shared search scratch.  No float atomics; nothing depends on the other queries of a call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "api_common.h"
#include "device_guard.h"
#include "kp2d_kernels.h"
#include "mix64.h"

using namespace kp2d;

namespace {

constexpr int PRE_MAX = 4096;               // prefix entries in LDS: groups of G = ceil(W / PRE_MAX) words

__host__ __device__ inline int64_t mask_words(int64_t ndb) { return (ndb + 31) >> 5; }

// word w of a mask row with the bits at or past ndb cleared
__device__ inline uint32_t live_word(const uint32_t* row, int64_t w, int64_t ndb) {
  uint32_t v = row[w];
  const int64_t left = ndb - (w << 5);
  if (left < 32) v &= (1u << (int)left) - 1u;
  return v;
}

// dx dx + dy dy <= r2 with every operation rounded on its own (sklearn's closed ball in float64)
__device__ inline bool inside(double dx, double dy, double r2) {
#pragma clang fp contract(off)
  const double a = dx * dx;
  const double b = dy * dy;
  const double s = a + b;
  return s <= r2;
}

__global__ __launch_bounds__(256) void geo_mask_kernel(const double* __restrict__ db, int64_t ndb, const double* __restrict__ q,
                                                       double r2, int invert, uint32_t* __restrict__ mask,
                                                       int32_t* __restrict__ count) {
  __shared__ int s_cnt[4];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double qx = q[2 * (int64_t)i], qy = q[2 * (int64_t)i + 1];
  const int64_t W = mask_words(ndb);
  uint32_t* row = mask + (int64_t)i * W;
  int cnt = 0;                                // lane 0 of each wave counts the wave's rows
  for (int64_t base = 0; base < ndb; base += 256) {
    const int64_t r = base + tid;
    bool in = false;
    if (r < ndb) {
      in = inside(db[2 * r] - qx, db[2 * r + 1] - qy, r2) != (invert != 0);
    }
    const unsigned long long b = __ballot(in);
    if (lane == 0) {
      const int64_t w = (base >> 5) + wave * 2;
      if (w < W) row[w] = (uint32_t)b;
      if (w + 1 < W) row[w + 1] = (uint32_t)(b >> 32);
      cnt += __popcll(b);
    }
  }
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (tid == 0) count[i] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(64) void mask_lists_kernel(const uint32_t* __restrict__ mask, int64_t ndb,
                                                        const int64_t* __restrict__ lims, int64_t* __restrict__ idx,
                                                        int64_t idx_len, int32_t* __restrict__ status) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const int64_t W = mask_words(ndb);
  const uint32_t* row = mask + (int64_t)i * W;
  const int64_t lo = lims[i], hi = lims[i + 1];
  int64_t run = 0;                            // rows of the words before this pass
  for (int64_t w0 = 0; w0 < W; w0 += 64) {
    const int64_t w = w0 + lane;
    uint32_t v = w < W ? live_word(row, w, ndb) : 0u;
    const int pc = __popc(v);
    int incl = pc;                            // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    int64_t at = lo + run + (incl - pc);
    while (v) {
      const int b = __ffs(v) - 1;
      v &= v - 1;
      if (at >= lo && at < hi && at >= 0 && at < idx_len) idx[at] = (w << 5) + b;
      ++at;
    }
    run += __shfl(incl, 63);
  }
  if (lane == 0 && (lo < 0 || hi < lo || hi > idx_len || run != hi - lo)) atomicOr(status, 1);
}

__host__ __device__ inline uint64_t mine_draw(uint64_t seed, int round, int i, int j) {
  return km_mix(km_mix(km_mix(seed + 0x9E3779B97F4A7C15ull) ^ (((uint64_t)(uint32_t)round << 32) | (uint32_t)i)) ^ (uint64_t)(uint32_t)j);
}

__global__ __launch_bounds__(256) void mine_cand_kernel(const uint32_t* __restrict__ neg_mask, const int32_t* __restrict__ cache,
                                                        const int32_t* __restrict__ qid, int64_t ndb, int n_sample,
                                                        int n_neg, uint64_t seed, int round, uint32_t* __restrict__ cand) {
  __shared__ int s_pre[PRE_MAX + 1];          // exclusive prefix of the groups' popcounts; s_pre[NG] = nPot
  __shared__ int s_tot[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int id = qid ? qid[i] : i;            // the query's number in the draws: its own, wherever it stands in the call
  const int64_t W = mask_words(ndb);
  const uint32_t* row = neg_mask + (int64_t)i * W;
  uint32_t* out = cand + (int64_t)i * W;      // zeroed before the launch
  if (cache)
    for (int j = tid; j < n_neg; j += 256) {
      const int r = cache[(int64_t)i * n_neg + j];
      if (r >= 0 && r < ndb) atomicOr(out + (r >> 5), 1u << (r & 31));
    }
  if (n_sample <= 0) return;
  const int G = (int)((W + PRE_MAX - 1) / PRE_MAX);            // words per group
  const int NG = (int)((W + G - 1) / G);                       // groups: at most PRE_MAX
  const int seg = (NG + 255) / 256, g0 = min(NG, tid * seg), g1 = min(NG, g0 + seg);
  int mine = 0;
  for (int g = g0; g < g1; ++g) {
    int c = 0;
    const int64_t wa = (int64_t)g * G, wb = min(W, wa + G);
    for (int64_t w = wa; w < wb; ++w) c += __popc(live_word(row, w, ndb));
    s_pre[g] = c;
    mine += c;
  }
  s_tot[tid] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {         // inclusive scan of the threads' totals
    const int add = tid >= o ? s_tot[tid - o] : 0;
    __syncthreads();
    s_tot[tid] += add;
    __syncthreads();
  }
  int run = s_tot[tid] - mine;
  for (int g = g0; g < g1; ++g) {
    const int c = s_pre[g];
    s_pre[g] = run;
    run += c;
  }
  if (tid == 255) s_pre[NG] = s_tot[255];
  __syncthreads();
  const int npot = s_pre[NG];
  if (npot <= 0) return;                      // nothing to draw from: the cache rows alone
  for (int j = tid; j < n_sample; j += 256) {
    int u = (int)(mine_draw(seed, round, id, j) % (uint64_t)npot);
    int lo = 0, hi = NG;                      // the group holding rank u: s_pre[lo] <= u < s_pre[lo + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_pre[mid] <= u) lo = mid; else hi = mid;
    }
    u -= s_pre[lo];
    const int64_t wa = (int64_t)lo * G, wb = min(W, wa + G);
    for (int64_t w = wa; w < wb; ++w) {
      uint32_t v = live_word(row, w, ndb);
      const int pc = __popc(v);
      if (u >= pc) { u -= pc; continue; }
      for (; u > 0; --u) v &= v - 1;          // drop the u lowest set bits
      const int b = __ffs(v) - 1;
      atomicOr(out + w, 1u << b);
      break;
    }
  }
}

__global__ __launch_bounds__(256) void mine_select_kernel(const int64_t* __restrict__ pos_idx, const float* __restrict__ dpos2,
                                                          const float* __restrict__ dneg2, const int64_t* __restrict__ ineg,
                                                          int nq, int K, int n_neg, float margin, int32_t* __restrict__ neg_idx,
                                                          int32_t* __restrict__ neg_cnt, float* __restrict__ d_pos) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nq) return;
  int32_t* o = neg_idx + (int64_t)i * n_neg;
  int n = 0;
  if (pos_idx[i] < 0) {
    d_pos[i] = __builtin_nanf("");
  } else {
    const double dp = sqrt((double)dpos2[i]);
    const double thr = dp + sqrt((double)margin);
    d_pos[i] = (float)dp;
    const float* dn = dneg2 + (int64_t)i * K;
    const int64_t* in = ineg + (int64_t)i * K;
    for (int j = 0; j < K && n < n_neg; ++j) {
      if (in[j] < 0 || !(sqrt((double)dn[j]) < thr)) break;    // ascending: the violators are a prefix
      o[n++] = (int32_t)in[j];
    }
  }
  neg_cnt[i] = n;
  for (int j = n; j < n_neg; ++j) o[j] = -1;
}

// scratch of a mining round as one walk: the candidate masks, the two searches' outputs and the search scratch they share
struct MinePlan {
  uint32_t* cand;
  float *dpos2, *dneg2;
  int64_t* ineg;
  unsigned char* vpr;
  size_t total;
};

MinePlan mine_plan(void* scratch, int nq, int64_t ndb, int dim, int K) {
  MinePlan p{};
  Carve c(scratch);
  p.cand = c.take<uint32_t>((size_t)nq * mask_words(ndb));
  p.dpos2 = c.take<float>(nq);
  p.dneg2 = c.take<float>((size_t)nq * K);
  p.ineg = c.take<int64_t>((size_t)nq * K);
  p.vpr = c.take<unsigned char>(std::max(kp2d_vpr_scratch_bytes(nq, ndb, dim, 1), kp2d_vpr_scratch_bytes(nq, ndb, dim, K)));
  p.total = c.bytes();
  return p;
}

bool dim_ok(int dim) { return dim >= 16 && dim <= 16384 && dim % 16 == 0; }

}  // namespace

extern "C" {

int kp2d_geo_radius_mask(const double* db_xy, int64_t ndb, const double* q_xy, int nq, double radius, uint32_t flags,
                         uint32_t* mask, int32_t* count, void* stream) {
  if (nq < 0 || ndb < 0) return fail(KP2D_ERR_ARG, "geo_radius_mask: negative size");
  if (ndb > INT32_MAX) return fail(KP2D_ERR_UNSUPPORTED, "geo_radius_mask: more than 2^31 - 1 database rows");
  if (!(radius >= 0.0)) return fail(KP2D_ERR_ARG, "geo_radius_mask: radius %g", radius);
  if (flags & ~(uint32_t)KP2D_GEO_INVERT) return fail(KP2D_ERR_ARG, "unknown geo flags 0x%x", flags);
  if (nq == 0) return KP2D_OK;
  if (!q_xy || !count || (ndb > 0 && (!db_xy || !mask))) return fail(KP2D_ERR_ARG, "null argument");
  if ((uintptr_t)db_xy % 8 || (uintptr_t)q_xy % 8 || (uintptr_t)mask % 4 || (uintptr_t)count % 4)
    return fail(KP2D_ERR_ARG, "geo_radius_mask: positions must be 8-byte aligned, mask and count 4-byte");
  DeviceGuard guard(q_xy, (hipStream_t)stream);
  hipLaunchKernelGGL(geo_mask_kernel, dim3(nq), dim3(256), 0, (hipStream_t)stream, db_xy, ndb, q_xy, radius * radius,
                     (flags & KP2D_GEO_INVERT) ? 1 : 0, mask, count);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_mask_lists(const uint32_t* mask, int nq, int64_t ndb, const int64_t* lims, int64_t* idx, int64_t idx_len,
                    int32_t* status, void* stream) {
  if (nq < 0 || ndb < 0 || idx_len < 0) return fail(KP2D_ERR_ARG, "mask_lists: negative size");
  if (ndb > INT32_MAX) return fail(KP2D_ERR_UNSUPPORTED, "mask_lists: more than 2^31 - 1 database rows");
  if (nq == 0) return KP2D_OK;
  if (!lims || !status || (ndb > 0 && !mask) || (idx_len > 0 && !idx)) return fail(KP2D_ERR_ARG, "null argument");
  if ((uintptr_t)mask % 4 || (uintptr_t)lims % 8 || (uintptr_t)idx % 8 || (uintptr_t)status % 4)
    return fail(KP2D_ERR_ARG, "mask_lists: mask and status must be 4-byte aligned, lims and idx 8-byte");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(lims, st);
  HIP_TRY(hipMemsetAsync(status, 0, 4, st));
  hipLaunchKernelGGL(mask_lists_kernel, dim3(nq), dim3(64), 0, st, mask, ndb, lims, idx, idx_len, status);
  HIP_TRY(hipGetLastError());
  int32_t bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, status, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (bad) return fail(KP2D_ERR_ARG, "mask_lists: a query's number of set bits disagrees with its span of lims");
  return KP2D_OK;
}

size_t kp2d_vpr_mine_scratch_bytes(int nq, int64_t ndb, int dim, int n_neg, int n_neg_factor) {
  if (nq < 1 || ndb < 0 || ndb > INT32_MAX || !dim_ok(dim) || n_neg < 1 || n_neg_factor < 1 ||
      (int64_t)n_neg * n_neg_factor > 1024)
    return 0;
  return mine_plan(nullptr, nq, ndb, dim, n_neg * n_neg_factor).total;
}

int kp2d_vpr_mine(const void* packed_db, const float* db, int64_t ndb, int dim, const float* q, int nq,
                  const int32_t* qid, const uint32_t* pos_mask, const uint32_t* neg_mask, const int32_t* neg_cache,
                  int n_sample, int n_neg, int n_neg_factor, float margin, uint64_t seed, int round, uint32_t flags,
                  int64_t* pos_idx, int32_t* neg_idx, int32_t* neg_cnt, float* d_pos, uint32_t* cand_mask, void* scratch,
                  size_t scratch_bytes, void* stream) {
  if (!dim_ok(dim)) return fail(KP2D_ERR_UNSUPPORTED, "vpr_mine: descriptor dim %d (needs dim %% 16 == 0, 16 <= dim <= 16384)", dim);
  if (nq < 0 || ndb < 0) return fail(KP2D_ERR_ARG, "vpr_mine: negative size");
  if (ndb > INT32_MAX) return fail(KP2D_ERR_UNSUPPORTED, "vpr_mine: more than 2^31 - 1 database rows");
  if (n_neg < 1 || n_neg_factor < 1 || (int64_t)n_neg * n_neg_factor > 1024)
    return fail(KP2D_ERR_ARG, "vpr_mine: n_neg * n_neg_factor = %lld outside [1, 1024]", (long long)n_neg * n_neg_factor);
  if (n_sample < 0 || round < 0 || !(margin >= 0.f)) return fail(KP2D_ERR_ARG, "vpr_mine: n_sample %d, round %d, margin %g", n_sample, round, (double)margin);
  if (flags & ~(uint32_t)KP2D_VPR_FP32) return fail(KP2D_ERR_ARG, "unknown vpr flags 0x%x", flags);
  if (nq == 0) return KP2D_OK;
  if (!q || !pos_idx || !neg_idx || !neg_cnt || !d_pos || !scratch || (ndb > 0 && (!packed_db || !db || !pos_mask || !neg_mask)))
    return fail(KP2D_ERR_ARG, "null argument");
  if ((uintptr_t)q % 16 || (uintptr_t)db % 16 || (uintptr_t)packed_db % 16 || (uintptr_t)scratch % 16)
    return fail(KP2D_ERR_ARG, "vpr_mine: q, db, packed_db and scratch must be 16-byte aligned");
  if ((uintptr_t)pos_mask % 4 || (uintptr_t)neg_mask % 4 || (uintptr_t)neg_cache % 4 || (uintptr_t)cand_mask % 4 || (uintptr_t)qid % 4 ||
      (uintptr_t)neg_idx % 4 || (uintptr_t)neg_cnt % 4 || (uintptr_t)d_pos % 4 || (uintptr_t)pos_idx % 8)
    return fail(KP2D_ERR_ARG, "vpr_mine: masks, qid, neg_cache, neg_idx, neg_cnt and d_pos must be 4-byte aligned, pos_idx 8-byte");
  const int K = n_neg * n_neg_factor;
  const MinePlan p = mine_plan(scratch, nq, ndb, dim, K);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_ARG, "vpr_mine scratch %zu B < required %zu B (kp2d_vpr_mine_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(q, st);
  const size_t mask_bytes = (size_t)nq * mask_words(ndb) * 4;
  uint32_t* cand = cand_mask ? cand_mask : p.cand;
  // a. candidates
  if (mask_bytes) {
    HIP_TRY(hipMemsetAsync(cand, 0, mask_bytes, st));
    hipLaunchKernelGGL(mine_cand_kernel, dim3(nq), dim3(256), 0, st, neg_mask, neg_cache, qid, ndb, n_sample, n_neg, seed, round, cand);
    HIP_TRY(hipGetLastError());
  }
  // b. the nearest positive, c. the K nearest candidates
  VprSearchArgs a{};
  a.dbp = static_cast<const unsigned char*>(packed_db);
  a.db = db; a.q = q; a.ndb = ndb; a.dim = dim; a.nq = nq;
  a.fp32 = (flags & KP2D_VPR_FP32) ? 1 : 0;
  a.mask = pos_mask; a.k = 1;
  if (int e = launch_vpr_search(a, p.vpr, p.dpos2, pos_idx, st)) return fail(KP2D_ERR_HIP, "vpr_mine: positive search kernels: %d", e);
  a.mask = cand; a.k = K;
  if (int e = launch_vpr_search(a, p.vpr, p.dneg2, p.ineg, st)) return fail(KP2D_ERR_HIP, "vpr_mine: negative search kernels: %d", e);
  // d. select
  hipLaunchKernelGGL(mine_select_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, pos_idx, p.dpos2, p.dneg2, p.ineg, nq, K, n_neg,
                     margin, neg_idx, neg_cnt, d_pos);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

}  // extern "C"
