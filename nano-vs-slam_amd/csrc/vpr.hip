// Place recognition on the device: exact brute-force squared-L2 top-k of query descriptors against a database of global
// descriptors (the `vlad` output).  Replaces the faiss.IndexFlatL2 search of the reference's evaluate_global_descriptor
// (src/evaluation/global_descriptor.py:55-60) without ever writing the Q x N distance matrix.
// Kernels:
//   vpr_pack_kernel    one row -> [meta 16 B: |x|^2, 2^-s, guard bit][hi: dim fp16 of x 2^s][lo: dim fp16 of x 2^s - hi]
//                      (the S16P idea of DESIGN.md §3: the two planes take the bytes of the fp32 row).  s is the row's own
//                      power of two, chosen so max|x| 2^s lies in [2^14, 2^15): hi is a normal fp16, lo stays above the
//                      fp16 subnormal floor for every element within 2^-14 of the row's largest, and the scale is exact.
//   vpr_search_kernel  64 queries x a slice of 128-row database tiles per workgroup.  Per tile: the 64 x 128 dot
//                      products over dim on the matrix cores (K loop through LDS in 32-element chunks, two LDS buffers
//                      filled by global_load_lds), key = |d|^2 - 2 q.d, then every query keeps its k best (key, row)
//                      of the slice in a list of the scratch.  Nothing Q x N is written.  vpr_search_kernel<true> is the
//                      masked form (kp2d_vpr_search_masked): a query sees the rows whose bit is set in its mask row, and
//                      a tile whose mask words are zero for all 64 queries is skipped before its products
//   vpr_merge_kernel   the k best of G slices' lists (bitonic sort in LDS), until one list per query is left
//   vpr_final_kernel   the k finalists re-scored as sum (q - d)^2 in fp32 (fixed order), sorted by (distance, row)
// Arithmetic of the key.  Default: split fp16, q.d = sum qh dh + qh dl + ql dh on v_mfma_f32_32x32x16_f16 with fp32
// accumulation (as knn2_mfma_kernel / the conv packs), undone by the two exact scales.  A database tile holding a row
// outside the range guard (a non-finite element, or max|x| outside [2^-40, 2^40)) is computed with exact fp32 products
// on v_mfma_f32_32x32x2_f32 instead; KP2D_VPR_FP32 takes that path for every tile.  Keys only rank: the finalists'
// distances come from the direct re-score, so near-duplicates (loop closures) get an accurate distance.
// Determinism: a key depends on its query, its row and its tile's mode only (tiles are fixed 128-row blocks of the
// database and slices are whole tiles), every reduction runs in a fixed order, and lists are cut by the total order of
// (key, row).  A query's answer is therefore bit-identical for any batch of queries and any number of slices.
// The entry points (kp2d_vpr_*, include/kp2d.h) are at the end of the file; kmeans.hip and mining.hip use the two launchers
// directly.
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <utility>

#include "api_common.h"
#include "device_guard.h"
#include "kp2d_kernels.h"

namespace kp2d {

namespace {

typedef _Float16 vh8 __attribute__((ext_vector_type(8)));
typedef float vf16 __attribute__((ext_vector_type(16)));

constexpr int QB = 64;                      // queries per workgroup (2 waves x 32)
constexpr int RB = 128;                     // database rows per tile (2 waves x 2 blocks x 32)
constexpr int KC = 32;                      // elements of dim per LDS chunk: 128 bytes of a row in either form
constexpr int CHB = 128;                    // bytes of one row's chunk
constexpr int STAGE = (RB + QB) * CHB;      // one LDS buffer: 24 KB
constexpr int KP = RB + 1;                  // pitch (floats) of the key tile, which reuses the staging buffers
constexpr int OFF_N2 = 2 * STAGE, OFF_DU = OFF_N2 + RB * 4, OFF_LIM = OFF_DU + RB * 4;
constexpr int SMEM = OFF_LIM + 16;
constexpr int MERGE_CAND = 2048;            // candidates one merge workgroup sorts
constexpr int TARGET_WGS = 768;             // three search workgroups per CU
constexpr unsigned long long EMPTY = ~0ull;
static_assert(QB * KP * 4 <= 2 * STAGE, "key tile must fit the staging buffers");

__host__ __device__ inline size_t row_bytes(int dim) { return (size_t)dim * 4 + 16; }

// float -> unsigned with the same order (negative keys are common: |d|^2 - 2 q.d)
__device__ inline unsigned fkey(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float fdec(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

__device__ inline void glds16(const void* src, unsigned char* lds) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}

// ascending bitonic sort of P (power of two) codes in LDS by the whole workgroup
__device__ void bitonic(unsigned long long* s, int P) {
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < P / 2; i += blockDim.x) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const unsigned long long x = s[lo], y = s[hi];
        if ((x > y) == asc) { s[lo] = y; s[hi] = x; }
      }
    }
  __syncthreads();
}

__global__ __launch_bounds__(256) void vpr_pack_kernel(const float* __restrict__ x, int dim, unsigned char* __restrict__ out) {
  __shared__ float s_n2[256], s_mx[256];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* xr = x + row * dim;
  float n2 = 0.f, mx = 0.f;
  int fin = 1;
  for (int c = tid; c < dim; c += 256) {
    const float v = xr[c];
    n2 = fmaf(v, v, n2);
    mx = fmaxf(mx, fabsf(v));
    fin &= isfinite(v) ? 1 : 0;
  }
  s_n2[tid] = n2;
  s_mx[tid] = mx;
  fin = __syncthreads_and(fin);
  for (int o = 128; o > 0; o >>= 1) {          // fixed tree: |x|^2 depends on the row alone
    if (tid < o) { s_n2[tid] += s_n2[tid + o]; s_mx[tid] = fmaxf(s_mx[tid], s_mx[tid + o]); }
    __syncthreads();
  }
  mx = s_mx[0];
  const int e = mx > 0.f ? ilogbf(mx) : 0;
  const int sh = min(125, max(-125, 14 - e));
  const float scale = ldexpf(1.f, sh);
  const bool safe = fin && (mx == 0.f || (e >= -40 && e < 40));
  unsigned char* o = out + (size_t)row * row_bytes(dim);
  if (tid == 0) *reinterpret_cast<float4*>(o) = make_float4(s_n2[0], ldexpf(1.f, -sh), safe ? 1.f : 0.f, 0.f);
  _Float16* hi = reinterpret_cast<_Float16*>(o + 16);
  _Float16* lo = hi + dim;
  for (int c = tid; c < dim; c += 256) {
    const float v = xr[c] * scale;            // exact: a power of two
    const _Float16 h = (_Float16)v;
    hi[c] = h;
    lo[c] = (_Float16)(v - (float)h);         // v - h is exact in fp32
  }
}

// what the upper half of the last chunk reads when dim is 16 mod 32: zeros add nothing to any product
__device__ __attribute__((aligned(16))) const unsigned char vpr_zero16[16] = {0};

// one LDS buffer <- chunk `ch` of the tile's 128 database rows and the workgroup's 64 queries.  LDS image: row-major,
// 128 B per row, the 16-B slot t of row r holding piece t ^ (r & 7) (the XOR swizzle sits on the global address, the
// LDS image stays lane-linear for global_load_lds).  Split pieces 0-3: hi, 4-7: lo; fp32 pieces: 4 floats each.
template <bool F32>
__device__ inline void issue_chunk(unsigned char* stage, const VprSearchArgs& a, int64_t r0, int q0, int ch, int wave, int lane) {
  const int rin = lane >> 3, piece = (lane & 7) ^ rin;
  const size_t rb = row_bytes(a.dim);
  const size_t poff = F32 ? (size_t)ch * CHB + piece * 16
                          : 16 + (piece < 4 ? (size_t)ch * 64 + piece * 16 : (size_t)a.dim * 2 + ch * 64 + (piece - 4) * 16);
  // elements 16 .. 31 of a chunk that ends past dim (fp32: pieces 4-7; split: pieces 2, 3 of hi and of lo) do not exist
  const bool dead = (ch + 1) * KC > a.dim && (F32 ? piece >= 4 : (piece & 3) >= 2);
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int g = wave * 6 + i;               // 24 wave instructions of 1 KB: 16 for the rows, 8 for the queries
    const unsigned char* src;
    if (g < 16) {
      int64_t r = r0 + g * 8 + rin;
      if (r >= a.ndb) r = a.ndb - 1;          // rows past the end: loaded from the last row, never selected
      src = F32 ? reinterpret_cast<const unsigned char*>(a.db + r * a.dim) : a.dbp + r * rb;
    } else {
      int qq = q0 + (g - 16) * 8 + rin;
      if (qq >= a.nq) qq = a.nq - 1;
      src = F32 ? reinterpret_cast<const unsigned char*>(a.q + (int64_t)qq * a.dim) : a.qp + (int64_t)qq * rb;
    }
    glds16(dead ? vpr_zero16 : src + poff, stage + g * 1024);   // (the hardware adds lane * 16 to the wave-uniform LDS base)
  }
}

__device__ inline const unsigned char* slot_ptr(const unsigned char* base, int r, int piece) {
  return base + r * CHB + ((piece ^ (r & 7)) << 4);
}

// one chunk of the 32 x 64 block of this wave: lane (j, h) holds query column j, rows (r & 3) + 8 (r >> 2) + 4 h
template <bool F32>
__device__ inline void mma_chunk(const unsigned char* stage, int wq, int wr, int j, int h, vf16 (&acc)[2]) {
  const unsigned char* qs = stage + RB * CHB;
  const int qr = wq * 32 + j;
  if constexpr (F32) {
    // 32x32x2: k = h inside the instruction; lane half h walks elements 16 h .. 16 h + 15 of the chunk
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float4 qv = *reinterpret_cast<const float4*>(slot_ptr(qs, qr, 4 * h + m));
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const float4 dv = *reinterpret_cast<const float4*>(slot_ptr(stage, wr * 64 + b * 32 + j, 4 * h + m));
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv.x, qv.x, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv.y, qv.y, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv.z, qv.z, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv.w, qv.w, acc[b], 0, 0, 0);
      }
    }
  } else {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const vh8 qh = *reinterpret_cast<const vh8*>(slot_ptr(qs, qr, 2 * s + h));
      const vh8 ql = *reinterpret_cast<const vh8*>(slot_ptr(qs, qr, 4 + 2 * s + h));
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int r = wr * 64 + b * 32 + j;
        const vh8 dh = *reinterpret_cast<const vh8*>(slot_ptr(stage, r, 2 * s + h));
        const vh8 dl = *reinterpret_cast<const vh8*>(slot_ptr(stage, r, 4 + 2 * s + h));
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dl, qh, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh, ql, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh, qh, acc[b], 0, 0, 0);
      }
    }
  }
}

// the K loop over dim: two LDS buffers, the load of chunk c + 1 in flight while chunk c is multiplied
template <bool F32>
__device__ inline void tile_products(unsigned char* smem, const VprSearchArgs& a, int64_t r0, int q0, int wave, int lane,
                                     vf16 (&acc)[2]) {
  const int j = lane & 31, h = lane >> 5, wq = wave >> 1, wr = wave & 1;
  const int nk = (a.dim + KC - 1) / KC;
  issue_chunk<F32>(smem, a, r0, q0, 0, wave, lane);
  for (int c = 0; c < nk; ++c) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (c + 1 < nk) issue_chunk<F32>(smem + ((c + 1) & 1) * STAGE, a, r0, q0, c + 1, wave, lane);
    mma_chunk<F32>(smem + (c & 1) * STAGE, wq, wr, j, h, acc);
  }
  __syncthreads();                            // every wave is done with the buffers: the key tile may overwrite them
}

// MASKED: query i only sees the rows whose bit is set in a.mask[i] (kp2d_vpr_search_masked); the selecting thread tests
// its query's bit where the unmasked form tests lim, and a tile none of the workgroup's queries has a row in is skipped
template <bool MASKED>
__global__ __launch_bounds__(256) void vpr_search_kernel(const VprSearchArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];   // one array: staging, key tile, tile norms
  float* s_key = reinterpret_cast<float*>(smem);
  float* s_n2 = reinterpret_cast<float*>(smem + OFF_N2);
  float* s_du = reinterpret_cast<float*>(smem + OFF_DU);
  int* s_lim = reinterpret_cast<int*>(smem + OFF_LIM);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5, wq = wave >> 1, wr = wave & 1;
  const int q0 = blockIdx.x * QB, z = blockIdx.y, nz = gridDim.y;
  const int T = (int)((a.ndb + RB - 1) / RB), per = (T + nz - 1) / nz;
  const int t_lo = z * per, t_hi = min(T, t_lo + per);
  const size_t rb = row_bytes(a.dim);
  // the selecting thread of query q0 + tid: rows [0, lim) exist for it; its list of the k best of this slice
  const int qs = q0 + tid;
  const bool selector = tid < QB && qs < a.nq;
  int lim = 0;
  if (selector) {
    int64_t l = (!MASKED && a.limit) ? a.limit[qs] : a.ndb;
    lim = (int)(l < 0 ? 0 : (l > a.ndb ? a.ndb : l));
  }
  const int64_t mw = (a.ndb + 31) >> 5;       // mask words per query
  if (tid == 0) *s_lim = 0;
  __syncthreads();
  if (selector && lim > 0) atomicMax(s_lim, lim);
  __syncthreads();
  const int wg_lim = *s_lim;                  // tiles at or past every query's limit are skipped
  unsigned long long* list = a.codes + ((size_t)z * a.nq + (selector ? qs : 0)) * a.k;
  int cnt = 0, wslot = 0;
  unsigned long long worst = EMPTY;
  // this lane's query scale 2^-s (split form)
  const int qlane = min(q0 + wq * 32 + j, a.nq - 1);
  const float uq = a.fp32 ? 1.f : reinterpret_cast<const float4*>(a.qp + (size_t)qlane * rb)->y;
  for (int t = t_lo; t < t_hi; ++t) {
    const int64_t r0 = (int64_t)t * RB;
    if (r0 >= wg_lim) break;
    unsigned m0 = 0, m1 = 0, m2 = 0, m3 = 0;  // the tile's four mask words of this thread's query (words past the row: 0)
    if constexpr (MASKED) {
      if (selector) {
        const uint32_t* mq = a.mask + (int64_t)qs * mw;
        const int64_t w0 = (int64_t)t * (RB / 32);
        m0 = mq[w0];
        if (w0 + 1 < mw) m1 = mq[w0 + 1];
        if (w0 + 2 < mw) m2 = mq[w0 + 2];
        if (w0 + 3 < mw) m3 = mq[w0 + 3];
      }
      if (!__syncthreads_or((m0 | m1 | m2 | m3) != 0)) continue;   // workgroup-uniform: no query has a row here
    }
    int bad = 0;
    if (tid < RB) {
      const int64_t r = r0 + tid;
      float4 m = make_float4(0.f, 0.f, 1.f, 0.f);
      if (r < a.ndb) m = *reinterpret_cast<const float4*>(a.dbp + r * rb);
      s_n2[tid] = m.x;
      s_du[tid] = m.y;
      bad = m.z == 0.f;
    }
    const bool f32 = __syncthreads_or(bad) || a.fp32;
    vf16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
    if (f32) tile_products<true>(smem, a, r0, q0, wave, lane, acc);
    else tile_products<false>(smem, a, r0, q0, wave, lane, acc);
    // keys of this lane's query against its 32 rows -> the key tile [query][row]
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wr * 64 + b * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float dot = f32 ? acc[b][r] : (acc[b][r] * s_du[row]) * uq;
        s_key[(wq * 32 + j) * KP + row] = fmaf(-2.f, dot, s_n2[row]);
      }
    __syncthreads();
    if (selector) {
      const int nrow = (int)min((int64_t)RB, (int64_t)lim - r0);
      for (int c = 0; c < nrow; ++c) {
        if constexpr (MASKED) {
          const unsigned w = c < 64 ? (c < 32 ? m0 : m1) : (c < 96 ? m2 : m3);
          if (!((w >> (c & 31)) & 1u)) continue;
        }
        const float key = s_key[tid * KP + c];
        if (key != key) continue;             // NaN (non-finite rows): never a neighbour
        const unsigned long long code = ((unsigned long long)fkey(key) << 32) | (unsigned)(r0 + c);
        if (cnt < a.k) {
          list[cnt++] = code;
          if (cnt < a.k) continue;
        } else {
          if (code >= worst) continue;
          list[wslot] = code;
        }
        worst = 0;                            // the list is full: find its worst (key, row)
        for (int i = 0; i < a.k; ++i) {
          const unsigned long long v = list[i];
          if (v >= worst) { worst = v; wslot = i; }
        }
      }
    }
    __syncthreads();                          // the key tile is read: the next tile's chunks may land
  }
  if (selector)
    for (int i = cnt; i < a.k; ++i) list[i] = EMPTY;
}

// the k best codes of G consecutive slices' lists -> one list (sorted)
__global__ __launch_bounds__(256) void vpr_merge_kernel(const unsigned long long* __restrict__ in, int nz_in,
                                                        unsigned long long* __restrict__ out, int nq, int k, int G) {
  __shared__ unsigned long long s[MERGE_CAND];
  const int q = blockIdx.x, zo = blockIdx.y;
  const int z0 = zo * G, zn = min(G, nz_in - z0);
  int P = 1;
  while (P < G * k) P <<= 1;
  for (int i = threadIdx.x; i < P; i += 256) {
    const int zz = i / k, e = i - zz * k;
    s[i] = zz < zn ? in[((size_t)(z0 + zz) * nq + q) * k + e] : EMPTY;
  }
  bitonic(s, P);
  for (int i = threadIdx.x; i < k; i += 256) out[((size_t)zo * nq + q) * k + i] = s[i];
}

// re-score the k finalists of a query as sum (q - d)^2 (each lane sums its float4 columns in order, then a fixed
// butterfly), sort by (distance, row), pad with (FLT_MAX, -1)
__global__ __launch_bounds__(256) void vpr_final_kernel(const unsigned long long* __restrict__ codes, const float* __restrict__ db,
                                                        const float* __restrict__ qv, int dim, int k, float* __restrict__ dist,
                                                        int64_t* __restrict__ idx) {
  __shared__ unsigned long long s[1024];
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int P = 1;
  while (P < k) P <<= 1;
  for (int i = threadIdx.x; i < P; i += 256) s[i] = (codes && i < k) ? codes[(size_t)q * k + i] : EMPTY;
  __syncthreads();
  const float* qr = qv + (size_t)q * dim;
  for (int f = wave; f < k; f += 4) {
    const unsigned long long code = s[f];
    if (code == EMPTY) continue;
    const unsigned row = (unsigned)(code & 0xffffffffu);
    const float* dr = db + (size_t)row * dim;
    float acc = 0.f;
    for (int c = lane * 4; c < dim; c += 256) {
      const float4 x = *reinterpret_cast<const float4*>(qr + c), y = *reinterpret_cast<const float4*>(dr + c);
      const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
      acc = fmaf(d0, d0, acc); acc = fmaf(d1, d1, acc); acc = fmaf(d2, d2, acc); acc = fmaf(d3, d3, acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) s[f] = ((unsigned long long)fkey(fmaxf(acc, 0.f)) << 32) | row;
  }
  bitonic(s, P);
  for (int i = threadIdx.x; i < k; i += 256) {
    const unsigned long long code = s[i];
    const bool ok = code != EMPTY;
    dist[(size_t)q * k + i] = ok ? fdec((unsigned)(code >> 32)) : FLT_MAX;
    idx[(size_t)q * k + i] = ok ? (int64_t)(code & 0xffffffffu) : -1;
  }
}

// database slices and merge fan-in of a search
struct VprPlan { int nz, G; };
VprPlan vpr_plan(int nq, int64_t ndb, int k) {
  VprPlan p{};
  const int64_t T = (ndb + RB - 1) / RB;
  const int qb = (nq + QB - 1) / QB;
  int64_t nz = (TARGET_WGS + qb - 1) / qb;
  const int64_t cap = ((int64_t)1 << 28) / ((int64_t)nq * k * 8);         // partial lists: at most 256 MB
  nz = std::max<int64_t>(1, std::min<int64_t>({nz, T, cap, 65535}));
  const int64_t per = T > 0 ? (T + nz - 1) / nz : 1;
  p.nz = T > 0 ? (int)((T + per - 1) / per) : 1;
  p.G = std::max(2, MERGE_CAND / k);
  return p;
}

// scratch: the packed queries (a.qp), the nz slices' lists (a.codes), and the lists of the first merge level (the levels
// alternate between the two); every piece on an ALIGN boundary, the total not rounded
struct VprScratch { unsigned long long* merged; size_t bytes; };
VprScratch vpr_layout(void* scratch, const VprPlan& p, VprSearchArgs& a) {
  Carve c(scratch);
  const size_t list = (size_t)a.nq * a.k;
  a.qp = c.take<unsigned char>((size_t)a.nq * row_bytes(a.dim));
  a.codes = c.take<unsigned long long>(p.nz * list);
  unsigned long long* merged = c.take<unsigned long long>((p.nz > 1 ? (p.nz + p.G - 1) / p.G : 0) * list);
  return {merged, c.end};
}

int vpr_dim_check(int dim) {
  if (dim < 16 || dim > 16384 || dim % 16) return fail(KP2D_ERR_UNSUPPORTED, "vpr: descriptor dim %d (needs dim %% 16 == 0, 16 <= dim <= 16384)", dim);
  return KP2D_OK;
}

}  // namespace

int launch_vpr_pack(const float* x, int64_t n, int dim, void* packed, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(vpr_pack_kernel, dim3((unsigned)n), dim3(256), 0, s, x, dim, (unsigned char*)packed);
  return (int)hipGetLastError();
}

int launch_vpr_search(VprSearchArgs a, void* scratch, float* dist, int64_t* idx, hipStream_t s) {
  const VprPlan p = vpr_plan(a.nq, a.ndb, a.k);
  unsigned long long* other = vpr_layout(scratch, p, a).merged;
  if (a.ndb == 0) {
    hipLaunchKernelGGL(vpr_final_kernel, dim3(a.nq), dim3(256), 0, s, nullptr, a.db, a.q, a.dim, a.k, dist, idx);
    return (int)hipGetLastError();
  }
  if (!a.fp32) hipLaunchKernelGGL(vpr_pack_kernel, dim3(a.nq), dim3(256), 0, s, a.q, a.dim, const_cast<unsigned char*>(a.qp));
  const dim3 grid((a.nq + QB - 1) / QB, p.nz);
  if (a.mask) hipLaunchKernelGGL(vpr_search_kernel<true>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(vpr_search_kernel<false>, grid, dim3(256), 0, s, a);
  unsigned long long* cur = a.codes;
  int nz = p.nz;
  while (nz > 1) {
    const int nout = (nz + p.G - 1) / p.G;
    hipLaunchKernelGGL(vpr_merge_kernel, dim3(a.nq, nout), dim3(256), 0, s, cur, nz, other, a.nq, a.k, p.G);
    std::swap(cur, other);
    nz = nout;
  }
  hipLaunchKernelGGL(vpr_final_kernel, dim3(a.nq), dim3(256), 0, s, cur, a.db, a.q, a.dim, a.k, dist, idx);
  return (int)hipGetLastError();
}

}  // namespace kp2d

using namespace kp2d;

extern "C" {

size_t kp2d_vpr_packed_bytes(int64_t n, int dim) {
  if (n < 0 || dim < 16 || dim > 16384 || dim % 16) return 0;
  return (size_t)n * row_bytes(dim);
}

int kp2d_vpr_pack(const float* x, int64_t n, int dim, void* packed, void* stream) {
  if (int e = vpr_dim_check(dim)) return e;
  if (n < 0 || n > INT32_MAX) return fail(KP2D_ERR_ARG, "vpr_pack: row count %lld", (long long)n);
  if (n == 0) return KP2D_OK;
  if (!x || !packed) return fail(KP2D_ERR_ARG, "null argument");
  if ((uintptr_t)x % 16 || (uintptr_t)packed % 16) return fail(KP2D_ERR_ARG, "vpr_pack: x and packed must be 16-byte aligned");
  DeviceGuard guard(x, (hipStream_t)stream);
  if (int e = launch_vpr_pack(x, n, dim, packed, (hipStream_t)stream)) return fail(KP2D_ERR_HIP, "vpr_pack kernel: %d", e);
  return KP2D_OK;
}

size_t kp2d_vpr_scratch_bytes(int nq, int64_t ndb, int dim, int k) {
  if (nq < 1 || ndb < 0 || ndb > INT32_MAX || dim < 16 || dim > 16384 || dim % 16 || k < 1 || k > 1024) return 0;
  VprSearchArgs a{};
  a.nq = nq; a.dim = dim; a.k = k;
  return vpr_layout(nullptr, vpr_plan(nq, ndb, k), a).bytes;
}

// kp2d_vpr_search and kp2d_vpr_search_masked: one body (limit and mask never both)
static int vpr_search_checked(const void* packed_db, const float* db, int64_t ndb, int dim, const float* q, int nq,
                              const int64_t* limit, const uint32_t* mask, int k, uint32_t flags, float* dist, int64_t* idx,
                              void* scratch, size_t scratch_bytes, void* stream) {
  if (int e = vpr_dim_check(dim)) return e;
  if (k < 1 || k > 1024) return fail(KP2D_ERR_ARG, "vpr_search: k = %d outside [1, 1024]", k);
  if (nq < 0 || ndb < 0) return fail(KP2D_ERR_ARG, "vpr_search: negative size");
  if (ndb > INT32_MAX) return fail(KP2D_ERR_UNSUPPORTED, "vpr_search: more than 2^31 - 1 database rows");
  if (flags & ~(uint32_t)KP2D_VPR_FP32) return fail(KP2D_ERR_ARG, "unknown vpr flags 0x%x", flags);
  if (nq == 0) return KP2D_OK;
  if (!q || !dist || !idx || !scratch || (ndb > 0 && (!packed_db || !db))) return fail(KP2D_ERR_ARG, "null argument");
  if ((uintptr_t)q % 16 || (uintptr_t)db % 16 || (uintptr_t)packed_db % 16 || (uintptr_t)scratch % 16)
    return fail(KP2D_ERR_ARG, "vpr_search: q, db, packed_db and scratch must be 16-byte aligned");
  const size_t need = kp2d_vpr_scratch_bytes(nq, ndb, dim, k);
  if (scratch_bytes < need) return fail(KP2D_ERR_WORKSPACE, "vpr scratch %zu B < required %zu B (kp2d_vpr_scratch_bytes)", scratch_bytes, need);
  DeviceGuard guard(q, (hipStream_t)stream);
  VprSearchArgs a{};
  a.dbp = static_cast<const unsigned char*>(packed_db);
  a.db = db; a.q = q; a.limit = limit; a.mask = mask; a.ndb = ndb; a.dim = dim; a.nq = nq; a.k = k;
  a.fp32 = (flags & KP2D_VPR_FP32) ? 1 : 0;
  if (int e = launch_vpr_search(a, scratch, dist, idx, (hipStream_t)stream)) return fail(KP2D_ERR_HIP, "vpr_search kernels: %d", e);
  return KP2D_OK;
}

int kp2d_vpr_search(const void* packed_db, const float* db, int64_t ndb, int dim, const float* q, int nq,
                    const int64_t* limit, int k, uint32_t flags, float* dist, int64_t* idx, void* scratch,
                    size_t scratch_bytes, void* stream) {
  return vpr_search_checked(packed_db, db, ndb, dim, q, nq, limit, nullptr, k, flags, dist, idx, scratch, scratch_bytes, stream);
}

int kp2d_vpr_search_masked(const void* packed_db, const float* db, int64_t ndb, int dim, const float* q, int nq,
                           const uint32_t* mask, int k, uint32_t flags, float* dist, int64_t* idx, void* scratch,
                           size_t scratch_bytes, void* stream) {
  if (nq > 0 && ndb > 0 && !mask) return fail(KP2D_ERR_ARG, "vpr_search_masked: null mask");
  if ((uintptr_t)mask % 4) return fail(KP2D_ERR_ARG, "vpr_search_masked: mask must be 4-byte aligned");
  return vpr_search_checked(packed_db, db, ndb, dim, q, nq, nullptr, mask, k, flags, dist, idx, scratch, scratch_bytes, stream);
}

}  // extern "C"
