// Fine-tuning of the NetVLAD layer on the device (kp2d_vlad_forward_train, kp2d_triplet_loss, kp2d_vlad_backward,
// kp2d_adam_step; include/kp2d.h): the step the reference's train_visloc.py:249-282 takes with torch autograd,
// TripletMarginLoss(margin ** 0.5, p=2, reduction="sum") / nNeg and Adam, for the two parameters of the layer
// (conv.weight [K, C] and centroids [K, C]).  Everything upstream is frozen: x is only_encoder's planar map [N, C, S].
//
//   forward, per frame       xh = x / max(||x||_C, 1e-12);  a = softmax_k(xh W^T);  r[k] = sum_s a[s,k]
//                            U[k] = sum_s a[s,k] xh[s] - r[k] cent[k];  n[k] = max(||U[k]||, 1e-12);  V[k] = U[k] / n[k]
//                            g = max(||V||_F, 1e-12);  v = V / g
//   backward, given dv       dV = (dv - v <v, dv>) / g;  dU[k] = (dV[k] - V[k] <V[k], dV[k]>) / n[k]
//                            dcent[k] = -r[k] dU[k];  da[s,k] = <xh[s], dU[k]> - <cent[k], dU[k]>
//                            dz[s,k] = a[s,k] (da[s,k] - sum_j a[s,j] da[s,j]);  dW[k] = sum_s dz[s,k] xh[s]
//
// Kernels (exact fp32 on the vector ALU, no float atomics, every sum in a fixed order):
//   vt_tile_kernel<false>   grid (tiles, N): one workgroup per 64-pixel tile, as netvlad.hip's tile mode: normalise, logits,
//                           softmax, the tile's [K, C] sum of a xh and its row sums -> one partial per (frame, tile)
//   vt_finish_kernel        grid (N): partials added in tile order, both normalisations; writes v and the saved record
//   vt_du_kernel            grid (N): dV, dU, <cent[k], dU[k]> and the frame's dcent from the saved record
//   vt_tile_kernel<true>    grid (tiles, N): the forward's tile again (a is recomputed, no [S, K] tensor is stored), the
//                           second [S, K] product with dU in the same loop as the logits, dz in place of a, the tile's
//                           [K, C] sum of dz xh -> one partial per (frame, tile)
//   vt_tile_kernel<true, true>   the same tile for kp2d_vlad_backward_input: a is kept beside dz, and the tile writes
//                           dx = the channel normalisation's backward of a dU + dz W instead of a dW partial
//   vt_frame_sum_kernel     grid (ceil(K C / 256), N): a frame's tile partials added in tile order
//   vt_grad_sum_kernel      grid (ceil(K C / 256)): the frames' sums added in frame order -> dW, dcent
//   tl_dist_kernel / tl_grad_kernel   the triplet loss: one workgroup per pair distance (squares summed in float64, stored
//                           as fp32), then one per descriptor row gathering its own triplets in triplet order; the last
//                           workgroup adds the fp32 hinge terms in float64
//   adam_kernel             torch.optim.Adam's element-wise update
// The order of a frame's sums depends on S alone (tile t covers pixels [64 t, 64 t + 64), tiles are added 0, 1, 2, ...),
// the order over frames on N alone (0, 1, 2, ...): bit-identical from run to run, and frames that contribute zeros
// behind the others change no bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "api_common.h"
#include "device_guard.h"
#include "train_common.h"

using namespace kp2d;

namespace {

constexpr int VT = 64;            // pixels per tile
constexpr int MAX_KC = 8192;      // K * C, the forward's limit (launch_netvlad)
constexpr int LDS_BUDGET = 160 * 1024;

// LDS of vt_tile_kernel in floats: W [K][C + 1], (backward: dU [K][C + 1],) xh [64][C + 1], a [64][K + 1].
constexpr size_t tile_lds_floats(int K, int C, bool bwd) {
  return (size_t)(bwd ? 2 : 1) * K * (C + 1) + (size_t)VT * (C + 1) + (size_t)VT * (K + 1);
}
// The largest case, K = 64, C = 128: forward (64 * 129 + 64 * 129 + 64 * 65) * 4 = 82 688 B,
// backward (2 * 64 * 129 + 64 * 129 + 64 * 65) * 4 = 115 712 B of the 160 KB a workgroup may take.
static_assert(tile_lds_floats(64, 128, false) * 4 == 82688, "forward tile LDS");
static_assert(tile_lds_floats(64, 128, true) * 4 == 115712 && tile_lds_floats(64, 128, true) * 4 <= LDS_BUDGET, "backward tile LDS");
// The input-gradient form (kp2d_vlad_backward_input) keeps a beside dz.  K <= C: in the rows of xh, whose entries each thread
// has taken into registers by then (the backward's own LDS, so as many workgroups share a CU as there: the second one halves
// the time at K = C = 64); K > C: one more [64][K + 1].
constexpr int DX_MAX_C = 128;     // a thread holds its C / 4 <= 32 entries of xh and of dxh in registers
constexpr size_t tile_lds_floats_dx(int K, int C) { return tile_lds_floats(K, C, true) + (K <= C ? 0 : (size_t)VT * (K + 1)); }
static_assert(tile_lds_floats_dx(64, 128) * 4 == 115712 && tile_lds_floats_dx(64, 16) * 4 == 46336,"input-gradient tile LDS");

__host__ __device__ inline int tiles_of(int S) { return (S + VT - 1) / VT; }
// floats of a frame's saved record: V [K C], n [K], r [K], g and three floats of padding (rows stay 16-byte aligned)
__host__ __device__ inline size_t saved_stride(int K, int C) { return (size_t)K * C + 2 * (size_t)K + 4; }

struct TileArgs {
  const float* x;      // [N][C][S] planar
  const float* w;      // [K][C]
  const float* du;     // BWD: [N][K][C]
  const float* cdu;    // BWD: [N][K]  <cent[k], dU[k]>
  float* part;         // [N][tiles][K C + K] (forward) / [N][tiles][K C] (backward)
  float* dx;           // DX: [N][C][S] planar
  int S, C, K;
};

// DX (with BWD): the gradient with respect to x in place of the tile's dW partial:
//   dxh[s] = sum_k a[s,k] dU[k] + sum_k dz[s,k] W[k];  dx[:,s] = (dxh[s] - xh[s] <xh[s], dxh[s]>) / max(||x[:,s]||, 1e-12)
template <bool BWD, bool DX = false>
__global__ __launch_bounds__(256) void vt_tile_kernel(const TileArgs a) {
  static_assert(BWD || !DX, "the input gradient is a backward form");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int C = a.C, K = a.K, S = a.S;
  const int CP = C + 1, KP = K + 1, KC = K * C;
  float* s_w = sm;                                   // [K][CP]
  float* s_d = s_w + K * CP;                         // BWD: [K][CP]
  float* s_x = s_d + (BWD ? K * CP : 0);             // [VT][CP]
  float* s_a = s_x + VT * CP;                        // [VT][KP]
  // DX: a beside dz, [VT][A2P].  K <= C: in the rows of xh (a pixel's row is read by its own four threads alone, lanes of one
  // wave, which take their entries into registers before they write a there); K > C: behind s_a
  float* s_a2 = (K <= C) ? s_x : s_a + VT * KP;
  const int A2P = (K <= C) ? CP : KP;
  const int tid = threadIdx.x;
  const int tile = blockIdx.x, b = blockIdx.y;
  const int t0 = tile * VT;
  const int np = min(VT, S - t0);                    // >= 1: the grid has ceil(S / 64) tiles
  const float* xb = a.x + (size_t)b * C * S;

  for (int e = tid; e < KC; e += 256) {
    const int k = e / C, c = e - k * C;
    s_w[k * CP + c] = a.w[e];
    if (BWD) s_d[k * CP + c] = a.du[(size_t)b * KC + e];
  }
  // planar map: consecutive threads read consecutive pixels of one channel; pixels past S are zeros
  for (int e = tid; e < VT * C; e += 256) {
    const int c = e >> 6, pp = e & 63;
    s_x[pp * CP + c] = (pp < np) ? xb[(size_t)c * S + t0 + pp] : 0.f;
  }
  __syncthreads();
  const int p = tid >> 2, q = tid & 3;               // 4 threads per pixel
  const int cq = C >> 2, kq = K >> 2;
  float xinv = 0.f;                                  // DX: 1 / max(||x[:,p]||, 1e-12)
  float xo[DX ? DX_MAX_C / 4 : 1];                   // DX: this thread's C / 4 entries of xh[p]
  {  // descriptor-wise L2 normalisation (F.normalize, eps 1e-12)
    float ss = 0.f;
    for (int c = q * cq; c < (q + 1) * cq; ++c) { const float v = s_x[p * CP + c]; ss = fmaf(v, v, ss); }
    ss += __shfl_xor(ss, 1);
    ss += __shfl_xor(ss, 2);
    const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
    for (int c = q * cq; c < (q + 1) * cq; ++c) s_x[p * CP + c] *= inv;
    if (DX) xinv = inv;
  }
  __syncthreads();
  {  // this thread owns clusters [q kq, (q + 1) kq) of pixel p: logits (and <xh, dU[k]>) in one walk over the channels
    float lg[16], da[16];
    const float* xr = &s_x[p * CP];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      lg[j] = 0.f;
      da[j] = 0.f;
      if (j < kq) {
        const float* wr = &s_w[(q * kq + j) * CP];
        const float* dr = &s_d[(q * kq + j) * CP];
        float d = 0.f, g = 0.f;
        for (int c = 0; c < C; ++c) {
          const float xv = xr[c];
          d = fmaf(wr[c], xv, d);
          if (BWD) g = fmaf(dr[c], xv, g);
        }
        lg[j] = d;
        if (BWD) da[j] = g - a.cdu[(size_t)b * K + q * kq + j];
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < kq) mx = fmaxf(mx, lg[j]);
    mx = fmaxf(mx, __shfl_xor(mx, 1));
    mx = fmaxf(mx, __shfl_xor(mx, 2));
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < kq) { lg[j] = expf(lg[j] - mx); se += lg[j]; }
    se += __shfl_xor(se, 1);
    se += __shfl_xor(se, 2);
    const float rs = (p < np) ? 1.f / se : 0.f;      // pixels past S: a = 0, and with it dz = 0
    float inner = 0.f;                               // BWD: sum_j a[j] da[j]
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < kq) { lg[j] *= rs; if (BWD) inner = fmaf(lg[j], da[j], inner); }
    if (BWD) {
      inner += __shfl_xor(inner, 1);
      inner += __shfl_xor(inner, 2);
    }
    if (DX) {
#pragma unroll
      for (int cc = 0; cc < DX_MAX_C / 4; ++cc) xo[cc] = (cc < cq) ? s_x[p * CP + q * cq + cc] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < kq) {
        s_a[p * KP + q * kq + j] = BWD ? lg[j] * (da[j] - inner) : lg[j];
        if (DX) s_a2[p * A2P + q * kq + j] = lg[j];
      }
  }
  __syncthreads();
  if (DX) {  // this thread's C / 4 channels of pixel p: both [S, K] x [K, C] products, then the normalisation's backward
    float dxh[DX_MAX_C / 4];
#pragma unroll
    for (int cc = 0; cc < DX_MAX_C / 4; ++cc) dxh[cc] = 0.f;
    const int c0 = q * cq;
    for (int k = 0; k < K; ++k) {
      const float ak = s_a2[p * A2P + k], zk = s_a[p * KP + k];
      const float* dr = &s_d[k * CP + c0];
      const float* wr = &s_w[k * CP + c0];
#pragma unroll
      for (int cc = 0; cc < DX_MAX_C / 4; ++cc)
        if (cc < cq) dxh[cc] = fmaf(zk, wr[cc], fmaf(ak, dr[cc], dxh[cc]));
    }
    float dot = 0.f;
#pragma unroll
    for (int cc = 0; cc < DX_MAX_C / 4; ++cc)
      if (cc < cq) dot = fmaf(xo[cc], dxh[cc], dot);
    dot += __shfl_xor(dot, 1);
    dot += __shfl_xor(dot, 2);
    if (p < np) {
      float* o = a.dx + (size_t)b * C * S + t0 + p;
#pragma unroll
      for (int cc = 0; cc < DX_MAX_C / 4; ++cc)
        if (cc < cq) o[(size_t)(c0 + cc) * S] = (dxh[cc] - xo[cc] * dot) * xinv;
    }
    return;
  }
  // the tile's [K][C] sum over its 64 pixels, pixel 0 first
  float* dst = a.part + ((size_t)b * gridDim.x + tile) * (BWD ? KC : KC + K);
  for (int e = tid; e < KC; e += 256) {
    const int k = e / C, c = e - k * C;
    float acc = 0.f;
#pragma unroll 8
    for (int pp = 0; pp < VT; ++pp) acc = fmaf(s_a[pp * KP + k], s_x[pp * CP + c], acc);
    dst[e] = acc;
  }
  if (!BWD && tid < K) {
    float at = 0.f;
    for (int pp = 0; pp < VT; ++pp) at += s_a[pp * KP + tid];
    dst[KC + tid] = at;
  }
}

struct FinishArgs {
  const float* part;   // [N][tiles][K C + K]
  const float* cent;   // [K][C]
  float* vlad;         // [N][K C]
  float* saved;        // [N][saved_stride]
  int tiles, C, K;
};

constexpr int FIN_T = 1024;
__global__ __launch_bounds__(FIN_T) void vt_finish_kernel(const FinishArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int C = a.C, K = a.K, KC = K * C;
  float* s_v = sm;            // [K C]
  float* s_r = s_v + KC;      // [K] row sums of a
  float* s_n = s_r + K;       // [K] 1 / n[k], then [FIN_T / 64] wave sums
  const int tid = threadIdx.x, b = blockIdx.x;
  const size_t ps = (size_t)KC + K;
  const float* base = a.part + (size_t)b * a.tiles * ps;
  float* sv = a.saved + (size_t)b * saved_stride(K, C);
  for (int e = tid; e < KC + K; e += FIN_T) s_v[e] = ordered_sum(base + e, ps, a.tiles);   // s_r follows s_v
  __syncthreads();
  for (int e = tid; e < KC; e += FIN_T) {
    const int k = e / C;
    s_v[e] = s_v[e] - s_r[k] * a.cent[e];
  }
  __syncthreads();
  for (int k = tid >> 2; k < K; k += FIN_T / 4) {     // intra-normalisation: 4 threads per cluster row
    const int q = tid & 3, cq = C >> 2;
    float ss = 0.f;
    for (int c = q * cq; c < (q + 1) * cq; ++c) { const float v = s_v[k * C + c]; ss = fmaf(v, v, ss); }
    ss += __shfl_xor(ss, 1);
    ss += __shfl_xor(ss, 2);
    if (q == 0) {
      const float n = fmaxf(sqrtf(ss), 1e-12f);
      s_n[k] = 1.f / n;
      sv[KC + k] = n;
      sv[KC + K + k] = s_r[k];
    }
  }
  __syncthreads();
  float tot = 0.f;
  for (int e = tid; e < KC; e += FIN_T) {
    const float v = s_v[e] * s_n[e / C];
    s_v[e] = v;
    sv[e] = v;
    tot = fmaf(v, v, tot);
  }
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
  __syncthreads();
  if ((tid & 63) == 0) s_n[tid >> 6] = tot;
  __syncthreads();
  float all = 0.f;
#pragma unroll
  for (int w = 0; w < FIN_T / 64; ++w) all += s_n[w];
  const float g = fmaxf(sqrtf(all), 1e-12f);
  const float inv = 1.f / g;
  if (tid < 4) sv[KC + 2 * K + tid] = tid == 0 ? g : 0.f;
  for (int e = tid; e < KC; e += FIN_T) a.vlad[(size_t)b * KC + e] = s_v[e] * inv;
}

struct DuArgs {
  const float* saved;  // [N][saved_stride]
  const float* dv;     // [N][K C]
  const float* cent;   // [K][C]
  float* du;           // [N][K C]
  float* cdu;          // [N][K]
  float* dcf;          // [N][K C]  the frame's dcent
  int C, K;
};

__global__ __launch_bounds__(256) void vt_du_kernel(const DuArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int C = a.C, K = a.K, KC = K * C;
  float* s_dv = sm;             // [K C] dV
  float* s_w = s_dv + KC;       // [4] wave sums
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* sv = a.saved + (size_t)b * saved_stride(K, C);
  const float* dv = a.dv + (size_t)b * KC;
  const float ig = 1.f / sv[KC + 2 * K];
  float dot = 0.f;                                    // <V, dv>; <v, dv> = dot / g
  for (int e = tid; e < KC; e += 256) dot = fmaf(sv[e], dv[e], dot);
  for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
  if ((tid & 63) == 0) s_w[tid >> 6] = dot;
  __syncthreads();
  const float vd = ((s_w[0] + s_w[1]) + (s_w[2] + s_w[3])) * ig;
  for (int e = tid; e < KC; e += 256) s_dv[e] = (dv[e] - sv[e] * ig * vd) * ig;
  __syncthreads();
  const int k = tid >> 2, q = tid & 3, cq = C >> 2;   // 4 threads per cluster row, K <= 64
  if (k < K) {
    const float* V = sv + (size_t)k * C;
    const float* dV = s_dv + k * C;
    float t = 0.f;
    for (int c = q * cq; c < (q + 1) * cq; ++c) t = fmaf(V[c], dV[c], t);
    t += __shfl_xor(t, 1);
    t += __shfl_xor(t, 2);
    const float in = 1.f / sv[KC + k], r = sv[KC + K + k];
    float cd = 0.f;
    for (int c = q * cq; c < (q + 1) * cq; ++c) {
      const float u = (dV[c] - V[c] * t) * in;
      a.du[(size_t)b * KC + k * C + c] = u;
      a.dcf[(size_t)b * KC + k * C + c] = -r * u;
      cd = fmaf(a.cent[k * C + c], u, cd);
    }
    cd += __shfl_xor(cd, 1);
    cd += __shfl_xor(cd, 2);
    if (q == 0) a.cdu[(size_t)b * K + k] = cd;
  }
}

// fs[b][e] = sum over the frame's tiles of part[b][t][e], tile order
__global__ __launch_bounds__(256) void vt_frame_sum_kernel(const float* part, float* fs, int tiles, int KC) {
  const int e = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (e < KC) fs[(size_t)b * KC + e] = ordered_sum(part + (size_t)b * tiles * KC + e, KC, tiles);
}

// dW[e] = sum over frames of fs[b][e], dcent[e] = sum over frames of dcf[b][e], frame order
__global__ __launch_bounds__(256) void vt_grad_sum_kernel(const float* fs, const float* dcf, float* dW, float* dcent, int N, int KC) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= KC) return;
  dW[e] = ordered_sum(fs + e, KC, N);
  dcent[e] = ordered_sum(dcf + e, KC, N);
}

// ---- triplet margin loss ------------------------------------------------------------------------------------------
__device__ __forceinline__ int clamp_off(int v, int n_neg) { return min(max(v, 0), n_neg); }

// the query that owns negative j: the first i with off[i] <= j < off[i + 1] (offsets clamped); -1: none.  A query's own
// rows walk its span [off[i], off[i + 1]) directly; the two agree for every valid prefix, and for any other one the
// clamping alone keeps every index inside vlad / dvlad (the result is then unspecified)
__device__ __forceinline__ int owner_of(const int32_t* off, int B, int n_neg, int j) {
  for (int i = 0; i < B; ++i)
    if (clamp_off(off[i], n_neg) <= j && j < clamp_off(off[i + 1], n_neg)) return i;
  return -1;
}

// block sum of a double in a fixed order: lanes by butterfly, the four waves as (0 + 1) + (2 + 3)
__device__ __forceinline__ double block_sum(double v, double* s_w) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// dist[r], r < B: d(q_r, p_r); r >= B: d(q_owner, n_{r - B}) (0 when no query owns the row).  The difference and the
// eps are fp32 operations as in torch's pairwise_distance; the squares, their sum and the square root are float64, and
// the distance is stored rounded to fp32 (the hinge terms and the gradients are fp32 arithmetic on it).
__global__ __launch_bounds__(256) void tl_dist_kernel(const float* __restrict__ v, int B, const int32_t* __restrict__ off, int n_neg,
                                                      int dim, float* __restrict__ dist) {
  __shared__ double s_w[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int i = r < B ? r : owner_of(off, B, n_neg, r - B);
  if (i < 0) {
    if (tid == 0) dist[r] = 0.f;
    return;
  }
  const float* q = v + (size_t)i * dim;
  const float* o = v + (size_t)(B + r) * dim;        // p_r is row B + r, and n_j is row 2 B + j = B + r too
  double ss = 0.0;
  for (int e = tid; e < dim; e += 256) {
    const float d = (q[e] - o[e]) + 1e-6f;
    ss += (double)d * (double)d;
  }
  ss = block_sum(ss, s_w);
  if (tid == 0) dist[r] = (float)sqrt(ss);
}

// One workgroup per descriptor row (grid 2 B + n_neg + 1): the row's gradient gathered from its own triplets in triplet
// order.  The extra last workgroup adds the hinge terms in triplet order (one wave: lane l takes triplets l, l + 64, ...,
// then a butterfly) and counts the active ones.
__global__ __launch_bounds__(256) void tl_grad_kernel(const float* __restrict__ v, int B, const int32_t* __restrict__ off, int n_neg,
                                                      int dim, float margin_sqrt, const float* __restrict__ dist,
                                                      float* __restrict__ dv, float* __restrict__ loss, int32_t* __restrict__ n_active) {
  const int N = 2 * B + n_neg;
  const int r = blockIdx.x, tid = threadIdx.x;
  const float scale = 1.f / (float)n_neg;
  if (r == N) {
    if (tid >= 64) return;
    double acc = 0.0;
    int act = 0;
    for (int i = 0; i < B; ++i) {
      const int lo = clamp_off(off[i], n_neg), hi = clamp_off(off[i + 1], n_neg);
      for (int j = lo + tid; j < hi; j += 64) {
        const float h = dist[i] - dist[B + j] + margin_sqrt;
        if (h > 0.f) { acc += (double)h; ++act; }
      }
    }
    for (int o = 32; o > 0; o >>= 1) { acc += __shfl_xor(acc, o); act += __shfl_xor(act, o); }
    if (tid == 0) { loss[0] = (float)(acc / (double)n_neg); n_active[0] = act; }
    return;
  }
  float* out = dv + (size_t)r * dim;
  if (r >= 2 * B) {                                   // a negative: one term
    const int j = r - 2 * B;
    const int i = owner_of(off, B, n_neg, j);
    const bool on = i >= 0 && dist[i] - dist[B + j] + margin_sqrt > 0.f;
    const float* q = v + (size_t)(i < 0 ? 0 : i) * dim;
    const float* n = v + (size_t)r * dim;
    const float s = on ? scale / dist[B + j] : 0.f;
    for (int e = tid; e < dim; e += 256) out[e] = on ? s * ((q[e] - n[e]) + 1e-6f) : 0.f;
    return;
  }
  const int i = r < B ? r : r - B;
  const int lo = clamp_off(off[i], n_neg), hi = clamp_off(off[i + 1], n_neg);
  const float* q = v + (size_t)i * dim;
  const float* p = v + (size_t)(B + i) * dim;
  const float dp = dist[i];
  if (r >= B) {                                       // the positive: -(q - p + eps) / d_pos once per active triplet
    int act = 0;
    for (int j = lo; j < hi; ++j)
      if (dp - dist[B + j] + margin_sqrt > 0.f) ++act;
    const float s = act ? -scale * (float)act / dp : 0.f;
    for (int e = tid; e < dim; e += 256) out[e] = act ? s * ((q[e] - p[e]) + 1e-6f) : 0.f;
    return;
  }
  for (int e = tid; e < dim; e += 256) {              // the query: its triplets in order
    const float qe = q[e];
    const float up = ((qe - p[e]) + 1e-6f) / dp;
    float acc = 0.f;
    for (int j = lo; j < hi; ++j) {
      const float dn = dist[B + j];
      if (dp - dn + margin_sqrt > 0.f)
        acc += up - ((qe - v[(size_t)(2 * B + j) * dim + e]) + 1e-6f) / dn;
    }
    out[e] = scale * acc;
  }
}

// ---- Adam -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, float w1, float beta2, float w2,
                                                   float step_size, float bc2_sqrt, float eps) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const float g = grad[e];
  const float me = m[e] + w1 * (g - m[e]);            // exp_avg.lerp_(grad, 1 - beta1)
  const float ve = v[e] * beta2 + w2 * g * g;         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  m[e] = me;
  v[e] = ve;
  const float denom = sqrtf(ve) / bc2_sqrt + eps;
  param[e] = param[e] - step_size * (me / denom);
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct TrainPlan {
  float *part, *du, *cdu, *dcf, *fs;
  size_t total;
};

// one walk: the tile partials (forward: K C + K per tile, backward: K C of the same piece) and the backward's per-frame
// pieces.  kp2d_triplet_loss knows no (S, C, K) and so walks no plan: its B + n_neg pair distances sit at the head of
// whatever scratch it is given.  In a step's shared scratch that is the head of `part`, free between the forward, whose
// finish pass has read the partials, and the backward, which writes them all again before it reads one.
TrainPlan train_plan(void* scratch, int N, int S, int C, int K) {
  TrainPlan p{};
  Carve c(scratch);
  const size_t KC = (size_t)K * C;
  p.part = c.take<float>((size_t)N * tiles_of(S) * (KC + K));
  p.du = c.take<float>((size_t)N * KC);
  p.cdu = c.take<float>((size_t)N * K);
  p.dcf = c.take<float>((size_t)N * KC);
  p.fs = c.take<float>((size_t)N * KC);
  p.total = c.bytes();
  return p;
}

// the forward's limits (launch_netvlad) and this file's LDS budget; nullptr: fine
const char* shape_problem(int N, int S, int C, int K, int* code) {
  *code = KP2D_ERR_ARG;
  if (N < 1 || N > 65535) return "N outside [1, 65535]";
  if (S < 1) return "S < 1";
  if (C < 4 || K < 4) return "K and C must be at least 4";
  *code = KP2D_ERR_UNSUPPORTED;
  if (K > 64 || (K & 3) || (C & 3) || (int64_t)K * C > MAX_KC) return "needs K % 4 == 0, C % 4 == 0, K <= 64 and K * C <= 8192";
  if (tile_lds_floats(K, C, true) * sizeof(float) > (size_t)LDS_BUDGET) return "the backward tile does not fit 160 KB of LDS";
  if ((int64_t)N * tiles_of(S) * ((int64_t)K * C + K) > (int64_t)1 << 40) return "N * S too large";
  return nullptr;
}

template <bool BWD, bool DX = false>
int launch_tile(const TileArgs& a, int N, hipStream_t st) {
  const size_t lds = (DX ? tile_lds_floats_dx(a.K, a.C) : tile_lds_floats(a.K, a.C, BWD)) * sizeof(float);
  const dim3 grid(tiles_of(a.S), N);
  static PerDeviceOnce once;      // per device: the tensors may live on any visible device
  if (int e = lds_opt_in(once, reinterpret_cast<const void*>(&vt_tile_kernel<BWD, DX>))) return e;
  hipLaunchKernelGGL((vt_tile_kernel<BWD, DX>), grid, dim3(256), lds, st, a);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t kp2d_vlad_train_scratch_bytes(int N, int S, int C, int K) {
  int code;
  if (shape_problem(N, S, C, K, &code)) return 0;
  return train_plan(nullptr, N, S, C, K).total;
}

int kp2d_vlad_forward_train(const float* x, const float* weight, const float* centroids, int N, int S, int C, int K,
                            float* vlad, float* saved, void* scratch, size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = shape_problem(N, S, C, K, &code)) return fail(code, "vlad_forward_train: %s (N %d, S %d, C %d, K %d)", why, N, S, C, K);
  if (any_null(x, weight, centroids, vlad, saved, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, weight, centroids, vlad, saved) || misaligned(scratch, 16))
    return fail(KP2D_ERR_ARG, "vlad_forward_train: float arrays must be 4-byte aligned, scratch 16-byte");
  const TrainPlan p = train_plan(scratch, N, S, C, K);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_ARG, "vlad_forward_train scratch %zu B < required %zu B (kp2d_vlad_train_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  TileArgs t{};
  t.x = x; t.w = weight; t.part = p.part; t.S = S; t.C = C; t.K = K;
  if (int e = launch_tile<false>(t, N, st)) return fail(KP2D_ERR_HIP, "vlad_forward_train: tile kernel: %d", e);
  FinishArgs f{};
  f.part = p.part; f.cent = centroids; f.vlad = vlad; f.saved = saved; f.tiles = tiles_of(S); f.C = C; f.K = K;
  const size_t lds = (size_t)(K * C + K + (K > FIN_T / 64 ? K : FIN_T / 64) + 8) * sizeof(float);
  hipLaunchKernelGGL(vt_finish_kernel, dim3(N), dim3(FIN_T), lds, st, f);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_vlad_backward(const float* x, const float* weight, const float* centroids, const float* saved, const float* dvlad,
                       int N, int S, int C, int K, float* d_weight, float* d_centroids, void* scratch, size_t scratch_bytes,
                       void* stream) {
  int code;
  if (const char* why = shape_problem(N, S, C, K, &code)) return fail(code, "vlad_backward: %s (N %d, S %d, C %d, K %d)", why, N, S, C, K);
  if (any_null(x, weight, centroids, saved, dvlad, d_weight, d_centroids, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, weight, centroids, saved, dvlad, d_weight, d_centroids) || misaligned(scratch, 16))
    return fail(KP2D_ERR_ARG, "vlad_backward: float arrays must be 4-byte aligned, scratch 16-byte");
  const TrainPlan p = train_plan(scratch, N, S, C, K);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_ARG, "vlad_backward scratch %zu B < required %zu B (kp2d_vlad_train_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  const int KC = K * C;
  DuArgs d{};
  d.saved = saved; d.dv = dvlad; d.cent = centroids; d.du = p.du; d.cdu = p.cdu; d.dcf = p.dcf; d.C = C; d.K = K;
  hipLaunchKernelGGL(vt_du_kernel, dim3(N), dim3(256), (size_t)(KC + 4) * sizeof(float), st, d);
  HIP_TRY(hipGetLastError());
  TileArgs t{};
  t.x = x; t.w = weight; t.du = p.du; t.cdu = p.cdu; t.part = p.part; t.S = S; t.C = C; t.K = K;
  if (int e = launch_tile<true>(t, N, st)) return fail(KP2D_ERR_HIP, "vlad_backward: tile kernel: %d", e);
  hipLaunchKernelGGL(vt_frame_sum_kernel, dim3((KC + 255) / 256, N), dim3(256), 0, st, p.part, p.fs, tiles_of(S), KC);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(vt_grad_sum_kernel, dim3((KC + 255) / 256), dim3(256), 0, st, p.fs, p.dcf, d_weight, d_centroids, N, KC);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_vlad_backward_input(const float* x, const float* weight, const float* centroids, const float* saved, const float* dvlad,
                             int N, int S, int C, int K, float* dx, void* scratch, size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = shape_problem(N, S, C, K, &code)) return fail(code, "vlad_backward_input: %s (N %d, S %d, C %d, K %d)", why, N, S, C, K);
  if (C > DX_MAX_C || tile_lds_floats_dx(K, C) * sizeof(float) > (size_t)LDS_BUDGET)
    return fail(KP2D_ERR_UNSUPPORTED, "vlad_backward_input: needs C <= %d and a tile within 160 KB of LDS (C %d, K %d)", DX_MAX_C, C, K);
  if (any_null(x, weight, centroids, saved, dvlad, dx, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(x, weight, centroids, saved, dvlad, dx) || misaligned(scratch, 16))
    return fail(KP2D_ERR_ARG, "vlad_backward_input: float arrays must be 4-byte aligned, scratch 16-byte");
  const TrainPlan p = train_plan(scratch, N, S, C, K);
  if (scratch_bytes < p.total) return fail(KP2D_ERR_ARG, "vlad_backward_input scratch %zu B < required %zu B (kp2d_vlad_train_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(x, st);
  DuArgs d{};      // dU and <cent[k], dU[k]> as kp2d_vlad_backward forms them (the frame's dcent lands in scratch, unused)
  d.saved = saved; d.dv = dvlad; d.cent = centroids; d.du = p.du; d.cdu = p.cdu; d.dcf = p.dcf; d.C = C; d.K = K;
  hipLaunchKernelGGL(vt_du_kernel, dim3(N), dim3(256), (size_t)(K * C + 4) * sizeof(float), st, d);
  HIP_TRY(hipGetLastError());
  TileArgs t{};
  t.x = x; t.w = weight; t.du = p.du; t.cdu = p.cdu; t.dx = dx; t.S = S; t.C = C; t.K = K;
  if (int e = launch_tile<true, true>(t, N, st)) return fail(KP2D_ERR_HIP, "vlad_backward_input: tile kernel: %d", e);
  return KP2D_OK;
}

int kp2d_triplet_loss(const float* vlad, int B, const int32_t* neg_offset, int n_neg, int dim, double margin, float* loss,
                      float* dvlad, int32_t* n_active, void* scratch, size_t scratch_bytes, void* stream) {
  if (B < 1 || n_neg < 0 || dim < 1) return fail(KP2D_ERR_ARG, "triplet_loss: B %d, n_neg %d, dim %d", B, n_neg, dim);
  if ((int64_t)2 * B + n_neg > 65535) return fail(KP2D_ERR_UNSUPPORTED, "triplet_loss: more than 65535 descriptor rows");
  if (!(margin >= 0.0) || std::isinf(margin)) return fail(KP2D_ERR_ARG, "triplet_loss: margin %g", margin);
  if (any_null(vlad, neg_offset, loss, dvlad, n_active, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(vlad, neg_offset, loss, dvlad, n_active, scratch))
    return fail(KP2D_ERR_ARG, "triplet_loss: arrays must be 4-byte aligned");
  const int N = 2 * B + n_neg;
  const size_t need = (size_t)(B + n_neg) * sizeof(float);
  if (scratch_bytes < need) return fail(KP2D_ERR_ARG, "triplet_loss scratch %zu B < required %zu B", scratch_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(vlad, st);
  if (n_neg == 0) {                                   // no triplet: loss 0, zero gradients
    HIP_TRY(hipMemsetAsync(loss, 0, sizeof(float), st));
    HIP_TRY(hipMemsetAsync(n_active, 0, sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(dvlad, 0, (size_t)N * dim * sizeof(float), st));
    return KP2D_OK;
  }
  float* dist = static_cast<float*>(scratch);
  hipLaunchKernelGGL(tl_dist_kernel, dim3(B + n_neg), dim3(256), 0, st, vlad, B, neg_offset, n_neg, dim, dist);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(tl_grad_kernel, dim3(N + 1), dim3(256), 0, st, vlad, B, neg_offset, n_neg, dim, (float)std::sqrt(margin),
                     dist, dvlad, loss, n_active);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_adam_step(float* param, const float* grad, float* m, float* v, int64_t n, int64_t step, double lr, double beta1,
                   double beta2, double eps, void* stream) {
  if (n < 0 || step < 1) return fail(KP2D_ERR_ARG, "adam_step: n %lld, step %lld (steps count from 1)", (long long)n, (long long)step);
  if (!(lr >= 0.0) || std::isinf(lr) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || std::isinf(eps))
    return fail(KP2D_ERR_ARG, "adam_step: lr %g, betas (%g, %g), eps %g", lr, beta1, beta2, eps);
  if (n == 0) return KP2D_OK;
  if (n > (int64_t)INT32_MAX * 256) return fail(KP2D_ERR_UNSUPPORTED, "adam_step: more than 2^39 elements");
  if (any_null(param, grad, m, v)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(param, grad, m, v)) return fail(KP2D_ERR_ARG, "adam_step: arrays must be 4-byte aligned");
  // the two bias corrections in double, as torch forms them on the host
  const double bc1 = 1.0 - std::pow(beta1, (double)step);
  const double bc2 = 1.0 - std::pow(beta2, (double)step);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(param, st);
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, param, grad, m, v, n, (float)(1.0 - beta1),
                     (float)beta2, (float)(1.0 - beta2), (float)(lr / bc1), (float)std::sqrt(bc2), (float)eps);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

}  // extern "C"
