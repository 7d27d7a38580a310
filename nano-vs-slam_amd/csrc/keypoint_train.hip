// Fine-tuning of the keypoint heads on the device (include/kp2d.h): the self-supervised keypoint loss of the reference's
// KeypointNetwithIOLoss.forward (KeypointNetwithIOLoss.py:423-541 with build_descriptor_loss, :25-154; with_io = False)
// over a frame (the TARGET view) and its homography-warped view (the SOURCE view), with its gradient with respect to the
// six maps the model's training forward returns.  Per frame pair b, N = Hc Wc cells, n = (Hc - 2)(Wc - 2) interior cells:
//
//   kl_decode       a thread per cell: both views' coordinates, the source's normalised and warped coordinates and the
//                   Jacobian of the warp with respect to the source coordinate
//   kl_nearest      a thread per source cell, the target coordinates tiled through LDS 256 at a time: d_i and a_i
//   kl_sums         a workgroup per pair: M_b, sum d, sum S, the consistency sum, float64, in an order the shapes fix
//   kl_merge_a      one thread: the pairs' sums in pair order -> M, mean d, mean S
//   kl_source_grad  a workgroup per pair: sum S (d - mean); per cell the gradient of its warped point, of its own score and
//                   shift, and what it sends to the target cells it touches
//   kl_target_grad  a thread per TARGET cell scans the pair's source cells in ascending order (LDS tiles) and adds what
//                   each sends it: through a_i (coordinate and score) and through the bilinear consistency sampling
//   kd_sample       a wave per interior cell and view: bilinear sampling of the descriptor map, the normalisation
//   kd_search       64 anchors per workgroup (16 per wave), candidates 64 at a time: the n x n x C products on
//                   v_mfma_f32_16x16x4_f32 with both running argmins per anchor; nothing of size n x n is stored
//   kd_hinge        a wave per anchor: the triplet term, its gradient with respect to ref
//   kd_tar_grad     a wave per candidate column scans neg[] in ascending anchor order: the gradient with respect to tar
//   kd_norm_back    a wave per anchor and view: back through the normalisation
//   kd_frame_sums   a workgroup per pair: the hinge sum (float64) and the recall count
//   kd_feat_grad    a thread per descriptor-map pixel scans the pair's anchors in ascending order: the bilinear backward
//   kl_merge_b      one thread: the parts, the total, the counts
// Per-cell and per-product arithmetic is fp32; the sums over cells and the per-anchor reductions over the channels are float64.
// No float atomics; every sum is taken in an order that depends on the shapes alone: bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "api_common.h"
#include "device_guard.h"
#include "train_common.h"

using namespace kp2d;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float DESC_EPS = 1e-8f, TRIPLET_EPS = 1e-6f, TRIPLET_MARGIN = (float)KP2D_KEYPOINT_MARGIN;
constexpr float VALID_DIST = (float)KP2D_KEYPOINT_VALID_DIST;
constexpr int MIN_ANCHORS = KP2D_KEYPOINT_MIN_ANCHORS;
constexpr int TP = 68;              // floats of an LDS row of kd_search: 64 channels + 4

struct Geo {
  int B, Hc, Wc, C, Hf, Wf, N, n, wi;       // wi = Wc - 2: interior cells of a row
  float H1, W1;                             // H - 1, W - 1
  float sx, sy;                             // (W - 1) / 2, (H - 1) / 2
  float cell, step, reach;                  // reach = cross_ratio * step
  float relax;
  bool desc;                                // n >= MIN_ANCHORS
};

struct Weights { double loc, desc, score, all; };

struct Plan {
  float2 *ct, *cs, *wn, *w;        // [B, N]: target / source coordinates, the source's warped normalised / warped ones
  float4* jac;                     // [B, N]: d w / d cs = (wx_cx, wx_cy, wy_cx, wy_cy)
  float* d;                        // [B, N]
  int* a;                          // [B, N]
  float* diff;                     // [B, N]: resampled target score - source score at an interior cell, else 0
  float4* send;                    // [B, N]: (gwx, gwy, score_t[a_i]'s share, the consistency coefficient)
  double* fsum;                    // [B, 6]: sum d, sum S, consistency, sum S (d - mean), hinge sum, spare
  long long* fcnt;                 // [B, 2]: M_b, matches
  double* coef;                    // [8]: mean d, mean S, 1 / M
  float *xr, *xt, *r, *t, *gr, *gt;      // [B, n, C]
  int *neg, *hit;                  // [B, n]
  float *cp, *cn, *hinge;          // [B, n]
  size_t total;
};

Plan make_plan(void* scratch, const Geo& g) {
  Plan p{};
  Carve c(scratch);
  const size_t BN = (size_t)g.B * g.N, Bn = (size_t)g.B * (g.desc ? g.n : 0), BnC = Bn * g.C;
  p.ct = c.take<float2>(BN);
  p.cs = c.take<float2>(BN);
  p.wn = c.take<float2>(BN);
  p.w = c.take<float2>(BN);
  p.jac = c.take<float4>(BN);
  p.d = c.take<float>(BN);
  p.a = c.take<int>(BN);
  p.diff = c.take<float>(BN);
  p.send = c.take<float4>(BN);
  p.fsum = c.take<double>((size_t)g.B * 6);
  p.fcnt = c.take<long long>((size_t)g.B * 2);
  p.coef = c.take<double>(8);
  p.xr = c.take<float>(BnC);
  p.xt = c.take<float>(BnC);
  p.r = c.take<float>(BnC);
  p.t = c.take<float>(BnC);
  p.gr = c.take<float>(BnC);
  p.gt = c.take<float>(BnC);
  p.neg = c.take<int>(Bn);
  p.hit = c.take<int>(Bn);
  p.cp = c.take<float>(Bn);
  p.cn = c.take<float>(Bn);
  p.hinge = c.take<float>(Bn);
  p.total = c.bytes();
  return p;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the four waves' values in wave order; every thread gets the sum (s: four slots of LDS)
template <class T>
__device__ __forceinline__ T block_sum(T v, T* s) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s[0] + s[1]) + (s[2] + s[3]);
}

__device__ __forceinline__ bool interior(const Geo& g, int i) {
  const int y = i / g.Wc, x = i - y * g.Wc;
  return y > 0 && y < g.Hc - 1 && x > 0 && x < g.Wc - 1;
}
// the cell of interior anchor k (row-major over the interior)
__device__ __forceinline__ int anchor_cell(const Geo& g, int k) {
  const int y = k / g.wi;
  return (y + 1) * g.Wc + (k - y * g.wi) + 1;
}

// post_processing's coordinate of cell i from its shift: *open = the clamp's gradient (1 on the closed interval)
__device__ __forceinline__ float2 decode(const Geo& g, const float* shift, int b, int i, bool* open_x, bool* open_y) {
  const int y = i / g.Wc, x = i - y * g.Wc;
  const float ux = ((float)x * g.cell + g.step) + shift[((size_t)b * 2) * g.N + i] * g.reach;
  const float uy = ((float)y * g.cell + g.step) + shift[((size_t)b * 2 + 1) * g.N + i] * g.reach;
  *open_x = ux >= 0.f && ux <= g.W1;
  *open_y = uy >= 0.f && uy <= g.H1;
  return make_float2(fminf(fmaxf(ux, 0.f), g.W1), fminf(fmaxf(uy, 0.f), g.H1));
}

__global__ __launch_bounds__(256) void kl_decode(Geo g, const float* __restrict__ shift_t, const float* __restrict__ shift_s,
                                                 const float* __restrict__ hom, Plan p) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= g.N) return;
  bool ox, oy;
  const float2 ct = decode(g, shift_t, b, i, &ox, &oy);
  const float2 cs = decode(g, shift_s, b, i, &ox, &oy);
  const float* h = hom + (size_t)b * 9;
  const float nx = cs.x / g.sx - 1.f, ny = cs.y / g.sy - 1.f;
  const float X = h[2] + (nx * h[0] + ny * h[1]), Y = h[5] + (nx * h[3] + ny * h[4]), Z = h[8] + (nx * h[6] + ny * h[7]);
  const float iz = 1.f / Z;
  const float wnx = X * iz, wny = Y * iz;
  const size_t at = (size_t)b * g.N + i;
  p.ct[at] = ct;
  p.cs[at] = cs;
  p.wn[at] = make_float2(wnx, wny);
  p.w[at] = make_float2((wnx + 1.f) * g.sx, (wny + 1.f) * g.sy);
  // d w / d cs: w = (X / Z + 1) s, n = c / s - 1
  p.jac[at] = make_float4((h[0] - wnx * h[6]) * iz, (h[1] - wnx * h[7]) * iz * (g.sx / g.sy),
                          (h[3] - wny * h[6]) * iz * (g.sy / g.sx), (h[4] - wny * h[7]) * iz);
}

__global__ __launch_bounds__(256) void kl_nearest(Geo g, Plan p) {
  __shared__ float2 s_t[256];
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  const float2 w = i < g.N ? p.w[(size_t)b * g.N + i] : make_float2(0.f, 0.f);
  float best = INFINITY;
  int arg = 0;
  for (int j0 = 0; j0 < g.N; j0 += 256) {
    __syncthreads();
    if (j0 + (int)threadIdx.x < g.N) s_t[threadIdx.x] = p.ct[(size_t)b * g.N + j0 + threadIdx.x];
    __syncthreads();
    const int m = g.N - j0 < 256 ? g.N - j0 : 256;
    for (int j = 0; j < m; ++j) {
      const float dx = w.x - s_t[j].x, dy = w.y - s_t[j].y;
      const float q = dx * dx + dy * dy;
      if (q < best) { best = q; arg = j0 + j; }      // ascending j and a strict test: the lowest index among equal values
    }
  }
  if (i < g.N) {
    p.d[(size_t)b * g.N + i] = sqrtf(best);
    p.a[(size_t)b * g.N + i] = arg;
  }
}

// bilinear tap of grid_sample (align_corners = True): the pixel coordinate and its lower corner, kept inside [-2, size]
__device__ __forceinline__ void tap(float nrm, int size, float* pix, int* lo) {
  *pix = ((nrm + 1.f) / 2.f) * (float)(size - 1);
  *lo = (int)fminf(fmaxf(floorf(*pix), -2.f), (float)size);
}

__device__ __forceinline__ float masked_score(const Geo& g, const float* score, int b, int y, int x) {
  if (y < 1 || y >= g.Hc - 1 || x < 1 || x >= g.Wc - 1) return 0.f;      // outside the map: zero padding; the border ring: masked
  return score[(size_t)b * g.N + y * g.Wc + x];
}

__global__ __launch_bounds__(256) void kl_sums(Geo g, const float* __restrict__ score_t, const float* __restrict__ score_s, Plan p) {
  __shared__ double s_d[4];
  __shared__ long long s_l[4];
  const int b = blockIdx.x;
  double sd = 0.0, sS = 0.0, sc = 0.0;
  long long M = 0;
  for (int i = threadIdx.x; i < g.N; i += 256) {
    const size_t at = (size_t)b * g.N + i;
    float diff = 0.f;
    if (interior(g, i)) {
      const float d = p.d[at];
      const float ss = score_s[at];
      if (d < VALID_DIST) {
        const int a = p.a[at];
        const float S = masked_score(g, score_t, b, a / g.Wc, a % g.Wc) + ss;
        ++M;
        sd += (double)d;
        sS += (double)S;
      }
      const float2 wn = p.wn[at];
      float px, py;
      int x0, y0;
      tap(wn.x, g.Wc, &px, &x0);
      tap(wn.y, g.Hc, &py, &y0);
      const float wx1 = px - (float)x0, wx0 = (float)(x0 + 1) - px, wy1 = py - (float)y0, wy0 = (float)(y0 + 1) - py;
      const float v = masked_score(g, score_t, b, y0, x0) * (wx0 * wy0) + masked_score(g, score_t, b, y0, x0 + 1) * (wx1 * wy0) +
                      masked_score(g, score_t, b, y0 + 1, x0) * (wx0 * wy1) + masked_score(g, score_t, b, y0 + 1, x0 + 1) * (wx1 * wy1);
      diff = v - ss;
      sc += (double)diff * (double)diff;
    }
    p.diff[at] = diff;
  }
  sd = block_sum(sd, s_d);
  sS = block_sum(sS, s_d);
  sc = block_sum(sc, s_d);
  M = block_sum(M, s_l);
  if (threadIdx.x == 0) {
    p.fsum[(size_t)b * 6] = sd;
    p.fsum[(size_t)b * 6 + 1] = sS;
    p.fsum[(size_t)b * 6 + 2] = sc;
    p.fcnt[(size_t)b * 2] = M;
  }
}

__global__ __launch_bounds__(64) void kl_merge_a(Geo g, Plan p) {
  if (threadIdx.x != 0) return;
  long long M = 0;
  double sd = 0.0, sS = 0.0;
  for (int b = 0; b < g.B; ++b) {
    M += p.fcnt[(size_t)b * 2];
    sd += p.fsum[(size_t)b * 6];
    sS += p.fsum[(size_t)b * 6 + 1];
  }
  p.coef[0] = M > 0 ? sd / (double)M : 0.0;
  p.coef[1] = M > 0 ? sS / (double)M : 0.0;
  p.coef[2] = M > 0 ? 1.0 / (double)M : 0.0;
}

__global__ __launch_bounds__(256) void kl_source_grad(Geo g, Weights wt, const float* __restrict__ score_t, const float* __restrict__ score_s,
                                                      const float* __restrict__ shift_s, Plan p, float* __restrict__ dscore_s,
                                                      float* __restrict__ dshift_s) {
  __shared__ double s_d[4];
  const int b = blockIdx.x;
  const double mean = p.coef[0], Sbar = p.coef[1], iM = p.coef[2];
  const float k_loc = (float)(wt.all * wt.loc * iM), k_usp = (float)(wt.all * wt.score * iM);
  const float k_con = g.n > 0 ? (float)(wt.all * wt.score * 4.0 / ((double)g.B * (double)g.n)) : 0.f;      // 2 MSE: 2 * 2 (v - s) / (B n)
  double su = 0.0;
  for (int i = threadIdx.x; i < g.N; i += 256) {
    const size_t at = (size_t)b * g.N + i;
    float4 send = make_float4(0.f, 0.f, 0.f, 0.f);
    float gs = 0.f;
    if (interior(g, i)) {
      const float d = p.d[at];
      if (d < VALID_DIST) {
        const int a = p.a[at];
        const float S = masked_score(g, score_t, b, a / g.Wc, a % g.Wc) + score_s[at];
        const float dev = (float)((double)d - mean);
        su += (double)S * ((double)d - mean);
        const float gd = k_loc + k_usp * (float)((double)S - Sbar);
        if (d > 0.f) {
          const float2 w = p.w[at], c = p.ct[(size_t)b * g.N + a];
          send.x = gd * ((w.x - c.x) / d);
          send.y = gd * ((w.y - c.y) / d);
        }
        send.z = k_usp * dev;
        gs = send.z;
      }
      send.w = k_con * p.diff[at];
      gs -= send.w;
    }
    p.send[at] = send;
    dscore_s[at] = gs;
    bool ox, oy;
    decode(g, shift_s, b, i, &ox, &oy);
    const float4 J = p.jac[at];
    dshift_s[((size_t)b * 2) * g.N + i] = ox ? (send.x * J.x + send.y * J.z) * g.reach : 0.f;
    dshift_s[((size_t)b * 2 + 1) * g.N + i] = oy ? (send.x * J.y + send.y * J.w) * g.reach : 0.f;
  }
  su = block_sum(su, s_d);
  if (threadIdx.x == 0) p.fsum[(size_t)b * 6 + 3] = su;
}

__global__ __launch_bounds__(256) void kl_target_grad(Geo g, const float* __restrict__ shift_t, Plan p, float* __restrict__ dscore_t,
                                                      float* __restrict__ dshift_t) {
  __shared__ float4 s_send[256];
  __shared__ float2 s_pix[256];
  __shared__ int s_a[256], s_x0[256], s_y0[256];
  const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  const int jy = j / g.Wc, jx = j - jy * g.Wc;
  float gx = 0.f, gy = 0.f, gs = 0.f, gc = 0.f;
  for (int i0 = 0; i0 < g.N; i0 += 256) {
    __syncthreads();
    const int i = i0 + threadIdx.x;
    if (i < g.N) {
      const size_t at = (size_t)b * g.N + i;
      s_send[threadIdx.x] = p.send[at];
      s_a[threadIdx.x] = p.a[at];
      const float2 wn = p.wn[at];
      float px, py;
      tap(wn.x, g.Wc, &px, &s_x0[threadIdx.x]);
      tap(wn.y, g.Hc, &py, &s_y0[threadIdx.x]);
      s_pix[threadIdx.x] = make_float2(px, py);
    }
    __syncthreads();
    const int m = g.N - i0 < 256 ? g.N - i0 : 256;
    for (int q = 0; q < m; ++q) {      // ascending source cell
      const float4 send = s_send[q];
      if (s_a[q] == j) { gx -= send.x; gy -= send.y; gs += send.z; }
      const int ex = jx - s_x0[q], ey = jy - s_y0[q];
      if ((unsigned)ex < 2u && (unsigned)ey < 2u && send.w != 0.f) {
        const float2 pix = s_pix[q];
        const float wx = ex ? pix.x - (float)s_x0[q] : (float)(s_x0[q] + 1) - pix.x;
        const float wy = ey ? pix.y - (float)s_y0[q] : (float)(s_y0[q] + 1) - pix.y;
        gc += send.w * (wx * wy);
      }
    }
  }
  if (j >= g.N) return;
  dscore_t[(size_t)b * g.N + j] = interior(g, j) ? gs + gc : 0.f;
  bool ox, oy;
  decode(g, shift_t, b, j, &ox, &oy);
  dshift_t[((size_t)b * 2) * g.N + j] = ox ? gx * g.reach : 0.f;
  dshift_t[((size_t)b * 2 + 1) * g.N + j] = oy ? gy * g.reach : 0.f;
}

// ---- the descriptor term -----------------------------------------------------------------------------------------------------
// grid (ceil(n / 4), B, 2): z = 0 ref (the source map at the source coordinate), z = 1 tar (the target map at the warped one)
__global__ __launch_bounds__(256) void kd_sample(Geo g, const float* __restrict__ feat_t, const float* __restrict__ feat_s, Plan p) {
  const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (k >= g.n) return;
  const bool tar = blockIdx.z == 1;
  const int cell = anchor_cell(g, k);
  float2 nrm;
  if (tar) {
    nrm = p.wn[(size_t)b * g.N + cell];
  } else {
    const float2 c = p.cs[(size_t)b * g.N + cell];
    nrm = make_float2(c.x / g.sx - 1.f, c.y / g.sy - 1.f);
  }
  const float* feat = (tar ? feat_t : feat_s) + (size_t)b * g.C * g.Hf * g.Wf;
  float px, py;
  int x0, y0;
  tap(nrm.x, g.Wf, &px, &x0);
  tap(nrm.y, g.Hf, &py, &y0);
  const float wx1 = px - (float)x0, wx0 = (float)(x0 + 1) - px, wy1 = py - (float)y0, wy0 = (float)(y0 + 1) - py;
  const bool in_x0 = x0 >= 0 && x0 < g.Wf, in_x1 = x0 + 1 >= 0 && x0 + 1 < g.Wf, in_y0 = y0 >= 0 && y0 < g.Hf, in_y1 = y0 + 1 >= 0 && y0 + 1 < g.Hf;
  float x[4];
  double sq = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = lane + 64 * u;
    x[u] = 0.f;
    if (c < g.C) {
      const float* m = feat + (size_t)c * g.Hf * g.Wf;
      const float v00 = in_y0 && in_x0 ? m[y0 * g.Wf + x0] : 0.f, v01 = in_y0 && in_x1 ? m[y0 * g.Wf + x0 + 1] : 0.f;
      const float v10 = in_y1 && in_x0 ? m[(y0 + 1) * g.Wf + x0] : 0.f, v11 = in_y1 && in_x1 ? m[(y0 + 1) * g.Wf + x0 + 1] : 0.f;
      x[u] = v00 * (wx0 * wy0) + v01 * (wx1 * wy0) + v10 * (wx0 * wy1) + v11 * (wx1 * wy1);
      const double e = (double)x[u] + (double)DESC_EPS;
      sq += e * e;
    }
  }
  sq = wave_sum(sq);                                  // the per-anchor reductions are float64: O(n C) work beside the n^2 C search
  const float inv = (float)(1.0 / (sqrt(sq) + (double)DESC_EPS));
  float* raw = (tar ? p.xt : p.xr) + ((size_t)b * g.n + k) * g.C;
  float* out = (tar ? p.t : p.r) + ((size_t)b * g.n + k) * g.C;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = lane + 64 * u;
    if (c < g.C) { raw[c] = x[u]; out[c] = x[u] * inv; }
  }
}

// lower value wins; of equal values the lower index
__device__ __forceinline__ void take_lower(float* v, int* j, float ov, int oj) {
  if (ov < *v || (ov == *v && oj < *j)) { *v = ov; *j = oj; }
}

// grid (ceil(n / 64), B).  The product tile is D[candidate][anchor]: A = tar (rows: candidates), B = ref (columns: anchors),
// so lane (col = lane & 15, grp = lane >> 4) holds candidates 16 t + 4 grp + reg of tile t for ITS anchor col.
__global__ __launch_bounds__(256) void kd_search(Geo g, Plan p) {
  __shared__ float s_r[64 * TP], s_t[64 * TP];
  __shared__ float2 s_w[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, grp = lane >> 4;
  const int b = blockIdx.y, i0 = blockIdx.x * 64, n = g.n, C = g.C;
  const int anchor = i0 + wave * 16 + col;
  const float2* w = p.w + (size_t)b * g.N;
  const float2 wa = anchor < n ? w[anchor_cell(g, anchor)] : make_float2(0.f, 0.f);
  const float* R = p.r + (size_t)b * n * C;
  const float* T = p.t + (size_t)b * n * C;
  const int chunks = (C + 63) / 64;
  float best_v = INFINITY, neg_v = INFINITY;
  int best_j = 0x7fffffff, neg_j = 0x7fffffff;
  for (int j0 = 0; j0 < n; j0 += 64) {
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < chunks; ++ch) {
      const int kc = C - 64 * ch < 64 ? C - 64 * ch : 64;      // a multiple of 16
      __syncthreads();
      for (int e = tid; e < 64 * kc; e += 256) {
        const int row = e / kc, k = e - row * kc;
        if (chunks > 1 || j0 == 0) s_r[row * TP + k] = i0 + row < n ? R[(size_t)(i0 + row) * C + 64 * ch + k] : 0.f;
        s_t[row * TP + k] = j0 + row < n ? T[(size_t)(j0 + row) * C + 64 * ch + k] : 0.f;
      }
      if (ch == 0 && tid < 64) s_w[tid] = j0 + tid < n ? w[anchor_cell(g, j0 + tid)] : make_float2(0.f, 0.f);
      __syncthreads();
      for (int kk = 0; kk < kc / 4; ++kk) {
        const float bv = s_r[(wave * 16 + col) * TP + 4 * kk + grp];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_t[(16 * t + col) * TP + 4 * kk + grp], bv, acc[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int jl = 16 * t + 4 * grp + reg, j = j0 + jl;
        if (j < n) {
          const float dot = fminf(fmaxf(acc[t][reg], -1.f), 1.f);
          const float v = sqrtf((2.f - 2.f * dot) + DESC_EPS);
          const float2 wj = s_w[jl];
          if (v < best_v) { best_v = v; best_j = j; }      // ascending j within the lane
          const bool within = fabsf(wj.x - wa.x) <= g.relax && fabsf(wj.y - wa.y) <= g.relax;
          if (!within && v < neg_v) { neg_v = v; neg_j = j; }
        }
      }
  }
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    take_lower(&best_v, &best_j, __shfl_xor(best_v, o), __shfl_xor(best_j, o));
    take_lower(&neg_v, &neg_j, __shfl_xor(neg_v, o), __shfl_xor(neg_j, o));
  }
  if (grp == 0 && anchor < n) {
    const float2 wb = w[anchor_cell(g, best_j)];
    p.hit[(size_t)b * n + anchor] = wb.x == wa.x && wb.y == wa.y ? 1 : 0;
    p.neg[(size_t)b * n + anchor] = neg_j == 0x7fffffff ? best_j : neg_j;      // no admissible column: the overall nearest
  }
}

// grid (ceil(n / 4), B): a wave per anchor
__global__ __launch_bounds__(256) void kd_hinge(Geo g, float scale, Plan p) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (i >= g.n) return;
  const size_t row = (size_t)b * g.n + i;
  const float* a = p.r + row * g.C;
  const float* pos = p.t + row * g.C;
  const float* ng = p.t + ((size_t)b * g.n + p.neg[row]) * g.C;
  float ep[4], en[4];
  double sp = 0.0, sn = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = lane + 64 * u;
    ep[u] = en[u] = 0.f;
    if (c < g.C) {
      ep[u] = (a[c] - pos[c]) + TRIPLET_EPS;
      en[u] = (a[c] - ng[c]) + TRIPLET_EPS;
      sp += (double)ep[u] * (double)ep[u];
      sn += (double)en[u] * (double)en[u];
    }
  }
  const double dp = sqrt(wave_sum(sp)), dn = sqrt(wave_sum(sn));
  const float h = (float)fmax(((double)TRIPLET_MARGIN + dp) - dn, 0.0);
  const float cp = h > 0.f && dp > 0.0 ? (float)((double)scale / dp) : 0.f, cn = h > 0.f && dn > 0.0 ? (float)((double)scale / dn) : 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = lane + 64 * u;
    if (c < g.C) p.gr[row * g.C + c] = cp * ep[u] - cn * en[u];
  }
  if (lane == 0) { p.cp[row] = cp; p.cn[row] = cn; p.hinge[row] = h; }
}

// grid (ceil(n / 4), B): a wave per tar column j: its own anchor's positive term, then every anchor that took it as its negative,
// in ascending anchor order
__global__ __launch_bounds__(256) void kd_tar_grad(Geo g, Plan p) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (j >= g.n) return;
  const size_t base = (size_t)b * g.n;
  const float* tj = p.t + (base + j) * g.C;
  float tv[4], acc[4];
  const float cpj = p.cp[base + j];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = lane + 64 * u;
    tv[u] = c < g.C ? tj[c] : 0.f;
    acc[u] = c < g.C ? -cpj * ((p.r[(base + j) * g.C + c] - tv[u]) + TRIPLET_EPS) : 0.f;
  }
  for (int i0 = 0; i0 < g.n; i0 += 64) {
    const int i = i0 + lane;
    const bool mine = i < g.n && p.neg[base + i] == j && p.cn[base + i] != 0.f;
    unsigned long long mask = __ballot(mine);
    while (mask) {
      const int q = i0 + __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const float cn = p.cn[base + q];
      const float* rq = p.r + (base + q) * g.C;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = lane + 64 * u;
        if (c < g.C) acc[u] += cn * ((rq[c] - tv[u]) + TRIPLET_EPS);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = lane + 64 * u;
    if (c < g.C) p.gt[(base + j) * g.C + c] = acc[u];
  }
}

// grid (ceil(n / 4), B, 2): y = x / (|x + eps| + eps): g <- g / D - (sum g x) / D^2 (x + eps) / s, in place
__global__ __launch_bounds__(256) void kd_norm_back(Geo g, Plan p) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (i >= g.n) return;
  const size_t row = ((size_t)b * g.n + i) * g.C;
  const float* x = (blockIdx.z ? p.xt : p.xr) + row;
  float* gy = (blockIdx.z ? p.gt : p.gr) + row;
  float xv[4], gv[4];
  double sq = 0.0, gx = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = lane + 64 * u;
    xv[u] = gv[u] = 0.f;
    if (c < g.C) {
      xv[u] = x[c];
      gv[u] = gy[c];
      const double e = (double)xv[u] + (double)DESC_EPS;
      sq += e * e;
      gx += (double)gv[u] * (double)xv[u];
    }
  }
  const double s = sqrt(wave_sum(sq)), D = s + (double)DESC_EPS;
  gx = wave_sum(gx);
  const double k = s > 0.0 ? gx / (D * D * s) : 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = lane + 64 * u;
    if (c < g.C) gy[c] = (float)((double)gv[u] / D - k * ((double)xv[u] + (double)DESC_EPS));
  }
}

__global__ __launch_bounds__(256) void kd_frame_sums(Geo g, Plan p) {
  __shared__ double s_d[4];
  __shared__ long long s_l[4];
  const int b = blockIdx.x;
  double h = 0.0;
  long long hit = 0;
  for (int i = threadIdx.x; i < g.n; i += 256) {
    h += (double)p.hinge[(size_t)b * g.n + i];
    hit += p.hit[(size_t)b * g.n + i];
  }
  h = block_sum(h, s_d);
  hit = block_sum(hit, s_l);
  if (threadIdx.x == 0) {
    p.fsum[(size_t)b * 6 + 4] = h;
    p.fcnt[(size_t)b * 2 + 1] = hit;
  }
}

// grid (ceil(Hf Wf / 256), B, 2): a thread per pixel of the descriptor map (z = 0 source, z = 1 target) scans the anchors
__global__ __launch_bounds__(256) void kd_feat_grad(Geo g, Plan p, float* __restrict__ dfeat_t, float* __restrict__ dfeat_s) {
  __shared__ float2 s_pix[256];
  __shared__ int s_x0[256], s_y0[256];
  const int px = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, HW = g.Hf * g.Wf;
  const bool tar = blockIdx.z == 1;
  const int y = px / g.Wf, x = px - y * g.Wf;
  float* out = (tar ? dfeat_t : dfeat_s) + (size_t)b * g.C * HW + px;
  const float* grad = (tar ? p.gt : p.gr) + (size_t)b * g.n * g.C;
  for (int i0 = 0; i0 < g.n; i0 += 256) {
    __syncthreads();
    const int i = i0 + threadIdx.x;
    if (i < g.n) {
      const int cell = anchor_cell(g, i);
      float2 nrm;
      if (tar) {
        nrm = p.wn[(size_t)b * g.N + cell];
      } else {
        const float2 c = p.cs[(size_t)b * g.N + cell];
        nrm = make_float2(c.x / g.sx - 1.f, c.y / g.sy - 1.f);
      }
      float fx, fy;
      tap(nrm.x, g.Wf, &fx, &s_x0[threadIdx.x]);
      tap(nrm.y, g.Hf, &fy, &s_y0[threadIdx.x]);
      s_pix[threadIdx.x] = make_float2(fx, fy);
    }
    __syncthreads();
    if (px >= HW) continue;
    const int m = g.n - i0 < 256 ? g.n - i0 : 256;
    for (int q = 0; q < m; ++q) {      // ascending anchor
      const int ex = x - s_x0[q], ey = y - s_y0[q];
      if ((unsigned)ex < 2u && (unsigned)ey < 2u) {
        const float2 pix = s_pix[q];
        const float wx = ex ? pix.x - (float)s_x0[q] : (float)(s_x0[q] + 1) - pix.x;
        const float wy = ey ? pix.y - (float)s_y0[q] : (float)(s_y0[q] + 1) - pix.y;
        const float wgt = wx * wy;
        const float* gq = grad + (size_t)(i0 + q) * g.C;
        for (int c = 0; c < g.C; ++c) out[(size_t)c * HW] += gq[c] * wgt;      // this thread owns the pixel
      }
    }
  }
}

__global__ __launch_bounds__(64) void kl_merge_b(Geo g, Weights wt, Plan p, float* __restrict__ loss, float* __restrict__ parts,
                                                 long long* __restrict__ counts) {
  if (threadIdx.x != 0) return;
  long long M = 0, hits = 0;
  double sc = 0.0, su = 0.0, metric = 0.0;
  for (int b = 0; b < g.B; ++b) {
    M += p.fcnt[(size_t)b * 2];
    sc += p.fsum[(size_t)b * 6 + 2];
    su += p.fsum[(size_t)b * 6 + 3];
    if (g.desc) {
      metric += p.fsum[(size_t)b * 6 + 4] / (double)g.n / (double)g.B;
      hits += p.fcnt[(size_t)b * 2 + 1];
    }
  }
  const double loc = p.coef[0], usp = su * p.coef[2];
  const double con = g.n > 0 ? 2.0 * sc / ((double)g.B * (double)g.n) : 0.0;
  parts[0] = (float)loc;
  parts[1] = (float)metric;
  parts[2] = (float)usp;
  parts[3] = (float)con;
  *loss = (float)(wt.all * (wt.loc * loc + wt.desc * 2.0 * metric + wt.score * usp + wt.score * con));
  counts[0] = M;
  counts[1] = g.desc ? g.n : 0;
  counts[2] = hits;
}

const char* shape_problem(int B, int Hc, int Wc, int C, int Hf, int Wf, int* code) {
  *code = KP2D_ERR_ARG;
  if (B < 1 || Hc < 1 || Wc < 1 || Hf < 1 || Wf < 1 || C < 1) return "every size must be at least 1";
  *code = KP2D_ERR_UNSUPPORTED;
  if (B > 65535) return "B above 65535";
  if ((long long)Hc * Wc > 65536) return "Hc * Wc above 65536";
  if (C % 16 || C < 16 || C > 256) return "C must be a multiple of 16 in [16, 256]";
  if ((long long)Hf * Wf > (1ll << 24)) return "Hf * Wf above 2^24";
  return nullptr;
}

Geo make_geo(int B, int Hc, int Wc, int C, int Hf, int Wf, int H, int W, int cell, double cross_ratio, double relax) {
  Geo g{};
  g.B = B; g.Hc = Hc; g.Wc = Wc; g.C = C; g.Hf = Hf; g.Wf = Wf;
  g.N = Hc * Wc;
  g.wi = Wc > 2 ? Wc - 2 : 0;
  g.n = Hc > 2 && Wc > 2 ? (Hc - 2) * (Wc - 2) : 0;
  g.desc = g.n >= MIN_ANCHORS;
  g.H1 = (float)(H - 1); g.W1 = (float)(W - 1);
  g.sx = (float)((double)(W - 1) / 2.0); g.sy = (float)((double)(H - 1) / 2.0);
  g.cell = (float)cell;
  g.step = (float)((cell - 1) / 2.0);
  g.reach = (float)(cross_ratio * ((cell - 1) / 2.0));
  g.relax = (float)relax;
  return g;
}

}  // namespace

extern "C" {

size_t kp2d_keypoint_loss_scratch_bytes(int B, int Hc, int Wc, int C, int Hf, int Wf) {
  int code;
  if (shape_problem(B, Hc, Wc, C, Hf, Wf, &code)) return 0;
  return make_plan(nullptr, make_geo(B, Hc, Wc, C, Hf, Wf, 2, 2, 2, 2.0, 4.0)).total;
}

int kp2d_keypoint_loss(const float* score_t, const float* shift_t, const float* feat_t, const float* score_s, const float* shift_s,
                       const float* feat_s, const float* homography, int B, int Hc, int Wc, int C, int Hf, int Wf, int H, int W,
                       int cell, double cross_ratio, double relax_field, double loc_weight, double descriptor_weight,
                       double score_weight, double keypoint_weight, float* loss, float* parts, float* dscore_t, float* dshift_t,
                       float* dfeat_t, float* dscore_s, float* dshift_s, float* dfeat_s, int64_t* counts, void* scratch,
                       size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = shape_problem(B, Hc, Wc, C, Hf, Wf, &code))
    return fail(code, "keypoint_loss: %s (B %d, cells %d x %d, C %d, feat %d x %d)", why, B, Hc, Wc, C, Hf, Wf);
  if (H < 2 || W < 2 || cell < 1) return fail(KP2D_ERR_ARG, "keypoint_loss: needs H, W >= 2 and cell >= 1 (got %d x %d, cell %d)", H, W, cell);
  for (double v : {cross_ratio, relax_field, loc_weight, descriptor_weight, score_weight, keypoint_weight})
    if (!(v >= 0.0 && v < INFINITY)) return fail(KP2D_ERR_ARG, "keypoint_loss: cross_ratio, relax_field and the weights must be finite and not negative");
  const void* ptrs[] = {score_t, shift_t, feat_t, score_s, shift_s, feat_s, homography, loss, parts, dscore_t, dshift_t, dfeat_t, dscore_s, dshift_s, dfeat_s};
  for (const void* q : ptrs) {
    if (!q) return fail(KP2D_ERR_ARG, "keypoint_loss: null argument");
    if (misaligned(q, 4)) return fail(KP2D_ERR_ARG, "keypoint_loss: misaligned argument");
  }
  if (!counts || !scratch || misaligned(counts, 8) || misaligned(scratch, 16)) return fail(KP2D_ERR_ARG, "keypoint_loss: null or misaligned counts / scratch");
  const Geo g = make_geo(B, Hc, Wc, C, Hf, Wf, H, W, cell, cross_ratio, relax_field);
  const Plan p = make_plan(scratch, g);
  if (scratch_bytes < p.total)
    return fail(KP2D_ERR_ARG, "keypoint_loss scratch %zu B < required %zu B (kp2d_keypoint_loss_scratch_bytes)", scratch_bytes, p.total);
  const Weights wt{loc_weight, descriptor_weight, score_weight, keypoint_weight};
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(score_t, st);
  const dim3 cells((g.N + 255) / 256, B), blk(256);
  hipLaunchKernelGGL(kl_decode, cells, blk, 0, st, g, shift_t, shift_s, homography, p);
  hipLaunchKernelGGL(kl_nearest, cells, blk, 0, st, g, p);
  hipLaunchKernelGGL(kl_sums, dim3(B), blk, 0, st, g, score_t, score_s, p);
  hipLaunchKernelGGL(kl_merge_a, dim3(1), dim3(64), 0, st, g, p);
  hipLaunchKernelGGL(kl_source_grad, dim3(B), blk, 0, st, g, wt, score_t, score_s, shift_s, p, dscore_s, dshift_s);
  hipLaunchKernelGGL(kl_target_grad, cells, blk, 0, st, g, shift_t, p, dscore_t, dshift_t);
  HIP_TRY(hipGetLastError());
  const size_t feat_bytes = (size_t)B * C * Hf * Wf * sizeof(float);
  HIP_TRY(hipMemsetAsync(dfeat_t, 0, feat_bytes, st));
  HIP_TRY(hipMemsetAsync(dfeat_s, 0, feat_bytes, st));
  if (g.desc) {
    const unsigned waves = (g.n + 3) / 4;
    const float scale = (float)(keypoint_weight * descriptor_weight * 2.0 / ((double)B * (double)g.n));
    hipLaunchKernelGGL(kd_sample, dim3(waves, B, 2), blk, 0, st, g, feat_t, feat_s, p);
    hipLaunchKernelGGL(kd_search, dim3((g.n + 63) / 64, B), blk, 0, st, g, p);
    hipLaunchKernelGGL(kd_hinge, dim3(waves, B), blk, 0, st, g, scale, p);
    hipLaunchKernelGGL(kd_tar_grad, dim3(waves, B), blk, 0, st, g, p);
    hipLaunchKernelGGL(kd_norm_back, dim3(waves, B, 2), blk, 0, st, g, p);
    hipLaunchKernelGGL(kd_frame_sums, dim3(B), blk, 0, st, g, p);
    hipLaunchKernelGGL(kd_feat_grad, dim3((Hf * Wf + 255) / 256, B, 2), blk, 0, st, g, p, dfeat_t, dfeat_s);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(kl_merge_b, dim3(1), dim3(64), 0, st, g, wt, p, loss, parts, (long long*)counts);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

}  // extern "C"
