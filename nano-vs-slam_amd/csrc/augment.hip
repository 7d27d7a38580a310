// View pairs on the device (include/kp2d.h): what the reference's dataset transforms do between "a batch of frames" and
// "image, image_aug, seg, seg_aug, depth, depth_aug, homography" (src/data/dataset_utils.py:9-136, :198-266, nyuv2.py:183-257),
// and the one loss term that needs the warp (KeypointNetwithIOLoss.py:587-603).
//
//   kp2d_homography_draws   hd_draws_kernel   a thread per (frame, slot): the nine draws of a frame from the library's counter
//                                             stream (mix64.h), uniforms and Box-Muller normals in double
//   kp2d_homography_sample  hs_sample_kernel  a thread per frame: sample_homography in double, the 8 x 8 system by elimination
//                                             with partial pivoting
//   kp2d_warp               wp_forward_kernel a thread per OUTPUT pixel, a workgroup per tile of TILE_H rows x TILE_W columns: the
//                                             coordinates once (src_coords, double, unfused), then the channels.  Stores are
//                                             coalesced along the row.  The loads are a gather, but a smooth one: the 64
//                                             outputs of a row of the tile read sources that lie along one line of the source
//                                             map, about a pixel apart, and the tile's next row reads the line next to it, so a
//                                             tile touches a few hundred bytes around a quadrilateral of the source plane; the
//                                             lines it shares with its neighbours stay in L2 (a 240 x 320 fp32 plane is 300 KB).
//   kp2d_warp_backward      wp_backward_kernel a thread per SOURCE pixel p: the receiving side scans.  The four corners of
//                                             [p - 1/2 - g, p + 1/2 + g]^2 go through the frame's inverse homography (formed in
//                                             double by the workgroup's first thread), their bounding box in output pixels is
//                                             widened by one and clamped, and every candidate q of the box is tested with the
//                                             forward's own nearest_src; the hits are added in ascending row-major order in
//                                             fp32.  A corner with inverse w' <= 0, or a singular or non-finite matrix, makes
//                                             that thread scan the whole output: slow and correct.
//   kp2d_cross_view_mse     cv_sums_kernel    the pixels (frame-major) in chunks of 1024, the chunks in at most 1024 runs: a
//                                             chunk's sum of diff^2 is a float64 butterfly over the wave and the four waves in
//                                             wave order, a run adds its chunks in chunk order
//                           cv_merge_kernel   one thread: the runs in run order -> loss, inside, the gradient's coefficient
//                           cv_grad_kernel    a thread per pixel: d_depth_aug; then wp_backward_kernel on it, negated: d_depth
// No float atomics; every order depends on the shapes alone: all outputs are bit-identical from run to run.
//
// The coordinate arithmetic must round exactly as the numpy oracle's does, operation by operation.  hipcc's round-to-nearest
// intrinsics are plain operators and its default contraction would fuse a product into the sum it feeds, so contraction is
// switched off for this whole file.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "api_common.h"
#include "device_guard.h"
#include "mix64.h"
#include "train_common.h"

using namespace kp2d;

namespace {

constexpr int TILE_W = 64, TILE_H = 4;      // a workgroup's pixels: 4 rows of 64 (KP2D_WARP_TILE_W / _H)
constexpr int MAX_EXTENT = 32768;           // H, W
constexpr int MAX_CHANNELS = 4096;
constexpr int BACK_CH = 4;                  // channels a backward thread accumulates per scan of its box
constexpr double BACK_GUARD = 1.0 / 64.0;   // g
constexpr int LP = 1024;                    // pixels of a chunk of the cross-view sum: four per thread
constexpr int MAX_RUNS = 1024;
constexpr int SLOTS = KP2D_HOMOGRAPHY_DRAWS;

static_assert(TILE_W == KP2D_WARP_TILE_W && TILE_H == KP2D_WARP_TILE_H, "the header states the tile");

struct Hom {
  double m[9];
};

__device__ __forceinline__ Hom load_hom(const void* hom, int f64, int n) {
  Hom h;
#pragma unroll
  for (int k = 0; k < 9; ++k) h.m[k] = f64 ? ((const double*)hom)[(size_t)n * 9 + k] : (double)((const float*)hom)[(size_t)n * 9 + k];
  return h;
}

// THE coordinate map (include/kp2d.h): pixel (X, Y) of the full-size H x W grid -> (px, py) in source pixels.
__device__ __forceinline__ void src_coords(const Hom& h, int X, int Y, int H, int W, double* px, double* py) {
  const double wm = (double)(W - 1), hm = (double)(H - 1);
  const double gx = __dadd_rn(__ddiv_rn(__dmul_rn(2.0, (double)X), wm), -1.0);
  const double gy = __dadd_rn(__ddiv_rn(__dmul_rn(2.0, (double)Y), hm), -1.0);
  const double u = __dadd_rn(__dadd_rn(__dmul_rn(h.m[0], gx), __dmul_rn(h.m[1], gy)), h.m[2]);
  const double v = __dadd_rn(__dadd_rn(__dmul_rn(h.m[3], gx), __dmul_rn(h.m[4], gy)), h.m[5]);
  const double w = __dadd_rn(__dadd_rn(__dmul_rn(h.m[6], gx), __dmul_rn(h.m[7], gy)), h.m[8]);
  *px = __dmul_rn(__ddiv_rn(__dadd_rn(__ddiv_rn(u, w), 1.0), 2.0), wm);
  *py = __dmul_rn(__ddiv_rn(__dadd_rn(__ddiv_rn(v, w), 1.0), 2.0), hm);
}

// the nearest source pixel of (X, Y), ties to even; false: outside (a non-finite coordinate is outside)
__device__ __forceinline__ bool nearest_src(const Hom& h, int X, int Y, int H, int W, int* xi, int* yi) {
  double px, py;
  src_coords(h, X, Y, H, W, &px, &py);
  const double rx = rint(px), ry = rint(py);
  if (!(rx >= 0.0 && rx <= (double)(W - 1) && ry >= 0.0 && ry <= (double)(H - 1))) return false;
  *xi = (int)rx;
  *yi = (int)ry;
  return true;
}

// ---- the forward warp --------------------------------------------------------------------------------------------------------
template <typename T, bool BILINEAR>
__global__ __launch_bounds__(TILE_W* TILE_H) void wp_forward_kernel(const T* __restrict__ src, const void* __restrict__ hom, int hom_f64,
                                                                     int C, int H, int W, int Ho, int Wo, int stride, T fill,
                                                                     T* __restrict__ dst) {
  const int j = blockIdx.x * TILE_W + (threadIdx.x % TILE_W), i = blockIdx.y * TILE_H + (threadIdx.x / TILE_W), n = blockIdx.z;
  if (i >= Ho || j >= Wo) return;
  const Hom h = load_hom(hom, hom_f64, n);
  const size_t plane = (size_t)H * W, oplane = (size_t)Ho * Wo;
  const T* s = src + (size_t)n * C * plane;
  T* d = dst + (size_t)n * C * oplane + (size_t)i * Wo + j;
  if constexpr (!BILINEAR) {
    int xi = 0, yi = 0;
    const bool in = nearest_src(h, j * stride, i * stride, H, W, &xi, &yi);
    const size_t at = (size_t)yi * W + xi;
    for (int c = 0; c < C; ++c) d[(size_t)c * oplane] = in ? s[(size_t)c * plane + at] : fill;
  } else {
    double px, py;
    src_coords(h, j * stride, i * stride, H, W, &px, &py);
    const double x0 = floor(px), y0 = floor(py);
    const double fx = __dadd_rn(px, -x0), fy = __dadd_rn(py, -y0);
    const double gx = __dadd_rn(1.0, -fx), gy = __dadd_rn(1.0, -fy);
    // a tap is live when its column and row exist; a non-finite coordinate has no live tap
    const bool cx0 = x0 >= 0.0 && x0 <= (double)(W - 1), cx1 = x0 >= -1.0 && x0 <= (double)(W - 2);
    const bool cy0 = y0 >= 0.0 && y0 <= (double)(H - 1), cy1 = y0 >= -1.0 && y0 <= (double)(H - 2);
    const bool t00 = cx0 && cy0, t01 = cx1 && cy0, t10 = cx0 && cy1, t11 = cx1 && cy1;
    const float w00 = t00 ? (float)__dmul_rn(gx, gy) : 0.f, w01 = t01 ? (float)__dmul_rn(fx, gy) : 0.f;
    const float w10 = t10 ? (float)__dmul_rn(gx, fy) : 0.f, w11 = t11 ? (float)__dmul_rn(fx, fy) : 0.f;
    const long long xa = (cx0 || cx1) ? (long long)x0 : 0, ya = (cy0 || cy1) ? (long long)y0 : 0;
    const size_t o00 = t00 ? (size_t)(ya * W + xa) : 0, o01 = t01 ? (size_t)(ya * W + xa + 1) : 0;
    const size_t o10 = t10 ? (size_t)((ya + 1) * W + xa) : 0, o11 = t11 ? (size_t)((ya + 1) * W + xa + 1) : 0;
    for (int c = 0; c < C; ++c) {
      const T* p = s + (size_t)c * plane;
      const float a = t00 ? (float)p[o00] : 0.f, b = t01 ? (float)p[o01] : 0.f, e = t10 ? (float)p[o10] : 0.f, f = t11 ? (float)p[o11] : 0.f;
      d[(size_t)c * oplane] = (T)__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w00, a), __fmul_rn(w01, b)), __fmul_rn(w10, e)), __fmul_rn(w11, f));
    }
  }
}

// ---- the nearest warp's backward -------------------------------------------------------------------------------------------------
// inverse of the frame's matrix as adjugate / determinant in double; false: singular or not finite
__device__ inline bool invert3(const Hom& h, double* inv) {
  const double* m = h.m;
  const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
  if (!(fabs(det) > 0.0) || !isfinite(det)) return false;
  inv[0] = c0 / det;
  inv[1] = (m[2] * m[7] - m[1] * m[8]) / det;
  inv[2] = (m[1] * m[5] - m[2] * m[4]) / det;
  inv[3] = c1 / det;
  inv[4] = (m[0] * m[8] - m[2] * m[6]) / det;
  inv[5] = (m[2] * m[3] - m[0] * m[5]) / det;
  inv[6] = c2 / det;
  inv[7] = (m[1] * m[6] - m[0] * m[7]) / det;
  inv[8] = (m[0] * m[4] - m[1] * m[3]) / det;
  bool ok = true;
  for (int k = 0; k < 9; ++k) ok = ok && isfinite(inv[k]);
  return ok;
}

// dx = scale * (the ordered fp32 sum); scale is 1 or -1, so it rounds nothing
__global__ __launch_bounds__(TILE_W* TILE_H) void wp_backward_kernel(const float* __restrict__ dy, const void* __restrict__ hom, int hom_f64,
                                                                      int C, int H, int W, int Ho, int Wo, int stride, float scale,
                                                                      float* __restrict__ dx) {
  __shared__ double s_inv[9];
  __shared__ int s_ok;
  const int n = blockIdx.z;
  const Hom h = load_hom(hom, hom_f64, n);
  if (threadIdx.x == 0) {
    double inv[9];
    s_ok = invert3(h, inv) ? 1 : 0;
    for (int k = 0; k < 9; ++k) s_inv[k] = s_ok ? inv[k] : 0.0;
  }
  __syncthreads();
  const int xp = blockIdx.x * TILE_W + (threadIdx.x % TILE_W), yp = blockIdx.y * TILE_H + (threadIdx.x / TILE_W);
  if (yp >= H || xp >= W) return;
  // the candidates: rows [i0, i1], columns [j0, j1] of the output
  int i0 = 0, i1 = Ho - 1, j0 = 0, j1 = Wo - 1;
  bool boxed = s_ok != 0;
  if (boxed) {
    double lo_x = INFINITY, hi_x = -INFINITY, lo_y = INFINITY, hi_y = -INFINITY;
    const double wm = (double)(W - 1), hm = (double)(H - 1);
    for (int k = 0; k < 4; ++k) {
      const double cx = (double)xp + ((k & 1) ? 0.5 + BACK_GUARD : -0.5 - BACK_GUARD);
      const double cy = (double)yp + ((k & 2) ? 0.5 + BACK_GUARD : -0.5 - BACK_GUARD);
      const double u = 2.0 * cx / wm - 1.0, v = 2.0 * cy / hm - 1.0;
      const double qx = s_inv[0] * u + s_inv[1] * v + s_inv[2], qy = s_inv[3] * u + s_inv[4] * v + s_inv[5];
      const double qw = s_inv[6] * u + s_inv[7] * v + s_inv[8];
      if (!(qw > 0.0)) boxed = false;
      const double X = (qx / qw + 1.0) * 0.5 * wm / (double)stride, Y = (qy / qw + 1.0) * 0.5 * hm / (double)stride;   // in output pixels
      if (!isfinite(X) || !isfinite(Y)) boxed = false;
      lo_x = fmin(lo_x, X);
      hi_x = fmax(hi_x, X);
      lo_y = fmin(lo_y, Y);
      hi_y = fmax(hi_y, Y);
    }
    if (boxed) {
      // clamped as doubles first: a far-away box must not overflow the conversion; an empty range scans nothing
      j0 = (int)fmin(fmax(floor(lo_x) - 1.0, 0.0), (double)Wo);
      i0 = (int)fmin(fmax(floor(lo_y) - 1.0, 0.0), (double)Ho);
      j1 = (int)fmax(fmin(ceil(hi_x) + 1.0, (double)(Wo - 1)), -1.0);
      i1 = (int)fmax(fmin(ceil(hi_y) + 1.0, (double)(Ho - 1)), -1.0);
    }
  }
  const size_t plane = (size_t)H * W, oplane = (size_t)Ho * Wo;
  const float* g = dy + (size_t)n * C * oplane;
  float* out = dx + (size_t)n * C * plane + (size_t)yp * W + xp;
  for (int c0 = 0; c0 < C; c0 += BACK_CH) {
    float acc[BACK_CH] = {0.f, 0.f, 0.f, 0.f};
    for (int i = i0; i <= i1; ++i)
      for (int j = j0; j <= j1; ++j) {
        int xi, yi;
        if (nearest_src(h, j * stride, i * stride, H, W, &xi, &yi) && xi == xp && yi == yp) {
#pragma unroll
          for (int k = 0; k < BACK_CH; ++k)
            if (c0 + k < C) acc[k] = __fadd_rn(acc[k], g[(size_t)(c0 + k) * oplane + (size_t)i * Wo + j]);
        }
      }
#pragma unroll
    for (int k = 0; k < BACK_CH; ++k)
      if (c0 + k < C) out[(size_t)(c0 + k) * plane] = scale * acc[k];
  }
}

// ---- the sampler ------------------------------------------------------------------------------------------------------------------
// the draw of kp2d_homography_draws (include/kp2d.h states the counter layout)
__host__ __device__ inline uint64_t hom_draw(uint64_t seed, uint32_t step, uint32_t frame, uint32_t slot, uint32_t k) {
  return km_mix(km_mix(km_mix(seed + 0x9E3779B97F4A7C15ull) ^ (((uint64_t)step << 32) | frame)) ^ (((uint64_t)slot << 32) | k));
}

__global__ __launch_bounds__(256) void hd_draws_kernel(double* __restrict__ draws, int B, uint64_t seed, uint32_t step) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)B * SLOTS) return;
  const uint32_t frame = (uint32_t)(e / SLOTS), slot = (uint32_t)(e % SLOTS);
  const double ua = (double)(hom_draw(seed, step, frame, slot, 0) >> 11) * 0x1p-53;
  const bool normal = slot < 4 || slot == 5;
  double out = ua;
  if (normal) {
    const double ub = (double)(hom_draw(seed, step, frame, slot, 1) >> 11) * 0x1p-53;
    out = sqrt(-2.0 * log(1.0 - ua)) * cos(6.283185307179586 * ub);
  }
  draws[e] = out;
}

struct SampleArgs {
  int H, W, perspective, scaling, rotation, translation, n_scales, n_angles;
  double scaling_amplitude, perspective_amplitude, patch_ratio, max_angle;
};

__device__ __forceinline__ double clip(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

__global__ __launch_bounds__(64) void hs_sample_kernel(const double* __restrict__ draws, int B, SampleArgs a, double* __restrict__ hom64,
                                                       float* __restrict__ hom32) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const double* d = draws + (size_t)b * SLOTS;
  const double hw = (double)a.H / (double)a.W;
  const double p1[4][2] = {{-1.0, -1.0}, {-1.0, 1.0}, {1.0, -1.0}, {1.0, 1.0}};
  double p2[4][2];
  for (int i = 0; i < 4; ++i) {
    p2[i][0] = p1[i][0] * a.patch_ratio;
    p2[i][1] = p1[i][1] * a.patch_ratio * hw;
  }
  if (a.perspective) {
    const double sx = a.perspective_amplitude / 2, sy = hw * a.perspective_amplitude / 2;
    const double ax0 = clip(sx * d[0], -sx, sx), ax1 = clip(sx * d[1], -sx, sx);
    const double ay0 = clip(sy * d[2], -sy, sy), ay1 = clip(sy * d[3], -sy, sy);
    p2[0][0] -= ax1; p2[0][1] -= ay1;
    p2[1][0] -= ax0; p2[1][1] += ay1;
    p2[2][0] += ax1; p2[2][1] -= ay0;
    p2[3][0] += ax0; p2[3][1] += ay0;
  }
  if (a.scaling) {
    int idx = (int)floor(d[4] * (double)a.n_scales);
    idx = idx < 0 ? 0 : idx > a.n_scales - 1 ? a.n_scales - 1 : idx;     // the reference's range: its last draw is never picked
    const double s = idx == 0 ? 1.0 : clip(1.0 + d[5] * (a.scaling_amplitude / 2), 1.0 - a.scaling_amplitude / 2, 1.0 + a.scaling_amplitude / 2);
    const double cx = (((p2[0][0] + p2[1][0]) + p2[2][0]) + p2[3][0]) / 4, cy = (((p2[0][1] + p2[1][1]) + p2[2][1]) + p2[3][1]) / 4;
    for (int i = 0; i < 4; ++i) {
      p2[i][0] = (p2[i][0] - cx) * s + cx;
      p2[i][1] = (p2[i][1] - cy) * s + cy;
    }
  }
  if (a.translation) {
    double tmin[2] = {INFINITY, INFINITY}, tmax[2] = {INFINITY, INFINITY};
    const double lim[2] = {1.0, hw};
    for (int i = 0; i < 4; ++i)
      for (int k = 0; k < 2; ++k) {
        tmin[k] = fmin(tmin[k], p2[i][k] + lim[k]);
        tmax[k] = fmin(tmax[k], lim[k] - p2[i][k]);
      }
    for (int k = 0; k < 2; ++k) {
      const double t = -tmin[k] + (tmax[k] + tmin[k]) * d[6 + k];
      for (int i = 0; i < 4; ++i) p2[i][k] += t;
    }
  }
  if (a.rotation) {
    const double cx = (((p2[0][0] + p2[1][0]) + p2[2][0]) + p2[3][0]) / 4, cy = (((p2[0][1] + p2[1][1]) + p2[2][1]) + p2[3][1]) / 4;
    const double step = a.n_angles > 1 ? (2.0 * a.max_angle) / (double)(a.n_angles - 1) : 0.0;
    // candidate 0 is the angle 0; candidate k >= 1 is numpy's linspace(-max_angle, max_angle, n_angles)[k - 1]
    auto angle = [&](int k) { return k == 0 ? 0.0 : k == a.n_angles && a.n_angles > 1 ? a.max_angle : -a.max_angle + (double)(k - 1) * step; };
    auto rotate = [&](int k, double out[4][2]) {
      const double ang = angle(k), c = cos(ang), s = sin(ang);
      bool ok = true;
      for (int i = 0; i < 4; ++i) {
        const double x = p2[i][0] - cx, y = p2[i][1] - cy;
        out[i][0] = (x * c + y * s) + cx;
        out[i][1] = (y * c - x * s) + cy;
        ok = ok && out[i][0] >= -1.0 && out[i][0] < 1.0 && out[i][1] >= -hw && out[i][1] < hw;
      }
      return ok;
    };
    double r[4][2];
    int valid = 0;
    for (int k = 0; k <= a.n_angles; ++k) valid += rotate(k, r) ? 1 : 0;
    if (valid > 0) {          // (none valid: the reference raises; here the view stays unrotated)
      int pick = (int)floor(d[8] * (double)valid);
      pick = pick < 0 ? 0 : pick > valid - 1 ? valid - 1 : pick;
      for (int k = 0; k <= a.n_angles; ++k)
        if (rotate(k, r) && pick-- == 0) {
          for (int i = 0; i < 4; ++i) { p2[i][0] = r[i][0]; p2[i][1] = r[i][1]; }
          break;
        }
    }
  }
  for (int i = 0; i < 4; ++i) p2[i][1] /= hw;
  // the 8 x 8 system [A | p]: rows ax, ay of the four point pairs; elimination with partial pivoting
  double m[8][9];
  for (int i = 0; i < 4; ++i) {
    const double px = p1[i][0], py = p1[i][1], qx = p2[i][0], qy = p2[i][1];
    const double rx[9] = {px, py, 1.0, 0.0, 0.0, 0.0, -px * qx, -py * qx, qx};
    const double ry[9] = {0.0, 0.0, 0.0, px, py, 1.0, -px * qy, -py * qy, qy};
    for (int k = 0; k < 9; ++k) { m[2 * i][k] = rx[k]; m[2 * i + 1][k] = ry[k]; }
  }
  for (int col = 0; col < 8; ++col) {
    int piv = col;
    for (int r = col + 1; r < 8; ++r)
      if (fabs(m[r][col]) > fabs(m[piv][col])) piv = r;
    for (int k = 0; k < 9; ++k) { const double t = m[col][k]; m[col][k] = m[piv][k]; m[piv][k] = t; }
    for (int r = col + 1; r < 8; ++r) {
      const double f = m[r][col] / m[col][col];
      for (int k = col; k < 9; ++k) m[r][k] -= f * m[col][k];
    }
  }
  double x[9];
  for (int r = 7; r >= 0; --r) {
    double s = m[r][8];
    for (int k = r + 1; k < 8; ++k) s -= m[r][k] * x[k];
    x[r] = s / m[r][r];
  }
  x[8] = 1.0;
  for (int k = 0; k < 9; ++k) {
    if (hom64) hom64[(size_t)b * 9 + k] = x[k];
    if (hom32) hom32[(size_t)b * 9 + k] = (float)x[k];
  }
}

// ---- the cross-view depth term ----------------------------------------------------------------------------------------------------
struct CrossGeo {
  long long total, chunks, cpr;     // pixels, chunks, chunks per run
  int runs;
};

CrossGeo cross_geo(int N, int64_t HW) {
  CrossGeo g{};
  g.total = (long long)N * HW;
  g.chunks = (g.total + LP - 1) / LP;
  g.cpr = (g.chunks + MAX_RUNS - 1) / MAX_RUNS;
  g.runs = (int)((g.chunks + g.cpr - 1) / g.cpr);
  return g;
}

struct CrossPlan {
  double* part;        // [runs]: sum of diff^2 over the counted pixels
  long long* cnt;      // [runs]: inside pixels
  double* coef;        // [1]: weight 2 / M
  size_t total;
};

CrossPlan cross_plan(void* scratch, int N, int64_t HW) {
  CrossPlan p{};
  Carve c(scratch);
  const CrossGeo g = cross_geo(N, HW);
  p.part = c.take<double>((size_t)g.runs);
  p.cnt = c.take<long long>((size_t)g.runs);
  p.coef = c.take<double>(1);
  p.total = c.bytes();
  return p;
}

// pixel gp of [N, H, W] -> diff = depth_aug - warp(depth, H) (outside: warp = 0); returns inside
__device__ __forceinline__ bool cross_diff(const float* depth, const float* depth_aug, const void* hom, int hom_f64, int H, int W,
                                           long long gp, float* diff) {
  const long long hw = (long long)H * W;
  const int n = (int)(gp / hw), r = (int)(gp % hw);
  const Hom h = load_hom(hom, hom_f64, n);
  int xi, yi;
  const bool in = nearest_src(h, r % W, r / W, H, W, &xi, &yi);
  const float warped = in ? depth[(size_t)n * hw + (size_t)yi * W + xi] : 0.f;
  *diff = __fsub_rn(depth_aug[gp], warped);
  return in;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(256) void cv_sums_kernel(const float* __restrict__ depth, const float* __restrict__ depth_aug,
                                                      const void* __restrict__ hom, int hom_f64, int H, int W, int inside_only,
                                                      CrossGeo geo, double* __restrict__ part, long long* __restrict__ cnt) {
  __shared__ double s_sum[4];
  __shared__ int s_in[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double run = 0.0;                 // thread 0's: the run so far
  long long run_in = 0;
  const long long q_end = ((long long)blockIdx.x + 1) * geo.cpr < geo.chunks ? ((long long)blockIdx.x + 1) * geo.cpr : geo.chunks;
  for (long long q = (long long)blockIdx.x * geo.cpr; q < q_end; ++q) {
    double s = 0.0;
    int in_n = 0;
#pragma unroll
    for (int i = 0; i < LP / 256; ++i) {
      const long long gp = q * LP + tid + 256 * i;
      if (gp < geo.total) {
        float diff;
        const bool in = cross_diff(depth, depth_aug, hom, hom_f64, H, W, gp, &diff);
        in_n += in ? 1 : 0;
        if (in || !inside_only) s += (double)diff * (double)diff;
      }
    }
    s = wave_sum(s);
    for (int o = 32; o > 0; o >>= 1) in_n += __shfl_xor(in_n, o);
    __syncthreads();              // the previous chunk's sums have been read
    if (lane == 0) { s_sum[wave] = s; s_in[wave] = in_n; }
    __syncthreads();
    if (tid == 0) {
      run += (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
      run_in += (long long)((s_in[0] + s_in[1]) + (s_in[2] + s_in[3]));
    }
  }
  if (tid == 0) {
    part[blockIdx.x] = run;
    cnt[blockIdx.x] = run_in;
  }
}

__global__ __launch_bounds__(64) void cv_merge_kernel(const double* __restrict__ part, const long long* __restrict__ cnt, int runs,
                                                      long long total, double weight, int inside_only, double* __restrict__ coef,
                                                      float* __restrict__ loss, long long* __restrict__ inside) {
  if (threadIdx.x != 0) return;
  double S = 0.0;
  long long in = 0;
  for (int r = 0; r < runs; ++r) {
    S += part[r];
    in += cnt[r];
  }
  const long long M = inside_only ? in : total;
  *loss = M > 0 ? (float)(weight * S / (double)M) : 0.f;
  *coef = M > 0 ? weight * 2.0 / (double)M : 0.0;
  *inside = in;
}

__global__ __launch_bounds__(256) void cv_grad_kernel(const float* __restrict__ depth, const float* __restrict__ depth_aug,
                                                      const void* __restrict__ hom, int hom_f64, int H, int W, int inside_only,
                                                      long long total, const double* __restrict__ coef, float* __restrict__ d_aug) {
  const double k = *coef;
  for (long long gp = (long long)blockIdx.x * 256 + threadIdx.x; gp < total; gp += (long long)gridDim.x * 256) {
    float diff;
    const bool in = cross_diff(depth, depth_aug, hom, hom_f64, H, W, gp, &diff);
    d_aug[gp] = (in || !inside_only) ? (float)(k * (double)diff) : 0.f;
  }
}

// ---- host: shapes ------------------------------------------------------------------------------------------------------------------
const char* warp_shape_problem(int N, int C, int H, int W, int stride, int* code) {
  *code = KP2D_ERR_ARG;
  if (N < 1 || N > 65535) return "N outside [1, 65535]";
  if (C < 1) return "C must be at least 1";
  if (H < 2 || W < 2) return "H and W must be at least 2";
  if (stride < 1 || H % stride || W % stride) return "the stride must be positive and divide H and W";
  *code = KP2D_ERR_UNSUPPORTED;
  if (H > MAX_EXTENT || W > MAX_EXTENT) return "H or W above 32768";
  if (C > MAX_CHANNELS) return "C above 4096";
  return nullptr;
}

dim3 tile_grid(int N, int H, int W) { return dim3((W + TILE_W - 1) / TILE_W, (H + TILE_H - 1) / TILE_H, N); }

template <typename T>
int launch_forward(const void* src, const void* hom, int hom_f64, int N, int C, int H, int W, int stride, int mode, double fill, void* dst,
                   hipStream_t st) {
  const int Ho = H / stride, Wo = W / stride;
  if (mode == KP2D_WARP_BILINEAR) {
    if constexpr (std::is_same<T, float>::value)
      hipLaunchKernelGGL((wp_forward_kernel<float, true>), tile_grid(N, Ho, Wo), dim3(TILE_W * TILE_H), 0, st, (const float*)src, hom, hom_f64, C,
                         H, W, Ho, Wo, stride, 0.f, (float*)dst);
  } else {
    hipLaunchKernelGGL((wp_forward_kernel<T, false>), tile_grid(N, Ho, Wo), dim3(TILE_W * TILE_H), 0, st, (const T*)src, hom, hom_f64, C, H, W,
                       Ho, Wo, stride, (T)fill, (T*)dst);
  }
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

}  // namespace

extern "C" {

int kp2d_homography_draws(double* draws, int B, uint64_t seed, int64_t step, void* stream) {
  if (B < 1) return fail(KP2D_ERR_ARG, "homography_draws: B %d must be at least 1", B);
  if (step < 0 || step > (int64_t)UINT32_MAX) return fail(KP2D_ERR_ARG, "homography_draws: step %lld outside [0, 2^32)", (long long)step);
  if (!draws) return fail(KP2D_ERR_ARG, "null argument");
  if (misaligned(draws, 8)) return fail(KP2D_ERR_ARG, "homography_draws: draws must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(draws, st);
  const long long total = (long long)B * SLOTS;
  hipLaunchKernelGGL(hd_draws_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, draws, B, seed, (uint32_t)step);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_homography_sample(const double* draws, int B, int H, int W, int perspective, int scaling, int rotation, int translation,
                           int n_scales, int n_angles, double scaling_amplitude, double perspective_amplitude, double patch_ratio,
                           double max_angle, double* hom64, float* hom32, void* stream) {
  if (B < 1 || H < 1 || W < 1) return fail(KP2D_ERR_ARG, "homography_sample: B %d, H %d, W %d must be at least 1", B, H, W);
  if (n_scales < 1 || n_angles < 1 || n_angles > 65536)
    return fail(KP2D_ERR_ARG, "homography_sample: n_scales %d must be at least 1 and n_angles %d in [1, 65536]", n_scales, n_angles);
  if (!(scaling_amplitude >= 0.0 && scaling_amplitude < 2.0 && perspective_amplitude >= 0.0 && perspective_amplitude < INFINITY &&
        patch_ratio > 0.0 && patch_ratio <= 1.0 && max_angle >= 0.0 && max_angle < INFINITY))
    return fail(KP2D_ERR_ARG, "homography_sample: needs 0 <= scaling_amplitude < 2, perspective_amplitude >= 0, 0 < patch_ratio <= 1, max_angle >= 0");
  if (!draws || (!hom64 && !hom32)) return fail(KP2D_ERR_ARG, "null argument");
  if (misaligned(draws, 8) || misaligned(hom64, 8) || misaligned(hom32, 4)) return fail(KP2D_ERR_ARG, "homography_sample: misaligned argument");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(draws, st);
  const SampleArgs a{H, W, perspective, scaling, rotation, translation, n_scales, n_angles, scaling_amplitude, perspective_amplitude, patch_ratio,
                     max_angle};
  hipLaunchKernelGGL(hs_sample_kernel, dim3((B + 63) / 64), dim3(64), 0, st, draws, B, a, hom64, hom32);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

int kp2d_warp(const void* src, int dtype, const void* hom, int hom_f64, int N, int C, int H, int W, int stride, int mode, double fill,
              void* dst, void* stream) {
  int code;
  if (const char* why = warp_shape_problem(N, C, H, W, stride, &code))
    return fail(code, "warp: %s (N %d, C %d, H %d, W %d, stride %d)", why, N, C, H, W, stride);
  if (dtype < KP2D_WARP_F32 || dtype > KP2D_WARP_I64) return fail(KP2D_ERR_ARG, "warp: dtype %d is none of KP2D_WARP_F32 / U8 / I32 / I64", dtype);
  if (mode != KP2D_WARP_NEAREST && mode != KP2D_WARP_BILINEAR) return fail(KP2D_ERR_ARG, "warp: mode %d is neither nearest nor bilinear", mode);
  if (mode == KP2D_WARP_BILINEAR && dtype != KP2D_WARP_F32) return fail(KP2D_ERR_ARG, "warp: bilinear takes float32 sources only");
  const double lo[4] = {-INFINITY, 0.0, -2147483648.0, -9007199254740992.0}, hi[4] = {INFINITY, 255.0, 2147483647.0, 9007199254740992.0};
  if (dtype == KP2D_WARP_F32 ? std::isnan(fill) : !(fill >= lo[dtype] && fill <= hi[dtype] && fill == std::floor(fill)))
    return fail(KP2D_ERR_ARG, "warp: fill %g is not a value of the source's type", fill);
  if (any_null(src, hom, dst)) return fail(KP2D_ERR_ARG, "null argument");
  const size_t esize[4] = {4, 1, 4, 8};
  if (misaligned(src, esize[dtype]) || misaligned(dst, esize[dtype]) || misaligned(hom, hom_f64 ? 8 : 4))
    return fail(KP2D_ERR_ARG, "warp: misaligned argument");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(src, st);
  switch (dtype) {
    case KP2D_WARP_F32: return launch_forward<float>(src, hom, hom_f64, N, C, H, W, stride, mode, fill, dst, st);
    case KP2D_WARP_U8: return launch_forward<uint8_t>(src, hom, hom_f64, N, C, H, W, stride, mode, fill, dst, st);
    case KP2D_WARP_I32: return launch_forward<int32_t>(src, hom, hom_f64, N, C, H, W, stride, mode, fill, dst, st);
    default: return launch_forward<int64_t>(src, hom, hom_f64, N, C, H, W, stride, mode, fill, dst, st);
  }
}

int kp2d_warp_backward(const float* dy, const void* hom, int hom_f64, int N, int C, int H, int W, int stride, float* dx, void* stream) {
  int code;
  if (const char* why = warp_shape_problem(N, C, H, W, stride, &code))
    return fail(code, "warp_backward: %s (N %d, C %d, H %d, W %d, stride %d)", why, N, C, H, W, stride);
  if (any_null(dy, hom, dx)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(dy, dx) || misaligned(hom, hom_f64 ? 8 : 4)) return fail(KP2D_ERR_ARG, "warp_backward: misaligned argument");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(dy, st);
  hipLaunchKernelGGL(wp_backward_kernel, tile_grid(N, H, W), dim3(TILE_W * TILE_H), 0, st, dy, hom, hom_f64, C, H, W, H / stride, W / stride,
                     stride, 1.f, dx);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

size_t kp2d_cross_view_scratch_bytes(int N, int64_t HW) {
  if (N < 1 || N > 65535 || HW < 4 || HW > (int64_t)MAX_EXTENT * MAX_EXTENT) return 0;
  return cross_plan(nullptr, N, HW).total;
}

int kp2d_cross_view_mse(const float* depth, const float* depth_aug, const void* hom, int hom_f64, int N, int H, int W, double weight,
                        int inside_only, float* loss, float* d_depth, float* d_depth_aug, int64_t* inside, void* scratch,
                        size_t scratch_bytes, void* stream) {
  int code;
  if (const char* why = warp_shape_problem(N, 1, H, W, 1, &code)) return fail(code, "cross_view_mse: %s (N %d, H %d, W %d)", why, N, H, W);
  if (!(weight >= 0.0 && weight < INFINITY)) return fail(KP2D_ERR_ARG, "cross_view_mse: weight %g must be finite and not negative", weight);
  if (any_null(depth, depth_aug, hom, loss, d_depth, d_depth_aug, inside, scratch)) return fail(KP2D_ERR_ARG, "null argument");
  if (any_misaligned4(depth, depth_aug, loss, d_depth, d_depth_aug) || misaligned(hom, hom_f64 ? 8 : 4) || misaligned(inside, 8) ||
      misaligned(scratch, 16))
    return fail(KP2D_ERR_ARG, "cross_view_mse: misaligned argument");
  const int64_t HW = (int64_t)H * W;
  const CrossPlan p = cross_plan(scratch, N, HW);
  if (scratch_bytes < p.total)
    return fail(KP2D_ERR_ARG, "cross_view_mse scratch %zu B < required %zu B (kp2d_cross_view_scratch_bytes)", scratch_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard guard(depth, st);
  const CrossGeo g = cross_geo(N, HW);
  hipLaunchKernelGGL(cv_sums_kernel, dim3(g.runs), dim3(256), 0, st, depth, depth_aug, hom, hom_f64, H, W, inside_only, g, p.part, p.cnt);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(cv_merge_kernel, dim3(1), dim3(64), 0, st, p.part, p.cnt, g.runs, g.total, weight, inside_only, p.coef, loss,
                     (long long*)inside);
  HIP_TRY(hipGetLastError());
  const long long need = (g.total + 255) / 256, blocks = need < (1 << 20) ? need : (1 << 20);
  hipLaunchKernelGGL(cv_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, st, depth, depth_aug, hom, hom_f64, H, W, inside_only, g.total,
                     p.coef, d_depth_aug);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(wp_backward_kernel, tile_grid(N, H, W), dim3(TILE_W * TILE_H), 0, st, d_depth_aug, hom, hom_f64, 1, H, W, H, W, 1, -1.f,
                     d_depth);
  HIP_TRY(hipGetLastError());
  return KP2D_OK;
}

}  // extern "C"
