// The three convolution-shaped products of the training kernels (vpr_head_train.hip, seg_train.hip): a 3x3 convolution
// (stride 1, padding 1) forward, its data gradient and its weight gradient as implicit GEMMs on v_mfma_f32_16x16x4_f32
// (exact fp32, bit for bit an fma chain); an output tile is 8 rows x 16 columns of the map.
//   hc_pack_kernel      w [Cout][Cin][3][3] -> [cin][tap][cout] as hc_conv_kernel stages it; the data gradient's form swaps
//                       the channel axes and turns the taps by 180 degrees, so dx is the forward kernel run on dc
//   hc_conv_kernel      grid (tiles, N): A = weights [16 cout][4 cin], B = input [4 cin][16 pixels of a row]; a wave owns two
//                       rows of the tile and every output channel; K = 9 Cin walked as chunks of 16 input channels staged in
//                       LDS (halo tile 16 x 10 x 18, weight slab 16 x 9 x Cout); epilogue: c and y, or the plain result
//   hc_dw_kernel        grid (slabs, Cin / 16): A = dc [16 cout][4 pixels], B = x shifted by the tap [4 pixels][16 cin]; a slab
//                       is a fixed run of tiles (at most 128 slabs), accumulated in registers, one partial per slab
//   hc_dw_sum_kernel    the slabs' partials added in slab order
// MASK = true (seg_train.hip's last layer) takes a channel count that is no multiple of 16 on w's Cout axis: the packed
// weights are padded with zeros to the next multiple of 16 (hc_pack_pad_kernel), a padded channel is staged as exact zeros
// without a load and is never stored; the epilogue adds a bias.  MASK = false is the kernel as it always was.
// Host side, for the entry points of both files: conv_shape_problem (what N, H, W, Cin, Cout the kernels take), conv_forward
// (pack the weights, convolve) and conv_backward_tail (weight gradient, and on request the data gradient).
// Every kernel lives in an anonymous namespace: each translation unit that includes this header gets its own copies.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "api_common.h"
#include "device_guard.h"
#include "train_common.h"

namespace {

using namespace kp2d;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TH = 8, TW = 16;              // output tile: 8 rows (two per wave) x 16 columns (one MFMA N / K run)
constexpr int HR = TH + 2, HC = TW + 2;     // halo tile
constexpr int KC = 16;                      // input channels per chunk
constexpr int MIN_CH = 16, MAX_CH = 128;
constexpr int MAX_SLABS = 128;
// LDS pitches in floats.  hc_conv_kernel: a wave's read is 16 consecutive pixels (or channels) for each of 4 input
// channels: a channel pitch of 16 mod 64 spreads them over all 64 banks (halo plane 180 -> 208; weight rows Cout | 16,
// whose 9-row channel stride is 16 or 48 mod 64).  hc_dw_kernel: 16 channels for each of 4 consecutive pixels: 4 mod 64.
constexpr int IN_P = 208;
constexpr int DW_DP = TH * TW + 4, DW_XP = 196;
static_assert(IN_P >= HR * HC && IN_P % 64 == 16 && DW_XP >= HR * HC && DW_XP % 64 == 4 && DW_DP % 64 == 4, "LDS pitches");
__host__ __device__ constexpr int cout_pitch(int co) { return co | 16; }
__host__ __device__ constexpr int pad16(int c) { return (c + 15) & ~15; }
constexpr size_t conv_lds_bytes(int co) { return (size_t)(KC * IN_P + KC * 9 * cout_pitch(co)) * sizeof(float); }
constexpr size_t dw_lds_bytes(int co) { return (size_t)(co * DW_DP + KC * DW_XP) * sizeof(float); }
static_assert(conv_lds_bytes(MAX_CH) == 96256 && dw_lds_bytes(MAX_CH) == 80128, "largest LDS images (of 160 KB)");

// ---- weights as the conv kernel stages them ---------------------------------------------------------------------------
// forward: wp[(ci 9 + t) Cout + co] = w[co][ci][t].  data gradient (its input channels are w's Cout, its output channels
// w's Cin): wp[(co 9 + t) Cin + ci] = w[co][ci][8 - t].
__global__ __launch_bounds__(256) void hc_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin, int dgrad) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= Cout * Cin * 9) return;
  const int t = e % 9, ci = (e / 9) % Cin, co = e / (9 * Cin);
  if (dgrad) wp[(co * 9 + (8 - t)) * Cin + ci] = w[e];
  else wp[(ci * 9 + t) * Cout + co] = w[e];
}

// the same two forms with w's Cout axis padded to CP = pad16(Cout): every one of the 9 Cin CP entries is written, the
// padded ones with 0, whatever the buffer held
__global__ __launch_bounds__(256) void hc_pack_pad_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin, int dgrad) {
  const int CP = pad16(Cout);
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= CP * Cin * 9) return;
  int co, ci, t;
  if (dgrad) { ci = e % Cin; t = 8 - (e / Cin) % 9; co = e / (9 * Cin); }
  else { co = e % CP; t = (e / CP) % 9; ci = e / (9 * CP); }
  wp[e] = co < Cout ? w[((size_t)co * Cin + ci) * 9 + t] : 0.f;
}

struct ConvA {
  const float* in;      // [N][CI][H][W]
  const float* wp;      // [CI][9][CO]
  const float* scale;   // [CO], or null: plain result into y_out
  const float* shift;   // [CO]
  float* c_out;         // [N][CO][H][W] conv result before the affine, or null
  float* y_out;         // [N][CO][H][W]
  int CI, H, W, tiles_x;
  float slope;
};

// the MASK form's arguments: the channels that exist (in: ci_real of pad16(ci_real) = CI; out: co_real of 16 NT), the bias or
// null.  A type of its own, so that the MASK = false kernels keep the argument block they always had.
struct ConvMA : ConvA {
  int ci_real, co_real;
  const float* bias;
};
template <bool MASK>
using ConvArgs = std::conditional_t<MASK, ConvMA, ConvA>;

template <int NT, bool MASK>      // CO = 16 NT output channels
__global__ __launch_bounds__(256) void hc_conv_kernel(const ConvArgs<MASK> a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int CO = NT * 16, COP = cout_pitch(CO);
  float* s_in = sm;                 // [KC][IN_P]: plane c holds the 10 x 18 halo tile
  float* s_w = sm + KC * IN_P;      // [KC * 9][COP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, k = lane >> 4;
  const int H = a.H, W = a.W;
  const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x, b = blockIdx.y;
  const int y0 = ty * TH, x0 = tx * TW;
  const size_t HW = (size_t)H * W;
  int ci_real = a.CI, co_real = CO;
  if constexpr (MASK) { ci_real = a.ci_real; co_real = a.co_real; }
  const float* inb = a.in + (size_t)b * ci_real * HW;

  f32x4 acc[2][NT];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunk = a.CI / KC;
  for (int ch = 0; ch < nchunk; ++ch) {
    __syncthreads();                // every wave is done with the previous chunk's images
    for (int e = tid; e < KC * HR * HC; e += 256) {
      const int c = e / (HR * HC), r = e - c * (HR * HC);
      const int py = r / HC, px = r - py * HC;
      const int gy = y0 - 1 + py, gx = x0 - 1 + px;
      float v = 0.f;                // the zero padding, the pixels of a ragged tile past the map, a padded channel
      if (gy >= 0 && gy < H && gx >= 0 && gx < W && (!MASK || ch * KC + c < ci_real))
        v = inb[(size_t)(ch * KC + c) * HW + (size_t)gy * W + gx];
      s_in[c * IN_P + r] = v;
    }
    const float* wsrc = a.wp + (size_t)ch * KC * 9 * CO;
    for (int e = tid; e < KC * 9 * CO; e += 256) {
      const int row = e / CO, col = e - row * CO;
      s_w[row * COP + col] = wsrc[e];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dy = t / 3, dx = t - 3 * (t / 3);
#pragma unroll
      for (int kk = 0; kk < KC / 4; ++kk) {
        const int ci = 4 * kk + k;
        float bv[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) bv[m] = s_in[ci * IN_P + (2 * wave + m + dy) * HC + j + dx];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const float av = s_w[(ci * 9 + t) * COP + n * 16 + j];
#pragma unroll
          for (int m = 0; m < 2; ++m) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[m], acc[m][n], 0, 0, 0);
        }
      }
    }
  }
  // accumulator register r of lane (j, k): output channel 16 n + 4 k + r at pixel (y0 + 2 wave + m, x0 + j)
  const int x = x0 + j;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int y = y0 + 2 * wave + m;
    if (y >= H || x >= W) continue;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = 16 * n + 4 * k + r;
        if (MASK && co >= co_real) continue;
        const size_t idx = ((size_t)b * co_real + co) * HW + (size_t)y * W + x;
        const float c = acc[m][n][r];
        if constexpr (MASK) {
          a.y_out[idx] = a.bias ? c + a.bias[co] : c;
          continue;
        }
        if (a.c_out) a.c_out[idx] = c;
        float v = c;
        if (a.scale) {
          v = fmaf(c, a.scale[co], a.shift[co]);
          v = v > 0.f ? v : a.slope * v;
        }
        a.y_out[idx] = v;
      }
  }
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------
struct DwA {
  const float* dc;      // [N][CO][H][W]
  const float* x;       // [N][CI][H][W]
  float* part;          // [slabs][CO][CI][9]
  long long tiles, tps; // all tiles (frame-major), tiles per slab
  int CI, H, W, tiles_x, tpf;
};
struct DwMA : DwA {
  int co_real;          // dc's channels, of 16 NT
};
template <bool MASK>
using DwArgs = std::conditional_t<MASK, DwMA, DwA>;

template <int NT, bool MASK>      // CO = 16 NT
__global__ __launch_bounds__(256) void hc_dw_kernel(const DwArgs<MASK> a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int CO = NT * 16, UNITS = 3 * NT, MAXU = (UNITS + 3) / 4;      // a unit: (16 output channels, tap row), 3 taps
  float* s_dc = sm;                 // [CO][DW_DP]: the 8 x 16 tile of dc
  float* s_x = sm + CO * DW_DP;     // [KC][DW_XP]: the 10 x 18 halo tile of this workgroup's 16 input channels
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, k = lane >> 4;
  const int H = a.H, W = a.W, chunk = blockIdx.y;
  const size_t HW = (size_t)H * W;
  int co_real = CO;
  if constexpr (MASK) co_real = a.co_real;

  f32x4 acc[MAXU][3];
#pragma unroll
  for (int it = 0; it < MAXU; ++it)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) acc[it][kx] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long long t_begin = (long long)blockIdx.x * a.tps;
  const long long t_end = t_begin + a.tps < a.tiles ? t_begin + a.tps : a.tiles;
  for (long long tile = t_begin; tile < t_end; ++tile) {
    const int b = (int)(tile / a.tpf), rem = (int)(tile - (long long)b * a.tpf);
    const int ty = rem / a.tiles_x, tx = rem - ty * a.tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    const float* dcb = a.dc + (size_t)b * co_real * HW;
    const float* xb = a.x + ((size_t)b * a.CI + (size_t)chunk * KC) * HW;
    __syncthreads();
    for (int e = tid; e < CO * TH * TW; e += 256) {
      const int co = e >> 7, r = e & 127;
      const int gy = y0 + (r >> 4), gx = x0 + (r & 15);
      s_dc[co * DW_DP + r] = (gy < H && gx < W && (!MASK || co < co_real)) ? dcb[(size_t)co * HW + (size_t)gy * W + gx] : 0.f;
    }
    for (int e = tid; e < KC * HR * HC; e += 256) {
      const int c = e / (HR * HC), r = e - c * (HR * HC);
      const int py = r / HC, px = r - py * HC;
      const int gy = y0 - 1 + py, gx = x0 - 1 + px;
      float v = 0.f;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xb[(size_t)c * HW + (size_t)gy * W + gx];
      s_x[c * DW_XP + r] = v;
    }
    __syncthreads();
    for (int s = 0; s < TH * TW / 4; ++s) {       // four pixels of a tile row per step, in pixel order
      const int yy = s >> 2, xx = 4 * (s & 3) + k;
#pragma unroll
      for (int it = 0; it < MAXU; ++it) {
        const int u = wave + 4 * it;
        if (u < UNITS) {
          const int n = u / 3, ky = u - 3 * n;
          const float av = s_dc[(16 * n + j) * DW_DP + yy * TW + xx];
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float bv = s_x[j * DW_XP + (yy + ky) * HC + xx + kx];
            acc[it][kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[it][kx], 0, 0, 0);
          }
        }
      }
    }
  }
  // register r of lane (j, k): output channel 16 n + 4 k + r, input channel 16 chunk + j
  float* dst = a.part + (size_t)blockIdx.x * co_real * a.CI * 9;
#pragma unroll
  for (int it = 0; it < MAXU; ++it) {
    const int u = wave + 4 * it;
    if (u < UNITS) {
      const int n = u / 3, ky = u - 3 * n;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (MASK && 16 * n + 4 * k + r >= co_real) continue;
          dst[((size_t)(16 * n + 4 * k + r) * a.CI + chunk * KC + j) * 9 + ky * 3 + kx] = acc[it][kx][r];
        }
    }
  }
}

__global__ __launch_bounds__(256) void hc_dw_sum_kernel(const float* __restrict__ part, float* __restrict__ dw, int slabs, int n) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) dw[e] = ordered_sum(part + e, (size_t)n, slabs);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct Geo {
  int tiles_x, tiles_y, tpf, slabs;
  long long tiles, tps;
};

inline Geo geo_of(int N, int H, int W) {
  Geo g{};
  g.tiles_x = (W + TW - 1) / TW;
  g.tiles_y = (H + TH - 1) / TH;
  g.tpf = g.tiles_x * g.tiles_y;
  g.tiles = (long long)N * g.tpf;
  g.tps = (g.tiles + MAX_SLABS - 1) / MAX_SLABS;
  g.slabs = (int)((g.tiles + g.tps - 1) / g.tps);
  return g;
}

// why the kernels do not take these sizes (*code: the entry point's return value), or null.  cout16: a layer with a BatchNorm,
// Cout a multiple of 16 in [16, 128]; otherwise the MASK form's any 1 <= Cout <= 128
inline const char* conv_shape_problem(int N, int H, int W, int Cin, int Cout, bool cout16, int* code) {
  *code = KP2D_ERR_ARG;
  if (N < 1 || N > 65535) return "N outside [1, 65535]";
  if (H < 1 || W < 1) return "H and W must be at least 1";
  if (Cin < 1 || Cout < 1) return "Cin and Cout must be at least 1";
  *code = KP2D_ERR_UNSUPPORTED;
  if (Cin % 16 || Cin < MIN_CH || Cin > MAX_CH || Cout > MAX_CH || (cout16 && (Cout % 16 || Cout < MIN_CH)))
    return cout16 ? "needs Cin % 16 == 0, Cout % 16 == 0 and 16 <= Cin, Cout <= 128" : "needs Cin % 16 == 0, 16 <= Cin <= 128 and 1 <= Cout <= 128";
  if ((int64_t)H * W > ((int64_t)1 << 30)) return "H * W above 2^30";
  return nullptr;
}

template <int NT, bool MASK>
int launch_conv_t(const ConvArgs<MASK>& a, const dim3& grid, hipStream_t st) {
  static PerDeviceOnce once;
  if (int e = lds_opt_in(once, reinterpret_cast<const void*>(&hc_conv_kernel<NT, MASK>))) return e;
  hipLaunchKernelGGL((hc_conv_kernel<NT, MASK>), grid, dim3(256), conv_lds_bytes(NT * 16), st, a);
  return (int)hipGetLastError();
}

// CO: the output channels, a multiple of 16 (MASK: padded)
template <bool MASK>
int launch_conv(const ConvArgs<MASK>& a, int CO, int N, const Geo& g, hipStream_t st) {
  const dim3 grid(g.tpf, N);
  switch (CO / 16) {
    case 1: return launch_conv_t<1, MASK>(a, grid, st);
    case 2: return launch_conv_t<2, MASK>(a, grid, st);
    case 3: return launch_conv_t<3, MASK>(a, grid, st);
    case 4: return launch_conv_t<4, MASK>(a, grid, st);
    case 5: return launch_conv_t<5, MASK>(a, grid, st);
    case 6: return launch_conv_t<6, MASK>(a, grid, st);
    case 7: return launch_conv_t<7, MASK>(a, grid, st);
    case 8: return launch_conv_t<8, MASK>(a, grid, st);
  }
  return -1000;
}

template <int NT, bool MASK>
int launch_dw_t(const DwArgs<MASK>& a, const dim3& grid, hipStream_t st) {
  static PerDeviceOnce once;
  if (int e = lds_opt_in(once, reinterpret_cast<const void*>(&hc_dw_kernel<NT, MASK>))) return e;
  hipLaunchKernelGGL((hc_dw_kernel<NT, MASK>), grid, dim3(256), dw_lds_bytes(NT * 16), st, a);
  return (int)hipGetLastError();
}

template <bool MASK>
int launch_dw(const DwArgs<MASK>& a, int CO, const Geo& g, hipStream_t st) {
  const dim3 grid(g.slabs, a.CI / KC);
  switch (CO / 16) {
    case 1: return launch_dw_t<1, MASK>(a, grid, st);
    case 2: return launch_dw_t<2, MASK>(a, grid, st);
    case 3: return launch_dw_t<3, MASK>(a, grid, st);
    case 4: return launch_dw_t<4, MASK>(a, grid, st);
    case 5: return launch_dw_t<5, MASK>(a, grid, st);
    case 6: return launch_dw_t<6, MASK>(a, grid, st);
    case 7: return launch_dw_t<7, MASK>(a, grid, st);
    case 8: return launch_dw_t<8, MASK>(a, grid, st);
  }
  return -1000;
}

// ---- the two halves of a conv-shaped entry point -----------------------------------------------------------------------
struct ConvCall {
  const char* who;      // the entry point's name in its messages
  const float* x;       // [N][Cin][H][W]
  const float* w;       // [Cout][Cin][3][3]
  float* wp;            // scratch of 9 Cin Cout floats (MASK: Cout padded to 16) for the packed weights
  int N, H, W, Cin, Cout;
  hipStream_t st;
};

// w in the form hc_conv_kernel stages: dgrad 0 the forward's, 1 the data gradient's
template <bool MASK>
void launch_pack(const ConvCall& k, int dgrad) {
  const dim3 grid(((MASK ? pad16(k.Cout) : k.Cout) * k.Cin * 9 + 255) / 256);
  if constexpr (MASK) hipLaunchKernelGGL(hc_pack_pad_kernel, grid, dim3(256), 0, k.st, k.w, k.wp, k.Cout, k.Cin, dgrad);
  else hipLaunchKernelGGL(hc_pack_kernel, grid, dim3(256), 0, k.st, k.w, k.wp, k.Cout, k.Cin, dgrad);
}

// pack, then convolve x.  `a` brings the epilogue (scale, shift, slope, c_out, y_out; MASK: bias); the rest is filled in here
template <bool MASK>
int conv_forward(const ConvCall& k, ConvArgs<MASK> a) {
  const Geo g = geo_of(k.N, k.H, k.W);
  launch_pack<MASK>(k, 0);
  HIP_TRY(hipGetLastError());
  a.in = k.x; a.wp = k.wp; a.CI = k.Cin; a.H = k.H; a.W = k.W; a.tiles_x = g.tiles_x;
  if constexpr (MASK) { a.ci_real = k.Cin; a.co_real = k.Cout; }
  if (int e = launch_conv<MASK>(a, MASK ? pad16(k.Cout) : k.Cout, k.N, g, k.st)) return fail(KP2D_ERR_HIP, "%s: conv kernel: %d", k.who, e);
  return KP2D_OK;
}

// from dc [N][Cout][H][W], the gradient of the convolution's result: the weight gradient's partials per slab (dwp), their
// ordered sum into d_weight, and with dx the forward kernel on dc (input channels Cout, MASK: padded and masked; output
// channels Cin; the weights turned and swapped).  d_weight has the same bits with and without dx.
template <bool MASK>
int conv_backward_tail(const ConvCall& k, const float* dc, float* dwp, float* d_weight, float* dx) {
  const Geo g = geo_of(k.N, k.H, k.W);
  const int CP = MASK ? pad16(k.Cout) : k.Cout;
  DwArgs<MASK> d{};
  d.dc = dc; d.x = k.x; d.part = dwp; d.tiles = g.tiles; d.tps = g.tps; d.CI = k.Cin; d.H = k.H; d.W = k.W; d.tiles_x = g.tiles_x; d.tpf = g.tpf;
  if constexpr (MASK) d.co_real = k.Cout;
  if (int e = launch_dw<MASK>(d, CP, g, k.st)) return fail(KP2D_ERR_HIP, "%s: weight-gradient kernel: %d", k.who, e);
  const int nw = k.Cout * k.Cin * 9;
  hipLaunchKernelGGL(hc_dw_sum_kernel, dim3((nw + 255) / 256), dim3(256), 0, k.st, dwp, d_weight, g.slabs, nw);
  HIP_TRY(hipGetLastError());
  if (!dx) return KP2D_OK;
  launch_pack<MASK>(k, 1);
  HIP_TRY(hipGetLastError());
  ConvArgs<MASK> a{};
  a.in = dc; a.wp = k.wp; a.y_out = dx; a.CI = CP; a.H = k.H; a.W = k.W; a.tiles_x = g.tiles_x;
  if constexpr (MASK) { a.ci_real = k.Cout; a.co_real = k.Cin; }
  if (int e = launch_conv<MASK>(a, k.Cin, k.N, g, k.st)) return fail(KP2D_ERR_HIP, "%s: data-gradient kernel: %d", k.who, e);
  return KP2D_OK;
}

}  // namespace
