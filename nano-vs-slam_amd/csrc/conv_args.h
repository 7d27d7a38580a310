// Launch arguments of the convolution kernels, without HIP: the tile-form policy (conv_policy.h) compiles with g++ too.
#pragma once

namespace kp2d {

// ---- activation / epilogue selectors -------------------------------------------------------
enum Act : int {
  ACT_NONE = 0,
  ACT_LEAKY = 1,           // LeakyReLU(0.01)       modules/base.py:33
  ACT_RELU = 2,            // ReLU (to_mcu configs) modules/base.py:35
  ACT_SIGMOID = 3,         // score head            models/kp2dtiny.py:574
  ACT_TANH = 4,            // loc head              models/kp2dtiny.py:575
  ACT_SIGMOID0_TANH = 5,   // V3 fused score/loc: ch0 sigmoid, ch1..2 tanh  models/kp2dtiny.py:927-935
  ACT_SOFTMAX_C = 6,       // V3 eval: Softmax2d over classes                models/kp2dtiny.py:942-943
  ACT_GELU = 7,            // exact-erf GELU inside MixFeedForward           modules/segformer.py:185
};

enum Store : int {
  ST_NHWC = 0,             // out0[pixel][os0] (+oo0), full resolution
  ST_NHWC_POOL = 1,        // out1 = MaxPool2d(2,2) of the activation only
  ST_NHWC_BOTH = 2,        // out0 full-res AND out1 pooled (conv3b: skip + x)
  ST_SHUFFLE = 3,          // PixelShuffle(2) folded into the store: out0 is the 2H x 2W NHWC tensor
  ST_NCHW = 4,             // API-facing planar output; channels [0,nsplit) -> out0, [nsplit,cout) -> out1
  ST_S16P = 5,             // out0 is an S16P tensor (below), full resolution
  ST_S16P_POOL = 6,        // out1 = MaxPool2d(2,2) of the activation as an S16P tensor (conv1b)
  ST_S16P_BOTH = 7,        // out0 full-res AND out1 pooled, both S16P tensors (conv3b: skip + x)
  ST_S16P_SHUFFLE = 8,     // PixelShuffle(2) folded into the store, out0 the 2H x 2W S16P tensor (cout / 4 a multiple of 32)
  ST_MIX16 = 9,            // 64-channel groups below channel `nsplit`: fp32 NHWC into out0 (os0 channels); from `nsplit` on: the
                           // S16P tensor out1 (os1 channels, its chunk 0 = channel nsplit) — the heads' merged first layer, whose
                           // score / location slices are read by the fp32 dot-product kernels and the rest by split-fp16 convs
  ST_IDS = 10,             // the layer's logits are NOT stored: only their per-pixel argmax, ids_out [B][H][W] int64 (out0 is left
                           // untouched).  conv3x3_s16.hip's ids-only form behind a 64-channel S16P tensor; no other kernel takes it
};
// S16P ("split, planar rows"): an activation kept as the fp16 halves the split-fp16 kernels multiply, x = hi + lo with
// hi = fp16(x), lo = fp16(x - hi) — per frame [C / 16 chunks][H][plane: hi | lo][W][16 halves], the same bytes as fp32 NHWC.
// A tile row of one plane is contiguous, so the consumer copies its LDS operand image straight from HBM (conv3x3_s16.hip).
// Only between layers of one forward (workspace tensors); C a multiple of 16.  Readers: conv3x3_s16.hip (32 input channels, the
// layer's weights resident in LDS) and conv3x3_wsm.hip's IN16 form (any whole number of chunks, one or two S16P sources).

// One 3x3 / stride 1 / pad 1 (taps = 9) or 1x1 (taps = 1) convolution over an NHWC activation that may be
// the channel-concat of two tensors (torch.cat([up, skip], 1): heads.py:99, segmentation.py:141,149).
// A source is addressed as ptr + b*bs + y*rs + x*ps + o + c, so strided views work too: the 2x2 stride-2
// to_kv conv (modules/segformer.py:93-95) is a 1x1 conv over two row-views of the full-resolution tensor.
struct ConvSrc { const float* p; int c, o; long bs, rs, ps; int fmt; };   // channels taken, first channel, strides (floats); fmt 1: an S16P tensor (bs only)
struct ConvArgs {
  ConvSrc in0, in1;
  int taps;                           // 9 or 1
  int prec;                           // 0: exact fp32 MFMA, 1: split-fp16 3xMFMA (weights packed as hi|lo halves)
  const float* w;                     // packed [group][cin_pad/KC][taps][ng][KC]
  const float* scale;                 // [npad]  BN: gamma/sqrt(var+eps); bias conv: 1
  const float* shift;                 // [npad]  BN: beta - mean*scale;   bias conv: bias
  float* out0; int os0, oo0;
  float* out1; int os1, oo1;
  int B, H, W;                        // conv resolution
  int cin, cout, npad;
  int act, store, nsplit;
  int tiles_x, tiles_y;
  int ng32;                           // 1: w holds 32-channel groups although npad >= 64 (small grids)
  int wsm_min;                        // least (tile, group) work items for the warp-specialised multi-chunk form; 0: automatic (conv_policy.h); < 0: never
  const float* w_tr;                  // the 64-channel-group pack with the taps transposed (dy <-> dx), nullptr: none (conv3x3_wsm.hip: transposed tiles)
  int wsm_tr;                         // conv3x3_wsm.hip: tiles walk the map transposed (tile rows = map columns).  In: 0 never, 1 always, 2 where cheaper; the launcher hands the kernel its decision (0 / 1)
  int wsm_lanes;                      // stream lanes launching side by side (the form takes CUs / lanes workgroups)
  long long* ids_out;                 // ST_NCHW, one channel group: also write argmax over the stored channels per pixel, [B][H][W] int64 (nullptr: no); ST_IDS: the only output
  int ws_min;                         // least tiles for the warp-specialised conv1b form (0: 1024)
  int wsm_grid;                       // most workgroups per launch of the persistent forms; 0: automatic (conv_policy.h)
  // conv1b's warp-specialised form with conv1a computed by its staging waves (conv3x3_f16.hip STEM): the frames [B,3,H,W] and
  // conv1a's weights [27][16] / folded BatchNorm; in0 is then unused.  nullptr: conv1a is its own launch
  const float* stem_x; const float* stem_w; const float* stem_scale; const float* stem_shift; const float* stem_wscale; int stem_act;   // stem_wscale: device pointer to 2^e
  int s16_min;                        // conv3x3_s16.hip: least work items for the form (0: automatic, three rounds per workgroup)
  int wsm_force;                      // the plan fixed this layer's tensor layouts on conv3x3_wsm.hip running it (S16P in or out): no item-count policy
  int dbg;                            // timing ablations only (KP2D_DBG): 1 skip the epilogue, 2 skip LDS commit, 4 skip global loads, 8 skip MFMA, 64 skip only the epilogue's global stores
};

}  // namespace kp2d
