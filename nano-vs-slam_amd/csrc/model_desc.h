// The host-only part of a model: its configuration, the state-dict tensors it consumes, the packed layers and where each
// sits in the weight blob.  No HIP: model_desc.cpp compiles with g++ (tests/test_model_desc.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/kp2d.h"
#include "weight_table.h"

namespace kp2d {

// one packed 3x3 convolution
struct ConvPack {
  std::string name;     // state-dict prefix, e.g. "backbone.conv2a"
  bool bn = false;      // AnnotatedConvBnReLUModel (conv.weight + bn.*) vs plain Conv2d (weight + bias)
  bool shuffle = false; // rows permuted for the PixelShuffle-folding store
  bool bias = true;     // plain conv only: has a .bias tensor
  bool tconv = false;   // TransposedConvUpsampleModel (base.py:80-117) restated as a pixel-shuffled 3x3 conv (add_tconv)
  int kind = 0;         // 0: 3x3 [co][ci][3][3]   1: 1x1 [co][ci][1][1]   2: 2x2 stride 2 [co][ci][2][2] as 1x1 over 4*ci
  std::vector<std::pair<std::string, int>> parts;   // merged CBRs over one input (name, cout): rows = the parts' rows in order
  int taps = 9;
  int cin = 0, cout = 0, npad = 0, kc = 16;   // cin = GEMM K per tap (4*ci for kind 2)
  size_t w_off = 0, sc_off = 0, sh_off = 0;   // float offsets into the blob
  size_t w16_off = 0, sc16_off = 0;           // split-fp16 pack: [hi16|lo16] half rows of w * 2^e, scale * 2^-e (pack())
  size_t w16n_off = 0;                        // the same rows in 32-channel groups (npad >= 64): small-grid launches
  size_t w16t_off = 0;                        // the 64-channel-group rows with the taps transposed (3x3, npad >= 64): transposed tiles of conv3x3_wsm.hip
  size_t wd_off = 0;                          // head layers (3x3, <= 4 output channels): fp32 [chunk][tap][4][16] for head3x3.hip
  bool head() const { return kind == 0 && cout <= 4 && !shuffle && !tconv && parts.empty(); }
  size_t wd_floats() const { return (size_t)((cin + 15) / 16) * 9 * 4 * 16; }
  size_t w_floats() const { return (size_t)((cin + kc - 1) / kc) * taps * npad * kc; }
  size_t w16_floats() const { return (size_t)((cin + 15) / 16) * taps * npad * 16; }
};

struct VecPack { size_t off = 0; int n = 0; };   // small per-channel vectors (LayerNorm g/b, depthwise w/b)

struct ModelDesc {
  kp2d_config cfg{};
  int c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, d1 = 0;   // cfg.channel_dims (describe())
  std::vector<WeightSpec> specs;
  std::map<std::string, int> spec_index;
  std::map<std::string, std::vector<float>> host;   // what kp2d_set_weight received, by key
  std::vector<ConvPack> convs;
  std::map<std::string, int> conv_index;
  std::map<std::string, VecPack> vecs;
  size_t conv1a_w = 0, conv1a_sc = 0, conv1a_sh = 0;
  size_t conv1a_ws = 0;       // blob offset of 2^e, the scale conv1a's weights are split at (pack(); in the blob, so that it travels with an RCCL weight broadcast)
  size_t vlad_wa = 0, vlad_cent = 0;
  size_t blob_floats = 0;
  const ConvPack* conv(const std::string& name) const {   // null: the model has no such layer
    const auto it = conv_index.find(name);
    return it == conv_index.end() ? nullptr : &convs[it->second];
  }
};

// cfg set: fill c1 .. d1, specs, convs, vecs and the blob layout.  KP2D_OK, or the error (kp2d_last_error() says what).
int describe(ModelDesc* m);
// every tensor of `specs` present in `host`: the blob the kernels read, blob_floats floats
int pack(const ModelDesc* m, std::vector<float>& blob);

}  // namespace kp2d
