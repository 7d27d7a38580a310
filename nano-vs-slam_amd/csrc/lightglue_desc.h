// The host-only part of a LightGlue handle: its configuration, the state-dict tensors it consumes, the packed linear layers and
// where each sits in the weight blob, and the workspace walk of a forward.  No HIP: lightglue_desc.cpp compiles with g++
// (tests/test_lightglue_desc.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/kp2d_lightglue.h"
#include "weight_table.h"

namespace kp2d {

// one packed linear layer: W^T [K][nout] then bias [nout] (nout padded to a multiple of 32)
// mf: the same matrix as split-fp16 matrix-core operand tiles (mfma_image), K * nout * 4 bytes, when K % 32 == 0
struct Lin { size_t w = 0, b = 0, mf = 0; int K = 0, nout = 0; };
struct Ffn { Lin l0, l3; size_t g = 0, be = 0; };
struct Layer { Lin qkv, out_proj, qkv_x, to_out; Ffn fs, fc; };

struct LgDesc {
  kp2d_lg_config cfg{};
  std::vector<WeightSpec> specs;
  std::map<std::string, int> index;
  std::map<std::string, std::vector<float>> host;
  std::vector<Layer> layers;
  Lin input_proj, final;
  std::vector<size_t> prune_w;      // matchability of layers 0 .. n-2 (point pruning): weight [d] then the bias
  size_t wr = 0, blob_floats = 0;
};

// cfg set: the widths this build has kernels for, then specs, the packed layers and the blob layout.  KP2D_OK, or the error
// (kp2d_last_error() says what).
int describe(LgDesc* m);
// every tensor of `specs` present in `host`: the blob the kernels read, blob_floats floats
int pack(const LgDesc* m, std::vector<float>& blob);

// workspace of a forward, every piece on an ALIGN boundary
struct Ws {
  float *x, *t3, *ctx, *msg, *hb, *cs, *fz;
  float *rp_m, *rp_s, *cp_m, *cp_s, *rmax, *cmax;     // per-tile partials of the assignment (LgAssignArgs)
  int *rarg, *carg;
  int32_t* cnt;                                       // [n0 | n1]: key counts of the 2B sequences (kp2d_lg_forward_counts)
  size_t total;
};
Ws layout(void* workspace, const LgDesc* m, int B, int M, int N);

}  // namespace kp2d
