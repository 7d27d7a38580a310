// The device side of a LightGlue handle and the launch sequence of one forward (lightglue_plan.cpp); the C ABI around them is
// lightglue_api.cpp.
#pragma once
#include "lightglue_desc.h"

struct kp2d_lg : kp2d::LgDesc {
  float* blob = nullptr;
  bool finalized = false;
};

namespace kp2d {

// outputs and threshold of point pruning (kp2d_lg_forward_pruned); null: every point stays through all layers
struct PruneIO {
  float thr;
  int32_t *keep0, *keep1, *nkeep0, *nkeep1;
  int64_t *prune0, *prune1;
};

// the launch sequence of one forward (lightglue.py:484-614)
int run_forward(kp2d_lg* m, const float* kpts0, const float* kpts1, const float* desc0, const float* desc1,
                const float* size0, const float* size1, const int32_t* n0, const int32_t* n1, int B, int M, int N,
                float filter_threshold, float* log_assignment, int64_t* matches0, int64_t* matches1,
                float* mscores0, float* mscores1, float* ref_desc0, float* ref_desc1, const PruneIO* pr, void* workspace,
                size_t workspace_bytes, void* stream);

}  // namespace kp2d
