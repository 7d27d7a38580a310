// The C ABI of include/kp2d_lightglue.h: every entry point checks its arguments and hands over to the matcher's description
// (lightglue_desc.cpp), the weight table (weight_table.h / weight_upload.h) or the launch sequence (lightglue_plan.cpp).
#include "../../include/kp2d_lightglue.h"

#include <hip/hip_runtime.h>

#include <vector>

#include "api_common.h"
#include "lightglue_plan.h"
#include "weight_upload.h"

using namespace kp2d;

extern "C" {

int kp2d_lg_create(const kp2d_lg_config* cfg, kp2d_lg** out) {
  if (!cfg || !out) return fail(KP2D_ERR_ARG, "null argument");
  if (cfg->struct_size != (int32_t)sizeof(kp2d_lg_config)) return fail(KP2D_ERR_ARG, "kp2d_lg_config.struct_size mismatch");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(KP2D_ERR_HIP, "no HIP device visible: this library has no CPU path");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(KP2D_ERR_ARG, "device %d out of range (%d visible)", cfg->device, ndev);
  auto* m = new kp2d_lg();
  m->cfg = *cfg;
  const int rc = describe(m);      // (refuses the widths the kernels are not built for)
  if (rc != KP2D_OK) { delete m; return rc; }
  *out = m;
  return KP2D_OK;
}

void kp2d_lg_destroy(kp2d_lg* m) {
  if (!m) return;
  if (m->blob) (void)hipFree(m->blob);
  delete m;
}

int kp2d_lg_num_weights(const kp2d_lg* m) { return m ? (int)m->specs.size() : 0; }

int kp2d_lg_weight_info(const kp2d_lg* m, int index, const char** key, int64_t shape[4], int* ndim) {
  if (!m || index < 0 || index >= (int)m->specs.size() || !key || !shape || !ndim) return fail(KP2D_ERR_ARG, "bad argument");
  weight_info(m->specs, index, key, shape, ndim, /*pad_shape=*/true);
  return KP2D_OK;
}

int kp2d_lg_set_weight(kp2d_lg* m, const char* key, const float* host, const int64_t* shape, int ndim) {
  if (!m || !key || !host || (!shape && ndim > 0)) return fail(KP2D_ERR_ARG, "null argument");
  const int rc = set_weight(m->specs, m->index, m->host, key, host, shape, ndim);
  if (rc == KP2D_OK) m->finalized = false;
  return rc;
}

int kp2d_lg_finalize_weights(kp2d_lg* m) {
  if (!m) return fail(KP2D_ERR_ARG, "null model");
  std::vector<float> blob;
  int rc = pack(m, blob);
  if (rc == KP2D_OK) rc = upload_blob(m->cfg.device, &m->blob, blob);
  if (rc == KP2D_OK) m->finalized = true;
  return rc;
}

size_t kp2d_lg_workspace_bytes(const kp2d_lg* m, int B, int M, int N) {
  if (!m || B < 1 || M < 1 || N < 1) return 0;
  return layout(nullptr, m, B, M, N).total;
}

int kp2d_lg_forward(kp2d_lg* m, const float* kpts0, const float* kpts1, const float* desc0, const float* desc1,
                    const float* size0, const float* size1, int B, int M, int N, float filter_threshold,
                    float* log_assignment, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                    float* ref_desc0, float* ref_desc1, void* workspace, size_t workspace_bytes, void* stream) {
  return kp2d_lg_forward_counts(m, kpts0, kpts1, desc0, desc1, size0, size1, nullptr, nullptr, B, M, N, filter_threshold,
                                log_assignment, matches0, matches1, mscores0, mscores1, ref_desc0, ref_desc1, workspace,
                                workspace_bytes, stream);
}

int kp2d_lg_forward_counts(kp2d_lg* m, const float* kpts0, const float* kpts1, const float* desc0, const float* desc1,
                           const float* size0, const float* size1, const int32_t* n0, const int32_t* n1, int B, int M, int N,
                           float filter_threshold, float* log_assignment, int64_t* matches0, int64_t* matches1,
                           float* mscores0, float* mscores1, float* ref_desc0, float* ref_desc1, void* workspace,
                           size_t workspace_bytes, void* stream) {
  return run_forward(m, kpts0, kpts1, desc0, desc1, size0, size1, n0, n1, B, M, N, filter_threshold, log_assignment, matches0,
                     matches1, mscores0, mscores1, ref_desc0, ref_desc1, nullptr, workspace, workspace_bytes, stream);
}

size_t kp2d_lg_workspace_bytes_pruned(const kp2d_lg* m, int B, int M, int N) {
  // the same walk: compaction is in place and the index state lives in the keep / prune outputs
  return kp2d_lg_workspace_bytes(m, B, M, N);
}

int kp2d_lg_forward_pruned(kp2d_lg* m, const float* kpts0, const float* kpts1, const float* desc0, const float* desc1,
                           const float* size0, const float* size1, const int32_t* n0, const int32_t* n1, int B, int M, int N,
                           float filter_threshold, float width_confidence, float* log_assignment, int64_t* matches0,
                           int64_t* matches1, float* mscores0, float* mscores1, float* ref_desc0, float* ref_desc1,
                           int32_t* keep0, int32_t* keep1, int32_t* nkeep0, int32_t* nkeep1, int64_t* prune0, int64_t* prune1,
                           void* workspace, size_t workspace_bytes, void* stream) {
  if (!(width_confidence > 0.f && width_confidence <= 1.f))
    return fail(KP2D_ERR_ARG, "width_confidence=%g: point pruning takes a value in (0, 1]", (double)width_confidence);
  if (!keep0 || !keep1 || !nkeep0 || !nkeep1 || !prune0 || !prune1) return fail(KP2D_ERR_ARG, "null pruning outputs");
  // keep = score > 1 - width_confidence (lightglue.py:622), the difference taken in double as Python does
  const PruneIO pr{(float)(1.0 - (double)width_confidence), keep0, keep1, nkeep0, nkeep1, prune0, prune1};
  return run_forward(m, kpts0, kpts1, desc0, desc1, size0, size1, n0, n1, B, M, N, filter_threshold, log_assignment, matches0,
                     matches1, mscores0, mscores1, ref_desc0, ref_desc1, &pr, workspace, workspace_bytes, stream);
}

}  // extern "C"
