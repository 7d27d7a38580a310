/* C ABI of the MI355X-native LightGlue matcher (BASELINE config 5).
 *
 * Replaces, for inference, the reference's `LightGlue(conf, weights_path)` torch module
 * (lightglue/lightglue.py:418-614; constructed at src/visual_odometry/visual_odometry.py:149-155 and by
 * gluefactory's `matchers.lightglue`, gluefactory/configs/kp2dtiny_S+lightglue_homography.yaml:25-31): eval mode,
 * flash = False, depth_confidence = -1 (the reference configs' value; early stopping is not built and the host layer
 * refuses it — the reference cannot run it either, lightglue.py:624/636).  Point pruning (width_confidence > 0,
 * lightglue.py:535-545, :564-579, :585-597, :618-625) is kp2d_lg_forward_pruned below.
 *
 * Conventions are those of include/kp2d.h: plain pointers and sizes, device pointers for tensors, caller-provided
 * workspace, work enqueued on the caller's stream, int status (0 = OK, kp2d_status codes, kp2d_last_error()).
 */
#ifndef KP2D_LIGHTGLUE_H
#define KP2D_LIGHTGLUE_H

#include "kp2d.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kp2d_lg kp2d_lg; /* opaque */

/* LightGlue.default_conf entries that change the arithmetic (lightglue.py:419-438; lightglue_configs.py:1-22) */
typedef struct kp2d_lg_config {
  int32_t struct_size;     /* sizeof(kp2d_lg_config)                                               */
  int32_t input_dim;       /* descriptor width of the extractor; != descriptor_dim adds input_proj */
  int32_t descriptor_dim;  /* D: 32 (configs S, A) or 64 (F); built for D % 32 == 0, D <= 64       */
  int32_t n_layers;        /* 4 in every reference config                                          */
  int32_t num_heads;       /* 4                                                                    */
  int32_t device;          /* HIP device ordinal                                                   */
} kp2d_lg_config;

/* replaces: LightGlue(conf) construction */
int kp2d_lg_create(const kp2d_lg_config* cfg, kp2d_lg** out);
void kp2d_lg_destroy(kp2d_lg* m);

/* weights: the reference module's state_dict is the wire format (keys in registration order, lightglue.py:444-470) */
int kp2d_lg_num_weights(const kp2d_lg* m);
int kp2d_lg_weight_info(const kp2d_lg* m, int index, const char** key, int64_t shape[4], int* ndim);
/* replaces: self.load_state_dict(torch.load(weights_path)) (lightglue.py:472-473); host float32, C-contiguous */
int kp2d_lg_set_weight(kp2d_lg* m, const char* key, const float* host, const int64_t* shape, int ndim);
int kp2d_lg_finalize_weights(kp2d_lg* m);

/* scratch for a batch of B image pairs with M / N keypoints each; 256-byte aligned device memory */
size_t kp2d_lg_workspace_bytes(const kp2d_lg* m, int B, int M, int N);

/* replaces: LightGlue.forward(data) (lightglue.py:484-614).
 *   kpts0 [B,M,2] / kpts1 [B,N,2]   keypoints in pixels (x, y)                   data["keypoints0/1"]
 *   desc0 [B,M,input_dim] / desc1 [B,N,input_dim]                                 data["descriptors0/1"]
 *   size0 / size1 [B,2] (w, h) or NULL: 1 + max - min of the keypoints            data["view0/1"]["image_size"]
 *   filter_threshold                                                              conf.filter_threshold
 * outputs (any of matches / scores / ref_desc may be NULL):
 *   log_assignment [B,M+1,N+1]   pred["log_assignment"]
 *   matches0 [B,M] / matches1 [B,N] int64 (-1: unmatched), mscores0 [B,M] / mscores1 [B,N]
 *   ref_desc0 [B,M,D] / ref_desc1 [B,N,D]  the last layer's descriptors (pred["ref_descriptors0/1"][:, 0])
 * Supported range.  The token-wise products and the attention run on split-fp16 operands (x = hi + lo, both fp16, fp32
 * accumulation: 2^-22 relative, "fp32-grade"); the split does not saturate.  So every value that enters a product — the
 * descriptors, every linear layer's output, the residual stream, q / k / v and the softmax weights — must stay below
 * fp16's largest finite value, 65504, in magnitude: beyond it the hi half is inf and the outputs are inf / NaN (no
 * error is reported).  Inside the range the results follow the float64 evaluation of the same network to a few fp32
 * roundoffs at any descriptor scale: tests/test_gpu_lightglue_forms.py checks descriptors of norm 2^-16 .. 2^12 with
 * unit-scale weights, where the largest intermediate value is 1.1e4 (LayerNorm bounds what the layers add, so the
 * residual stream keeps the scale of the descriptors).  Operand components below fp16's subnormal step (2^-24) keep an
 * ABSOLUTE precision of 2^-25, not a relative one.  Inputs must be finite. */
int kp2d_lg_forward(kp2d_lg* m, const float* kpts0, const float* kpts1, const float* desc0, const float* desc1,
                    const float* size0, const float* size1, int B, int M, int N, float filter_threshold,
                    float* log_assignment, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                    float* ref_desc0, float* ref_desc1, void* workspace, size_t workspace_bytes, void* stream);

/* The same on PADDED keypoint sets: n0 / n1 [B] int32 device arrays say how many rows of kpts0 / desc0 (kpts1 / desc1) exist,
 * the remaining rows of the M / N are padding.  This is what lets the matcher sit inside a replayed HIP graph behind a
 * threshold + top-k selection whose count changes from frame to frame (the reference hands LightGlue exactly the selected
 * rows, src/visual_odometry/visual_odometry.py:198-258: a different tensor shape every frame).  Padding rows are no keys in
 * any attention, carry no assignment mass, and come out as matches = -1 / scores = 0; the valid rows' results are those of
 * kp2d_lg_forward on the n0 / n1 rows alone (up to fp32 summation order).  log_assignment entries of padding rows / columns
 * are -inf (inner block) or unspecified (border).  size0 / size1 are required (the default would look at every row). */
int kp2d_lg_forward_counts(kp2d_lg* m, const float* kpts0, const float* kpts1, const float* desc0, const float* desc1,
                           const float* size0, const float* size1, const int32_t* n0, const int32_t* n1, int B, int M, int N,
                           float filter_threshold, float* log_assignment, int64_t* matches0, int64_t* matches1,
                           float* mscores0, float* mscores1, float* ref_desc0, float* ref_desc1, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Point pruning (width_confidence > 0 in eval mode).  After every layer but the last, and for each set, a point stays iff
 * sigmoid(log_assignment[i].matchability(desc)) > 1 - width_confidence (get_pruning_mask :618-625 without token confidences:
 * early stopping is off); the survivors keep their ascending order, and the later layers, the assignment and filter_matches
 * see only them.  The reference asserts B == 1; here every pair of the batch is pruned on its own and its result is that of
 * its B == 1 call.  The sets stay PADDED (static shapes): pruning compacts the surviving rows to the front of each set and
 * lowers the per-pair counts on the device, exactly the padded-set convention of kp2d_lg_forward_counts.
 *   n0 / n1 may be NULL: every pair starts with M / N points (then size0 / size1 may be NULL too).
 *   matches0/1, mscores0/1 are in the ORIGINAL index space; pruned and padding rows get -1 / 0.
 *   log_assignment [B,M+1,N+1] and ref_desc0/1 are in SURVIVOR order: inner entries (j < nkeep0[b], l < nkeep1[b]) are
 *     valid, the other inner entries -inf, the dustbin column N / row M holds the survivors' entries, the rest is unspecified
 *     (as in kp2d_lg_forward_counts).
 *   keep0 [B,M] / keep1 [B,N] int32: original index of survivor j, ascending; -1 past the count.
 *   nkeep0 / nkeep1 [B] int32: survivors of each pair.
 *   prune0 [B,M] / prune1 [B,N] int64, original index space: a point dropped after layer i holds i + 1, a survivor
 *     n_layers (lightglue.py:543-544, :572), a padding row 0.
 * A pair one of whose sets becomes (or starts) empty has matches -1 and scores 0; its other outputs are unspecified (they
 * may be NaN) and nothing of it reaches another pair.  (The reference fails there: max over an empty dimension.)
 * width_confidence outside (0, 1] -> KP2D_ERR_ARG; a null output other than ref_desc0/1 -> KP2D_ERR_ARG; a workspace below
 * kp2d_lg_workspace_bytes_pruned -> KP2D_ERR_WORKSPACE.  No host synchronisation, no allocation: the call can be captured
 * into a HIP graph. */
size_t kp2d_lg_workspace_bytes_pruned(const kp2d_lg* m, int B, int M, int N);
int kp2d_lg_forward_pruned(kp2d_lg* m, const float* kpts0, const float* kpts1, const float* desc0, const float* desc1,
                           const float* size0, const float* size1, const int32_t* n0, const int32_t* n1, int B, int M, int N,
                           float filter_threshold, float width_confidence, float* log_assignment, int64_t* matches0,
                           int64_t* matches1, float* mscores0, float* mscores1, float* ref_desc0, float* ref_desc1,
                           int32_t* keep0, int32_t* keep1, int32_t* nkeep0, int32_t* nkeep1, int64_t* prune0, int64_t* prune1,
                           void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KP2D_LIGHTGLUE_H */
