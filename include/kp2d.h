/* kp2d.h — C ABI of the MI355X-native kp2dtiny multi-task inference path.
 *
 * The reference (ETH-PBL/Nano-VS-SLAM) is pure Python: its boundary for this path is the
 * torch.nn.Module surface of KP2DTinyV2 / KP2DTinyV3 (src/kp2dtiny/models/kp2dtiny.py:284-1015).
 * This header is the layer UNDER that surface: the entry points a maintainer binds (ctypes stub in
 * INTEGRATION.md) so that Module.forward / Module.post_processing and the callers' keypoint
 * selectors run as hand-written gfx950 kernels.  Each function names the reference code it replaces.
 *
 * Conventions
 *   - plain C types only; every tensor is a raw pointer + sizes; float32 unless stated
 *   - "dev" pointers are HIP device pointers on the model's device, "host" pointers are CPU memory
 *   - API tensors are NCHW exactly as the reference returns them
 *   - every call returns 0 (KP2D_OK) or a negative kp2d_status; kp2d_last_error() gives the text
 *   - all device work is enqueued on the caller's stream; no call synchronises the device except
 *     kp2d_finalize_weights / kp2d_import_packed (one-time uploads) and kp2d_profile_* readers
 *   - the library never allocates caller-visible memory: outputs and the workspace are caller-owned
 *   - one handle per (device, stream); a handle is not thread-safe
 */
#ifndef KP2D_H_
#define KP2D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KP2D_ABI_VERSION 1

typedef enum kp2d_status {
  KP2D_OK = 0,
  KP2D_ERR_ARG = -1,          /* bad argument (null pointer, bad shape, H/W not divisible by 8 ...)      */
  KP2D_ERR_UNSUPPORTED = -2,  /* configuration outside the built path (see DESIGN.md "out of scope")     */
  KP2D_ERR_STATE = -3,        /* call order: weights not finalised, profiling off, ...                    */
  KP2D_ERR_WEIGHT = -4,       /* unknown key / wrong shape / missing tensor at finalise                    */
  KP2D_ERR_WORKSPACE = -5,    /* workspace too small or misaligned                                         */
  KP2D_ERR_HIP = -6           /* a HIP runtime call or kernel launch failed                                */
} kp2d_status;

typedef struct kp2d_model kp2d_model; /* opaque */

/* Constructor arguments of KP2DTinyV2.__init__ (kp2dtiny.py:301-319) / KP2DTinyV3.__init__ (:680-702)
 * that change the arithmetic.  get_config()/tiny_factory() (:221-281) live in the Python host layer. */
typedef struct kp2d_config {
  int32_t struct_size;      /* sizeof(kp2d_config), for ABI evolution                                   */
  int32_t version;          /* 2 = KP2DTinyV2, 3 = KP2DTinyV3                                            */
  int32_t channel_dims[6];  /* c1,c2,c3,c4,c5,d1                                                         */
  int32_t nfeatures;        /* descriptor channels                                                       */
  int32_t n_classes;        /* nClasses                                                                  */
  int32_t num_clusters;     /* NetVLAD K                                                                 */
  int32_t encoder_dim;      /* NetVLAD C                                                                 */
  int32_t downsample;       /* 2 for every S/N config (cell = 4)                                         */
  int32_t use_attention;    /* SegFormerAttentionModule x2 in the seg head                               */
  int32_t leaky_relu;       /* 1: LeakyReLU(0.01), 0: ReLU                                               */
  int32_t remove_softmax;   /* V3 only (kp2dtiny.py:698,942)                                             */
  int32_t device;           /* HIP device ordinal                                                        */
  int32_t global_descriptor;/* KP2D_GD_NETVLAD / KP2D_GD_GEM / KP2D_GD_CONVAP (vpr.py:53-76)                     */
  int32_t remove_netvlad;   /* to_export configs: "vlad" is the encoder map [B,enc,H/4,W/4] (vpr.py:84)          */
  int32_t depth;            /* depth=True: V2 second seg-like head, V3 third slice + featD (kp2dtiny.py:402-437)  */
  int32_t upscale_method;   /* KP2D_UP_PIXELSHUFFLE / KP2D_UP_CONVTRANSPOSE (to_mcu, kp2dtiny.py:271-273; base.py:80-117)  */
  int32_t in_channels;      /* 3 = RGB frames; 1 = KP2DTinyV3(use_color=False) (kp2dtiny.py:718-721); 0 means 3.  A caller built
                               against the struct without this field (struct_size 84) gets 3.                               */
} kp2d_config;
#define KP2D_UP_PIXELSHUFFLE 0
#define KP2D_UP_CONVTRANSPOSE 1
#define KP2D_GD_NETVLAD 0
#define KP2D_GD_GEM 1
#define KP2D_GD_CONVAP 2

/* kp2d_forward flags */
#define KP2D_FWD_EVAL 1u    /* model.training is False: V3 applies Softmax2d to seg (kp2dtiny.py:942-943) */
#define KP2D_FWD_ONLY_ENCODER 2u /* model.only_encoder(x) (kp2dtiny.py:515-518, vpr.py:78-89): backbone + convlad1-3 only;
                                    vlad = channel-wise L2-normalised encoder map [B,enc,Hc,Wc] (raw map when
                                    remove_netvlad); score/shift/feat/seg/depth are not written and may be NULL */
#define KP2D_FWD_NO_SEG_LOGITS 4u /* the caller will not read seg: it wants the dense class ids this forward writes
                                    (kp2d_set_seg_ids) and nothing else of the segmentation head.  Honoured only while
                                    kp2d_set_seg_ids holds a buffer, ignored otherwise.  seg must still be a valid buffer
                                    of the usual size; after the call its contents are UNSPECIFIED (big grids of the plain
                                    V2 S configuration in f16x3 arithmetic skip the logits store and write ids only; every
                                    other case — V3 / softmax, fp32 arithmetic, a tap set, small grids — runs as without
                                    the flag and writes both).  The ids, and every other output, are the same bits either
                                    way: the flag never changes a result, only whether the logits are stored */

const char* kp2d_last_error(void);
int32_t kp2d_abi_version(void);

/* ---- lifetime ------------------------------------------------------------------------------- */
/* replaces: KP2DTinyV2(**conf, nClasses=..) / KP2DTinyV3(..) construction (eval_multitask.py:150-159) */
int kp2d_create(const kp2d_config* cfg, kp2d_model** out);
void kp2d_destroy(kp2d_model* m);

/* ---- weights: the state_dict is the wire format ---------------------------- */
/* enumerate the tensors the model expects, in the reference's registration order */
int kp2d_num_weights(const kp2d_model* m);
int kp2d_weight_info(const kp2d_model* m, int index, const char** key, int64_t shape[4], int* ndim);
/* replaces: model.load_state_dict(sd) (eval_multitask.py:161-167, demo.py:12-15); host float32, C-contiguous.
 * BatchNorm num_batches_tracked entries are not part of the arithmetic and are ignored if passed. */
int kp2d_set_weight(kp2d_model* m, const char* key, const float* host, const int64_t* shape, int ndim);
/* fold BatchNorm into per-channel scale/shift, re-lay conv weights for the kernels, upload.  Blocking. */
int kp2d_finalize_weights(kp2d_model* m);
/* the packed device blob, for the one-off RCCL broadcast rank 0 -> all ranks */
size_t kp2d_packed_bytes(const kp2d_model* m);
int kp2d_export_packed(const kp2d_model* m, void* dev_dst, void* stream);
int kp2d_import_packed(kp2d_model* m, const void* dev_src, void* stream);

/* ---- forward --------------------------------------------------------------------------------- */
/* scratch the caller must provide for a (B,H,W) call; 256-byte aligned device memory */
size_t kp2d_workspace_bytes(const kp2d_model* m, int B, int H, int W);
/* replaces: KP2DTinyV2.forward (kp2dtiny.py:552-591) / KP2DTinyV3.forward (:906-957).
 *   x      [B,3,H,W]  RGB in [-1,1] ([B,1,H,W] for in_channels = 1); H, W divisible by 8
 *   score  [B,1,H/4,W/4]  sigmoid, un-bordered      shift [B,2,H/4,W/4]  tanh ("coord" key of forward)
 *   feat   [B,nfeatures,H/2,W/2] dense descriptors   seg   [B,n_classes,H/2,W/2] logits (V3 eval: probabilities)
 *   vlad   [B,kp2d_vlad_dim]: NetVLAD K*C; GeM / ConvAP encoder_dim*16; remove_netvlad: [B,encoder_dim,H/4,W/4] */
size_t kp2d_vlad_dim(const kp2d_model* m, int H, int W);
/*   depth  [B,1,H/2,W/2] sigmoid, only for depth=1 models (NULL otherwise) */
int kp2d_forward(kp2d_model* m, const float* x, int B, int H, int W, uint32_t flags, float* score, float* shift,
                 float* feat, float* seg, float* vlad, float* depth, void* workspace, size_t workspace_bytes,
                 void* stream);

/* kp2d_forward with the frame front-end as the first layer's prologue: frames is uint8 [B,Hs,Ws,3]
 * on the device; /255, the bilinear resize to (H, W) and .sub(0.5).mul(2) (src/evaluation/visual_odometry.py:77-87)
 * happen while conv1a stages its input tile, so the float [B,3,H,W] frame is never written.  Bit-identical to
 * kp2d_preprocess followed by kp2d_forward.  RGB models with a 16-channel first layer (every S / N / F config);
 * others return KP2D_ERR_UNSUPPORTED (use the two calls). */
int kp2d_forward_frames(kp2d_model* m, const uint8_t* frames, int B, int Hs, int Ws, int H, int W, uint32_t flags,
                        float* score, float* shift, float* feat, float* seg, float* vlad, float* depth, void* workspace,
                        size_t workspace_bytes, void* stream);

/* replaces: post_processing (kp2dtiny.py:593-625 / :959-993).  `desc` and `seg_ids` may be NULL when the
 * module is in training mode (the reference skips sampling: kp2dtiny.py:615).
 *   score_out [B,1,Hc,Wc] border-zeroed   coord [B,2,Hc,Wc] pixels (ch0 = x)
 *   desc [B,C,Hc,Wc] bilinearly sampled, unit norm   seg_ids [B,1,Hs,Ws] int64 argmax over seg's channels */
int kp2d_post(kp2d_model* m, const float* score, const float* shift, const float* feat, const float* seg, int B,
              int H, int W, int Hc, int Wc, int feat_c, int Hf, int Wf, int seg_c, int Hs, int Ws, float* score_out,
              float* coord, float* desc, int64_t* seg_ids, int sample_segmentation, void* stream);
/* sample_segmentation != 0 (model.sample_segmentation, kp2dtiny.py:634-639): seg_ids is [B,1,Hc,Wc], the class of the
 * nearest seg pixel at each cell's coordinate, instead of the dense [B,1,Hs,Ws] argmax. */

/* replaces the callers' selectors: threshold + top-k on the cell grid, batched and on device
 * (evaluation/visual_odometry.py:105-117 K1, evaluation/descriptor.py:12-36 K2,
 *  gluefactory/models/extractors/kp2dtiny.py:38-42 K3).  Order: score descending, flat index ascending.
 *   score [B,n]; idx [B,k] (-1 padded); val [B,k] or NULL; count [B]; thr = -INFINITY for plain top-k.
 *   Any k >= 1: the reference's "no cap" (top_k <= 0: every cell above thr, frontend.py:122) is k = n.  k <= 16384
 *   selects and sorts in LDS; larger k sorts in place in the idx row (slower, same result). */
int kp2d_select_topk(const float* score, int B, int n, int k, float thr, int32_t* idx, float* val, int32_t* count,
                     void* stream);
/* gather the selected cells: pts [B,k,2] (x,y), dsel [B,k,C]; rows of padded (-1) entries are zero */
int kp2d_gather_keypoints(const float* coord, const float* desc, const int32_t* idx, int B, int C, int n, int k,
                          float* pts, float* dsel, void* stream);

/* kp2d_select_topk + kp2d_gather_keypoints as one call (still two launches): what every caller of the selectors
 * does next (visual_odometry.py:113-117 indexes coord / feat with the selection; extractors/kp2dtiny.py:41-42 gathers
 * keypoints and descriptors).  Same outputs, bit for bit, as the two calls. */
int kp2d_select_keypoints(const float* score, const float* coord, const float* desc, int B, int C, int n, int k, float thr,
                          int32_t* idx, float* val, int32_t* count, float* pts, float* dsel, void* stream);

/* replaces the per-frame front-end of inference() (src/evaluation/visual_odometry.py:77-87): kornia.image_to_tensor
 * / 255, kornia bilinear resize (align_corners=False), .sub(0.5).mul(2).  frames: uint8 [B,Hs,Ws,3] on the device;
 * x: float32 [B,3,H,W]. */
int kp2d_preprocess(const uint8_t* frames, int B, int Hs, int Ws, float* x, int H, int W, void* stream);

/* replaces: BfFeatureMatcher.match = cv2.BFMatcher(NORM_L2).knnMatch(k=2) + goodMatchesOneToOne
 * (src/visual_odometry/feature_matcher.py:89-98, :179-209), batched over B frame pairs, on device.
 *   d0 [B,max0,C] query descriptors, n0 [B] valid rows; d1 [B,max1,C] train descriptors, n1 [B]; C in {32,64,128}
 *   nn_idx / nn_dist / nn_dist2 [B,max0]  nearest train row, its L2 distance, second-nearest distance
 *     (nn_idx alone = cv2.BFMatcher(NORM_L2, crossCheck=False).match, src/evaluation/descriptor.py:132-134)
 *     For ANY finite input: with >= 256 train rows the search ranks on split-fp16 matrix-core keys and decides on an
 *     exact pass, which needs every row's norm in [0.5, 2^15] (unit-norm descriptors are); a workgroup that meets a
 *     row outside that range scans its rows with the exact arithmetic instead (slower, same answer).  On equal fp32
 *     distances the lower train index wins, except that among THREE train rows within ~1e-6 of each other (not
 *     identical) the matrix-core form may return either of the two nearest as nn_idx; nn_dist / nn_dist2 are exact.
 *   match_q [B,max1]  the query kept for each train row after ratio test + one-to-one filtering (-1: none)
 *   match_d [B,max1]  its distance
 *   scratch: B*max1*8 bytes of device memory */
int kp2d_match_descriptors(const float* d0, const int32_t* n0, const float* d1, const int32_t* n1, int B, int max0,
                           int max1, int C, float ratio, int32_t* nn_idx, float* nn_dist, float* nn_dist2,
                           int32_t* match_q, float* match_d, void* scratch, void* stream);
/* The same with the matcher variants of the reference's callers:
 *   cls0 [B,max0] / cls1 [B,max1] (both or neither): per-row class ids — a query only sees train rows of its own class.
 *     Replaces VisualOdometry.match_semantic (src/visual_odometry/visual_odometry.py:347-380: one BF match per class
 *     id, 28 of them per frame) with ONE launch.  A query whose class has fewer than two train rows gets no match (the
 *     reference's knnMatch(k=2) has no second neighbour there and match_semantic skips the class).  NOTE: as shipped,
 *     the reference's match_semantic unpacks two values from a matcher that returns three, so every class lands in its
 *     bare `except` and it returns no matches at all; this implements what the loop is written to do.
 *   flags & KP2D_MATCH_MUTUAL: match_q[t] = q iff t is q's nearest train row AND q is t's nearest query; no ratio test
 *     (cv2.BFMatcher(NORM_L2, crossCheck=True).match, src/evaluation/descriptor.py:221-222).
 *   scratch: kp2d_match_scratch_bytes(B, max0, max1) bytes, 8-byte aligned (B*max1*16 is the least accepted; the rest
 *     lets a search with few pairs spread one query's train rows over several workgroups). */
#define KP2D_MATCH_MUTUAL 1u
size_t kp2d_match_scratch_bytes(int B, int max0, int max1);
int kp2d_match_descriptors_ex(const float* d0, const int32_t* n0, const float* d1, const int32_t* n1, int B, int max0,
                              int max1, int C, float ratio, const int32_t* cls0, const int32_t* cls1, uint32_t flags,
                              int32_t* nn_idx, float* nn_dist, float* nn_dist2, int32_t* match_q, float* match_d,
                              void* scratch, size_t scratch_bytes, void* stream);
/* The matched rows of every pair as compact lists in train order (what the VO loop takes to the host instead of every
 * keypoint and descriptor: visual_odometry.py:270-284 kps0 = prev_keypoints[idxs0], kps1 = kps_cur[idxs1]):
 *   pairs [B,max1,4] (x0, y0, x1, y1) from pts0 [B,max0,2] / pts1 [B,max1,2]; idx [B,max1,2] (query row, train row);
 *   dist [B,max1]; count [B].  pairs / idx / dist may each be NULL. */
int kp2d_match_pairs(const int32_t* match_q, const float* match_d, const float* pts0, const float* pts1, int B, int max0,
                     int max1, float* pairs, int32_t* idx, float* dist, int32_t* count, void* stream);

/* The VO loop's top_k_matches cap on the device, fused with the compaction above (replaces
 * src/visual_odometry/visual_odometry.py:272-283 — BF branch: np.argpartition(score, k)[:k], the k SMALLEST distances —
 * and :26-32 + :260-266 — LightGlue branch: get_matches_scores(...) then scores.topk(k), the k LARGEST matching scores):
 *   mode KP2D_TOPK_BF: match_q [B,max1] + val = match_d [B,max1] (kp2d_match_descriptors); pair = (pts0[match_q[t]], pts1[t])
 *   mode KP2D_TOPK_LG: matches0 [B,max0] int64 + val = matching_scores0 [B,max0] (kp2d_lg_forward);
 *                      pair = (pts0[q], pts1[matches0[q]])
 *   k <= 0: every match.  At most kcap = min(k, n) pairs per frame pair (n = max1 / max0), BEST FIRST, equal values by lower
 *   source row (the reference's order within its k survivors is unspecified; callers use the set).
 *   pairs [B,kcap,4] (x0, y0, x1, y1), idx [B,kcap,2] (row in set 0, row in set 1; -1 past count), out_val [B,kcap]
 *   (distance / score), count [B]; pairs / idx / out_val may each be NULL.
 *   scratch: kp2d_match_topk_scratch_bytes(B, max0, max1) bytes of device memory. */
#define KP2D_TOPK_BF 0
#define KP2D_TOPK_LG 1
size_t kp2d_match_topk_scratch_bytes(int B, int max0, int max1);
int kp2d_match_topk_pairs(int mode, const int32_t* match_q, const int64_t* matches0, const float* val, const float* pts0,
                          const float* pts1, int B, int max0, int max1, int k, float* pairs, int32_t* idx, float* out_val,
                          int32_t* count, void* scratch, size_t scratch_bytes, void* stream);

/* ---- measurement ------------------------------------------------------------------------------ */
/* when on, every kernel launch of kp2d_forward is bracketed by HIP events on the caller's stream */
int kp2d_set_profiling(kp2d_model* m, int on);
/* number of launches recorded by the last kp2d_forward; blocks until those events have completed */
int kp2d_profile_count(kp2d_model* m);
/* one record: layer name, kernel family, elapsed ms, algorithmic FLOPs and HBM bytes of that launch */
int kp2d_profile_get(kp2d_model* m, int index, const char** layer, const char** kernel, float* ms, double* flops,
                     double* bytes);
/* Arithmetic of the convolution kernels (both accumulate in fp32 and meet the 1e-3 / index-identity bar):
 *   KP2D_PREC_FP32   exact fp32 on v_mfma_f32_32x32x2_f32 (bit-for-bit an fp32 fma chain)
 *   KP2D_PREC_F16X3  split fp16: x*w = xh*wh + xh*wl + xl*wh on v_mfma_f32_16x16x32_f16 (3x3 convolutions; the 1x1
 *                    convolutions and the attention kernel use v_mfma_f32_32x32x16_f16), fp32 accumulate, fp32-grade error
 *                    (default; see DESIGN.md "Numerics").  Both weight packs are resident; switching is free.
 *                    Range: every layer's output stays inside the float64 error bound of tests/layer_ref.py (fp32
 *                    accumulation plus the split's 2^-22 relative / 2^-25 absolute representation error) for input
 *                    activations of any magnitude below 2^16, fp16 subnormals and zero included (checked per layer down
 *                    to 2^-24 of the layer's normal range by tests/test_gpu_layer_fp64.py).  From 65504 to 131008 the hi
 *                    half saturates and the lo half carries the rest in fp16 precision (no longer fp32-grade); values
 *                    beyond +-131008 saturate. */
#define KP2D_PREC_FP32 0
#define KP2D_PREC_F16X3 1
int kp2d_set_precision(kp2d_model* m, int mode);
int kp2d_get_precision(const kp2d_model* m);
/* Parity aid: the next kp2d_forward calls also copy ONE intermediate activation, as planar [B,C,H,W] fp32, to dst
 * (device memory, capacity in floats; a forward that needs more fails with KP2D_ERR_ARG).  layer = a CBR's state-dict
 * prefix ("backbone.conv1a", "backbone.conv3b", "vlad_head.convlad3", ...; a layer whose MaxPool2d is folded into its
 * store yields the pooled tensor), "<attention module>.att" / ".mff" (modules/segformer.py:217-220), or a stage inside an
 * attention module: its 1x1 layers by their state-dict prefix ("<module>.att.fn.to_q", ".att.fn.to_out", ".mff.fn.net.0",
 * ".mff.fn.net.1.net.1", ".mff.fn.net.3"), ".att.norm" / ".mff.norm" (the LayerNorm outputs), ".att.fn.to_kv" [2C, H/2, W/2],
 * ".att.fn" (the attention output in front of to_out) and ".mff.fn.net.1.net.0" (the depthwise output; three-launch MixFFN
 * only, the fused tail never writes it).  This is how
 * the tests compare the kernels with the reference's recorded intermediates (tests/golden *_taps fixtures) layer by
 * layer.  layer = NULL or dst = NULL switches it off. */
int kp2d_set_tap(kp2d_model* m, const char* layer, float* dst, size_t capacity_floats);
/* The next kp2d_forward / kp2d_forward_frames calls (not ONLY_ENCODER) also write the dense class map — the argmax over
 * the class planes of `seg`, what post_processing computes first (kp2dtiny.py:609 / :975) — to ids [B,1,H2,W2] int64
 * (device memory, capacity in elements), from the epilogue of the layer that writes `seg` while its tile is still in LDS.
 * kp2d_post with seg = NULL and seg_ids = that buffer then leaves the ids as they are instead of reading `seg` again.
 * ids = NULL switches it off.  Only valid while `seg` is unchanged between the two calls (the Python host checks the
 * tensor's identity and version counter). */
int kp2d_set_seg_ids(kp2d_model* m, int64_t* ids, size_t capacity);
/* frames per internal sub-batch (0 = automatic).  Intermediates of one sub-batch stay in the 256 MB Infinity Cache. */
int kp2d_set_chunk_frames(kp2d_model* m, int frames);
/* Tuning options of the engine (never needed for correct results; the A/B scripts and the parity tests use them to force a
 * kernel form).  Keys: "wsm_min_items", "ws_min_tiles", "wsm_grid", "wsm_transposed", "s16_min_items", "s16_all",
 * "multi_launch", "mff_fused", "stem_fusion", "side_overlap", "lanes"; kp2d_option_name lists them (KP2D_ERR_ARG past the last
 * index).  Meaning, default and range of each, and the KP2D_* environment variable that gives it its initial value when
 * kp2d_create runs, are the rows of ONE table: kOptions in nano-vs-slam_amd/csrc/options.h (README.md's table of knobs
 * describes the variables).  Setting a tile-form option back to 0 restores the built-in automatic policy
 * (nano-vs-slam_amd/csrc/conv_policy.h); "lanes" = 0 restores the handle's initial lane count.  An unknown key or a value
 * outside the row's range returns KP2D_ERR_ARG and changes nothing.  kp2d_get_option reads the value in effect ("lanes": the
 * lane count, never 0).  kp2d_profile_get reports the tile form each conv launch took behind its kernel family
 * ("conv3x3_f16x3<wsm>", "conv3x3_f16x3<2,1,16>", ...). */
int kp2d_set_option(kp2d_model* m, const char* key, long value);
int kp2d_get_option(const kp2d_model* m, const char* key, long* value);
int kp2d_option_name(int index, const char** key);

/* ---- Place recognition: flat squared-L2 top-k over global descriptors (nano-vs-slam_amd/csrc/vpr.hip) ----------
 * Replaces the faiss.IndexFlatL2 search of the reference's evaluate_global_descriptor
 * (src/evaluation/global_descriptor.py:55-60): for every query row the k nearest database rows by exact brute-force
 * squared L2 distance.  Stateless like the rest of the ABI: caller-owned device buffers, the caller's stream, no
 * synchronisation.  The Q x N distance matrix is never written.
 *   dim: dim % 16 == 0 and 16 <= dim <= 16384 (every shipped descriptor: 768 ... 8192), else KP2D_ERR_UNSUPPORTED.
 *   kp2d_vpr_pack: the database rows x [n,dim] fp32 -> packed [kp2d_vpr_packed_bytes(n, dim)] bytes.  Row r occupies
 *     bytes [r (4 dim + 16), (r + 1)(4 dim + 16)) and depends on row r alone, so a database grows by packing only the
 *     new rows at its end.  Holds |x|^2, the split-fp16 form of the row and its range-guard bit.
 *   kp2d_vpr_search: db [ndb,dim] fp32 and packed_db (kp2d_vpr_pack of the same rows; both precisions read its row
 *     norms), queries q [nq,dim] fp32 -> dist [nq,k] float, idx [nq,k] int64.
 *     dist holds SQUARED L2 distances (what IndexFlatL2.search returns), ascending, equal distances by lower row; equal
 *     rows therefore come out in ascending index order and a query equal to a row gets distance 0.  Slots past the rows
 *     available get idx = -1 and dist = FLT_MAX (faiss's flat-index padding).
 *     limit [nq] int64 or NULL: query i only sees rows [0, limit[i]) (<= 0: none) — e.g. loop-closure candidates of a
 *     whole trajectory in one call with limit[t] = t - W.
 *     k in [1, 1024] (k <= 32 is the fast path: the merge of database slices then takes 64 or more slices per pass).
 *     scratch: kp2d_vpr_scratch_bytes(nq, ndb, dim, k) bytes; q, db, packed_db and scratch 16-byte aligned.
 *     Bad arguments: KP2D_ERR_ARG.
 *   Accuracy.  Candidates are ranked by key = |d|^2 - 2 q.d; the k finalists are then re-scored directly as
 *     sum (q - d)^2 in fp32, so a returned distance is within 32 u d64 + 2 u d64 of float64 (u = 2^-24; d64 the float64
 *     distance of the same fp32 rows).  Default (flags = 0): the key's q.d in split fp16, q = 2^-s (qh + ql) with a
 *     power of two s per row putting max|q| 2^s in [2^14, 2^15), three fp16 products per pair on the matrix cores,
 *     fp32 accumulation: |key error| <= 2 (32 u + 3 * 2^-22) sum|q_i d_i| + 32 u |d|^2, plus the subnormal floor
 *     2^-38 (max|q| sum|d_i| + max|d| sum|q_i|) (tests/test_vpr_cpu.py).  A row can be missing from the answer only if
 *     its distance lies within twice that bound of the k-th distance.
 *     flags & KP2D_VPR_FP32: q.d from exact fp32 products (v_mfma_f32_32x32x2_f32), key error <= 2 * 32 u sum|q_i d_i|
 *     + 32 u |d|^2.
 *     Range guard: a database row with a non-finite element or with max|d| outside [2^-40, 2^40) makes its 128-row
 *     block of the database (rows [128 b, 128 b + 128)) take the fp32 products for every query; rows in range keep
 *     the split's bound for any magnitude in between (the scale is per row), unnormalised GeM descriptors included.
 *   Determinism: a query's result is bit-identical whatever nq is, whichever other queries share the call and however
 *     the database is sliced over workgroups; packing rows in several calls gives the bytes of one call. */
#define KP2D_VPR_FP32 1u
size_t kp2d_vpr_packed_bytes(int64_t n, int dim);
int kp2d_vpr_pack(const float* x, int64_t n, int dim, void* packed, void* stream);
size_t kp2d_vpr_scratch_bytes(int nq, int64_t ndb, int dim, int k);
int kp2d_vpr_search(const void* packed_db, const float* db, int64_t ndb, int dim, const float* q, int nq,
                    const int64_t* limit, int k, uint32_t flags, float* dist, int64_t* idx, void* scratch,
                    size_t scratch_bytes, void* stream);
/* kp2d_vpr_search_masked: kp2d_vpr_search restricted to a per-query subset of the database rows.
 *   Mask format (one format for every call that takes or writes a mask): uint32 words, [nq, W] with
 *     W = ceil(ndb / 32); row r of query i is bit r & 31 of word i W + (r >> 5).  Bits at or past ndb are zero on
 *     output and ignored on input.  mask: 4-byte aligned, required (non-NULL) when ndb > 0.
 *   Everything else is kp2d_vpr_search's: the same packed database, the same scratch (kp2d_vpr_scratch_bytes), the same
 *     key arithmetic in both precisions, the same range guard, the same (key, row) total order, merge, fp32 re-score and
 *     (FLT_MAX, -1) padding where a query's mask holds fewer than k rows (an empty mask: every slot is padding).  The
 *     accuracy text above holds with "the database" read as "the rows of the query's mask".
 *   A 128-row block of the database whose mask words are zero for all 64 queries of a workgroup is skipped before its
 *     products: a search over a few positives touches a few blocks.
 *   Determinism: as above.  A key depends on its query, its row and its block's mode only, and a skipped block holds no
 *     row of any of the workgroup's queries, so a query's result is bit-identical whatever nq is, whichever other queries
 *     share the call and whatever their masks are. */
int kp2d_vpr_search_masked(const void* packed_db, const float* db, int64_t ndb, int dim, const float* q, int nq,
                           const uint32_t* mask, int k, uint32_t flags, float* dist, int64_t* idx, void* scratch,
                           size_t scratch_bytes, void* stream);

/* ---- Triplet mining: geographic radius masks, lists, one mining round (nano-vs-slam_amd/csrc/mining.hip) ----------
 * Replaces the two sklearn.neighbors.NearestNeighbors jobs of the reference's dataset classes (src/data/pittsburgh.py,
 * the same code in src/data/tokyo247.py): ground truth from UTM positions by radius_neighbors (getPositives :189-200,
 * the non-trivial positives and potential negatives of QueryDatasetFromStruct.__init__ :258-289) and the hard-triplet
 * mining of QueryDatasetFromStruct.__getitem__ (:295-333).  Stateless like the calls above: caller-owned device buffers,
 * the caller's stream; masks in the format stated at kp2d_vpr_search_masked.  nq >= 0, 0 <= ndb < 2^31.
 *
 * kp2d_geo_radius_mask: db_xy [ndb,2], q_xy [nq,2] FLOAT64 (8-byte aligned), radius >= 0 (not NaN) ->
 *   mask [nq, W] uint32, count [nq] int32 (set bits per query).  Row r is inside for query i when
 *     dx * dx + dy * dy <= radius * radius,   dx = db_x[r] - q_x[i],  dy = db_y[r] - q_y[i],
 *   every operation a separately rounded float64 operation (NO fused multiply-add): the CLOSED ball, which is what
 *   sklearn's radius_neighbors returns.  float64 on purpose: UTM northings near 4.5e6 m are 0.5 m apart in fp32.
 *   flags & KP2D_GEO_INVERT: the complement among rows [0, ndb) (the reference's potential negatives).  Every word of
 *   mask is written by exactly one wave (ballot-packed), no atomics; no synchronisation.
 *
 * kp2d_mask_lists: mask [nq, W] and lims [nq + 1] int64 on the device, lims[0] = 0, lims[i + 1] - lims[i] = the number
 *   of rows of query i (the caller's cumulative sum of count) -> idx [idx_len] int64 with idx_len = lims[nq]: query i's
 *   rows in ASCENDING order at idx[lims[i] .. lims[i + 1]) (scipy's / faiss's range-search layout; the reference sorts
 *   its lists, :271-273).  status: one int32 on the device, the call's own.  Nothing is written outside a query's span
 *   or outside [0, idx_len).  When a query's popcount disagrees with its span the call returns KP2D_ERR_ARG; to say so
 *   it waits for the stream (the caller has read lims[nq] from the device to size idx anyway).
 *
 * kp2d_vpr_mine: one mining round for nq queries, enqueued on the stream with no host round trip.
 *   In: the packed database and its fp32 rows (as kp2d_vpr_search), q [nq,dim]; qid [nq] int32 or NULL: the number each
 *     query is drawn under (NULL: its position i in the call), so a subset of queries draws what the whole set draws;
 *     pos_mask (the non-trivial positives) and
 *     neg_mask (the potential negatives), [nq, W]; neg_cache [nq, n_neg] int32 padded with -1 (last round's neg_idx), or
 *     NULL; n_sample >= 0 draws; 1 <= n_neg, 1 <= n_neg_factor, n_neg * n_neg_factor within [1, 1024]; margin >= 0;
 *     seed, round >= 0; flags: KP2D_VPR_FP32.  dim as the index's (else KP2D_ERR_UNSUPPORTED); q, db, packed_db and
 *     scratch 16-byte aligned, the masks and int32 / float arrays 4-byte, pos_idx 8-byte; violations: KP2D_ERR_ARG.
 *   a. Candidates: cand(i) = { cache rows in [0, ndb) } U { the n_sample draws }.  With nPot(i) the number of set bits of
 *      neg_mask[i], draw j is u = mix(mix(mix(seed + 0x9E3779B97F4A7C15) ^ (round << 32 | qid[i])) ^ j) mod nPot(i) (mix:
 *      the splitmix64 finaliser kp2d_kmeans_step's split uses; 64-bit unsigned arithmetic, round and qid as uint32) and selects
 *      the row of rank u among the set bits, ascending.  Draws are with replacement and the set removes duplicates: the
 *      reference's np.unique(concatenate(negCache, np.random.choice(potential_negatives, nNegSample))).  This is the
 *      reference's ALGORITHM, not numpy's random stream.  A cache row outside neg_mask is still a candidate, as in the
 *      reference.  nPot(i) = 0: no draws (the reference raises).  Bits are set with integer atomic OR: order-free.
 *   b. Positive: kp2d_vpr_search_masked over pos_mask with k = 1 -> pos_idx [nq] int64 and the squared distance dPos2.
 *      A query without a positive gets pos_idx = -1, neg_cnt = 0, d_pos = NaN and neg_idx all -1.
 *   c. Negatives: kp2d_vpr_search_masked over cand with k = n_neg * n_neg_factor (ascending, padded).
 *   d. Select: in float64, negative j violates when sqrt((double)dNeg2_j) < sqrt((double)dPos2) + sqrt((double)margin):
 *      Euclidean distances and margin ** 0.5, as the reference compares them (:325).  The violators are a prefix of the
 *      ascending list; the first n_neg of them -> neg_idx [nq, n_neg] int32 padded with -1, their number -> neg_cnt [nq]
 *      int32 (0 is the reference's `return None`).  d_pos [nq] float = (float)sqrt((double)dPos2), Euclidean.
 *      cand_mask [nq, W] or NULL: the candidate set of step a, for callers and tests.
 *   scratch: kp2d_vpr_mine_scratch_bytes(nq, ndb, dim, n_neg, n_neg_factor) bytes (0: bad shape); a shorter one is
 *     KP2D_ERR_ARG.
 *   Accuracy: pos_idx and the negatives carry the masked search's contract; dPos2 and dNeg2 are its fp32 re-scores
 *     (within 34 u d64, u = 2^-24), so d_pos is within 18 u d of the float64 Euclidean distance d (17 u from the square
 *     root of 1 + 34 u, one u from rounding to float), and a negative can be classified differently from float64 only
 *     when its distance lies within such a band of the threshold.
 *   Determinism: no float atomics; the draws are a function of (seed, round, qid[i], j) and neg_mask[i] alone, the
 *     searches are deterministic (above) and the selection is per query: every output is bit-identical from run to run,
 *     and a query mined alone under its qid gets what it gets inside a batch. */
#define KP2D_GEO_INVERT 1u
int kp2d_geo_radius_mask(const double* db_xy, int64_t ndb, const double* q_xy, int nq, double radius, uint32_t flags,
                         uint32_t* mask, int32_t* count, void* stream);
int kp2d_mask_lists(const uint32_t* mask, int nq, int64_t ndb, const int64_t* lims, int64_t* idx, int64_t idx_len,
                    int32_t* status, void* stream);
size_t kp2d_vpr_mine_scratch_bytes(int nq, int64_t ndb, int dim, int n_neg, int n_neg_factor);
int kp2d_vpr_mine(const void* packed_db, const float* db, int64_t ndb, int dim, const float* q, int nq,
                  const int32_t* qid, const uint32_t* pos_mask, const uint32_t* neg_mask, const int32_t* neg_cache,
                  int n_sample, int n_neg, int n_neg_factor, float margin, uint64_t seed, int round, uint32_t flags,
                  int64_t* pos_idx, int32_t* neg_idx, int32_t* neg_cnt, float* d_pos, uint32_t* cand_mask, void* scratch,
                  size_t scratch_bytes, void* stream);

/* ---- k-means over descriptors (nano-vs-slam_amd/csrc/kmeans.hip) ------------------------------------------------
 * Replaces the faiss.Kmeans fit of the reference's NetVLAD initialisation (utils/netvlad_utils.py:83-88,
 * train_visloc.py:119-183).  Stateless like kp2d_vpr_*: caller-owned device buffers, the caller's stream, no
 * synchronisation and no host round trip inside a call.
 *   Algorithm: Lloyd iterations with faiss's conventions.  One kp2d_kmeans_step on x [n,dim] fp32 and
 *     centroids_in [k,dim] fp32:
 *     assign [n] int64, dist [n] float: every point's nearest centroid and its squared L2 distance, by kp2d_vpr_search
 *       with the centroids as the database and k = 1, in the caller's precision (flags & KP2D_VPR_FP32 as there), in
 *       query chunks of a fixed size.  Tie rule: equal distances go to the LOWER centroid index.  A point with a
 *       non-finite element gets assign = -1 and belongs to no cluster.
 *     counts [k] int64: points per cluster.  obj [1] float: the sum of dist (faiss's obj[i]: distances to the centroids
 *       the iteration started with).
 *     centroids_out [k,dim] (not centroids_in): a non-empty cluster's mean, sum * (1 / count) in fp32.  An empty cluster
 *       takes faiss's split_clusters rule, in ascending cluster order: a donor cj is drawn with probability proportional
 *       to max(count_j - 1, 0) over the running counts, c[ci] = c[cj], then for even j c[ci][j] *= 1 + 1/1024 and
 *       c[cj][j] *= 1 - 1/1024 (odd j: the factors swapped), and the donor's running count is halved between the two.
 *       This is faiss's algorithm, NOT faiss's random stream: the draw is a counter-based hash of (seed, iteration, ci),
 *       so the same arguments give the same split, with no state anywhere.
 *     flags: KP2D_VPR_FP32; KP2D_KMEANS_SPHERICAL (every centroid L2-normalised after the update, faiss spherical=True);
 *       KP2D_KMEANS_NO_SPLIT (empty clusters keep their input centroid).
 *   kp2d_kmeans_train: niter steps (iteration = 0 .. niter - 1) from centroids (in: initial, out: final), ping-ponging
 *     two centroid buffers inside scratch; obj [niter].  assign / dist / counts are the last iteration's, i.e. against
 *     the centroids BEFORE the final update, exactly what faiss's loop leaves.
 *   dim: the index's rule (dim % 16 == 0, 16 <= dim <= 16384), else KP2D_ERR_UNSUPPORTED.  1 <= k <= 65536, n >= k,
 *     niter >= 1, else KP2D_ERR_ARG; n < 2^31.  scratch: kp2d_kmeans_scratch_bytes(n, dim, k) bytes (0: bad shape); x,
 *     centroids and scratch 16-byte aligned.
 *   Determinism: no float atomics.  Each cluster's rows are listed in ascending point order by a stable counting sort
 *     and summed in a fixed order: lists are cut into chunks of 512 rows, a chunk is summed by one wave (8 accumulators
 *     per lane, a lane group count that depends on dim alone, fixed trees) and the chunk sums are added in chunk order.
 *     Every size involved is a constant or a function of (n, k, dim), and the search is deterministic (above), so all
 *     outputs are bit-identical across runs, devices of the same kind and however the work is sliced; kp2d_kmeans_train
 *     equals niter calls of kp2d_kmeans_step.
 *   Accuracy (u = 2^-24): assign and dist carry the search's contract with k = 1.  Given the assignment, a centroid
 *     component is within 32 u mean_i |x_i| + 2 u |c64| of the float64 mean of the same rows (mean over the cluster's
 *     rows of that component's magnitude); obj is within sum_i 34 u d64_i + 32 u obj64 of the float64 objective
 *     (tests/kmeans_ref.py, pinned from both sides in tests/test_kmeans_cpu.py). */
#define KP2D_KMEANS_SPHERICAL 2u
#define KP2D_KMEANS_NO_SPLIT 4u
size_t kp2d_kmeans_scratch_bytes(int64_t n, int dim, int k);
int kp2d_kmeans_step(const float* x, int64_t n, int dim, const float* centroids_in, int k, uint32_t flags, uint64_t seed,
                     int iteration, float* centroids_out, int64_t* assign, float* dist, int64_t* counts, float* obj,
                     void* scratch, size_t scratch_bytes, void* stream);
int kp2d_kmeans_train(const float* x, int64_t n, int dim, float* centroids /* in: initial, out: final */, int k, int niter,
                      uint32_t flags, uint64_t seed, float* obj /* [niter] */, int64_t* assign, float* dist,
                      int64_t* counts, void* scratch, size_t scratch_bytes, void* stream);

/* ---- Fine-tuning the NetVLAD layer: forward with saved state, triplet loss, backward, Adam (nano-vs-slam_amd/csrc/vlad_train.hip) ----
 * The gradient step of the reference's place-recognition training (train_visloc.py:249-282: NetVLAD forward,
 * TripletMarginLoss(margin ** 0.5, p=2, reduction="sum") / nNeg, backward, Adam) for the two parameters of the layer,
 * conv.weight W [K,C] and centroids cent [K,C].  Everything upstream of the layer is frozen and no gradient with respect
 * to x is formed.  Stateless like the calls above: caller-owned device buffers, the caller's stream, no synchronisation,
 * no host round trip; arguments are checked on the host before any launch.
 *   Shapes: x [N,C,S] fp32 PLANAR (a frame's C channel planes of S pixels: only_encoder's [N,C,Hc,Wc]); 1 <= N <= 65535,
 *     S >= 1 (else KP2D_ERR_ARG); K % 4 == 0, C % 4 == 0, 4 <= K <= 64, K * C <= 8192 (the forward's limits) and
 *     (2 K (C + 1) + 64 (C + 1) + 64 (K + 1)) * 4 <= 160 KB of LDS (else KP2D_ERR_UNSUPPORTED); K = 64, C = 128 takes 115 712 B.
 *   scratch: kp2d_vlad_train_scratch_bytes(N, S, C, K) bytes (0: bad shape), 16-byte aligned, shared by the three calls of a
 *     step; a shorter one is KP2D_ERR_ARG.  kp2d_triplet_loss needs 4 (B + n_neg) bytes and takes them
 *     at the head of the scratch it is given; in a step's shared scratch that head is free between the forward and the backward
 *     (the forward has read its tile partials there, the backward writes them all again before it reads one).
 *
 * kp2d_vlad_forward_train: per frame
 *       xh[s] = x[:,s] / max(||x[:,s]||, 1e-12);  a = softmax_k(xh W^T);  r[k] = sum_s a[s,k]
 *       U[k] = sum_s a[s,k] xh[s] - r[k] cent[k];  n[k] = max(||U[k]||, 1e-12);  V[k] = U[k] / n[k]
 *       g = max(||V||_F, 1e-12);  v = V / g
 *   -> vlad [N, K*C] (v flattened k-major: the model's own "vlad" output in fp32 arithmetic) and saved [N, K*C + 2K + 4]:
 *   per frame V [K*C], n [K], r [K], g, three zeros.  saved is what kp2d_vlad_backward reads; nothing of size [S,K] is kept.
 *
 * kp2d_triplet_loss: vlad [N, dim] with rows [q_0..q_{B-1}, p_0..p_{B-1}, the n_neg negatives in query order], N = 2B + n_neg,
 *   B >= 1, n_neg >= 0; neg_offset [B + 1] int32 on the device, the exclusive prefix of the queries' negative counts
 *   (neg_offset[0] = 0, neg_offset[B] = n_neg); margin >= 0 is the SQUARED margin, the hinge uses margin ** 0.5.
 *       d(u, w) = || u - w + 1e-6 ||_2          (torch's pairwise_distance: eps added to the difference)
 *       loss = (1 / n_neg) sum_i sum_j max(0, d(q_i, p_i) - d(q_i, n_ij) + margin ** 0.5)
 *   -> loss (one float), dvlad [N, dim] = d loss / d vlad, n_active (one int32: triplets with a positive hinge).
 *   Differences and the eps are fp32 operations; a distance's squares, their sum and its square root are float64 and the
 *   distance is then rounded to fp32; every hinge term and every gradient entry is fp32 arithmetic on those distances; the
 *   hinge terms are added in float64 and the loss is rounded to fp32 once.
 *   Each row's gradient is gathered from its own triplets in triplet order: dq_i and dp_i are sums over j, a negative's
 *   row has one term; the rows of a query without negatives, of an inactive negative and of a positive without an active
 *   triplet are exactly zero.  n_neg == 0: loss = 0, dvlad = 0, n_active = 0.  The kernels clamp every offset to [0, n_neg],
 *   so a wrong prefix reads and writes nothing outside vlad / dvlad; its result is then unspecified.
 *
 * kp2d_vlad_backward: x, W, cent as in the forward, saved from it, dvlad [N, K*C] -> d_weight [K,C], d_centroids [K,C]:
 *       dV = (dv - v <v,dv>) / g;  dU[k] = (dV[k] - V[k] <V[k],dV[k]>) / n[k];  dcent[k] = -r[k] dU[k]
 *       da[s,k] = <xh[s],dU[k]> - <cent[k],dU[k]>;  dz[s,k] = a[s,k] (da[s,k] - sum_j a[s,j] da[s,j]);  dW[k] = sum_s dz[s,k] xh[s]
 *   summed over a frame's pixels, then over the frames.  a is recomputed per 64-pixel tile; pixels past S are masked in
 *   both [S,K] products and in the softmax.  (Where a norm met its 1e-12 floor the formulas above are used as they stand.)
 *
 * kp2d_adam_step: torch.optim.Adam's update (no weight decay, no amsgrad) of n floats, step = 1, 2, ...:
 *       m = m + (1 - beta1) (grad - m);  v = beta2 v + (1 - beta2) grad^2
 *       denom = sqrt(v) / sqrt(1 - beta2^step) + eps;  param -= lr / (1 - beta1^step) * m / denom
 *   The two bias corrections are formed on the host in double.  lr >= 0, 0 <= beta < 1, eps >= 0 (else KP2D_ERR_ARG).
 *   A zero gradient on zero moments leaves param bit-unchanged.
 *
 *   Arithmetic: exact fp32 on the vector ALU (no split-fp16 anywhere in training), float64 where stated.
 *   Determinism: no float atomics.  Tile t of a frame covers pixels [64 t, 64 t + 64); a tile's sums run over its pixels
 *     in pixel order, a frame's tiles are added in tile order and the frames in frame order, one workgroup per tile
 *     whatever N is: a frame's sums depend on S alone, the order over frames on N alone.  All outputs are bit-identical from
 *     run to run, vlad / saved rows do not depend on the other frames of the call, and frames behind the others whose
 *     dvlad rows are zero change no bit of d_weight or d_centroids. */
size_t kp2d_vlad_train_scratch_bytes(int N, int S, int C, int K);
int kp2d_vlad_forward_train(const float* x, const float* weight, const float* centroids, int N, int S, int C, int K,
                            float* vlad, float* saved, void* scratch, size_t scratch_bytes, void* stream);
int kp2d_triplet_loss(const float* vlad, int B, const int32_t* neg_offset, int n_neg, int dim, double margin, float* loss,
                      float* dvlad, int32_t* n_active, void* scratch, size_t scratch_bytes, void* stream);
int kp2d_vlad_backward(const float* x, const float* weight, const float* centroids, const float* saved, const float* dvlad,
                       int N, int S, int C, int K, float* d_weight, float* d_centroids, void* scratch, size_t scratch_bytes,
                       void* stream);
int kp2d_adam_step(float* param, const float* grad, float* m, float* v, int64_t n, int64_t step, double lr, double beta1,
                   double beta2, double eps, void* stream);

/* ---- Fine-tuning the whole place-recognition head: Conv + BatchNorm + (Leaky)ReLU forward and backward, and NetVLAD's
 *      input gradient (nano-vs-slam_amd/csrc/vpr_head_train.hip, vlad_train.hip) ----
 * What the reference's train_visloc.py --freeze_backbone moves: vlad_head.convlad{1,2,3}.conv.weight, .bn.weight, .bn.bias and
 * the two NetVLAD parameters above, all updated by kp2d_adam_step.  The backbone and every other head are frozen.
 * These three calls run BatchNorm on its RUNNING statistics, which are not updated, without Dropout2d: vlad_head.eval() under
 * autograd.  The reference's own mode, the head under model.train(), is the next section's.  Loss, row order, the squared margin and
 * the Adam conventions are those of kp2d_triplet_loss and kp2d_adam_step.  Stateless like the calls above: caller-owned
 * device buffers, the caller's stream, no synchronisation, no host round trip; arguments are checked on the host before any
 * launch.
 *   Shapes: tensors are fp32 PLANAR [N, C, H, W]; w is [Cout, Cin, 3, 3].  1 <= N <= 65535, H, W >= 1 (else KP2D_ERR_ARG);
 *     Cin % 16 == 0, Cout % 16 == 0, 16 <= Cin, Cout <= 128, H * W <= 2^30 (else KP2D_ERR_UNSUPPORTED).
 *   scratch: kp2d_cbr_train_scratch_bytes(N, H, W, Cin, Cout) bytes (0: bad shape), 16-byte aligned; a shorter one is
 *     KP2D_ERR_ARG.  Each call writes what it reads there, so one buffer of the largest layer's size serves every layer.
 *   slope: 0.01 for LeakyReLU, 0 for ReLU; 0 <= slope < 1 (else KP2D_ERR_ARG).
 *
 * kp2d_cbr_forward_train: c = conv3x3(x, w) (stride 1, padding 1, no bias);  y = act(scale c + shift) per output channel,
 *       act(v) = v > 0 ? v : slope v;  scale = gamma / sqrt(var + eps), shift = beta - mean scale (formed by the caller)
 *   -> y [N, Cout, H, W] and c [N, Cout, H, W], the convolution's own result, which kp2d_cbr_backward reads.
 *
 * kp2d_cbr_backward: x, w, scale as in the forward, mean and invstd = 1 / sqrt(var + eps) [Cout], y and c from the forward,
 *   dy [N, Cout, H, W]:
 *       dpre = dy (y > 0 ? 1 : slope)        (torch's rule; y > 0 is the pre-activation's sign for both slopes)
 *       d_beta[co] = sum dpre;  d_gamma[co] = sum dpre (c - mean) invstd      (from c itself: right where gamma = 0)
 *       dc = dpre scale
 *       d_weight[co,ci,ky,kx] = sum_{n,y,x} dc[n,co,y,x] x[n,ci,y+ky-1,x+kx-1]
 *       dx[n,ci,y,x] = sum_{co,ky,kx} dc[n,co,y-ky+1,x-kx+1] w[co,ci,ky,kx]      (skipped when dx is NULL: the first layer
 *                                                                                  behind a frozen backbone)
 *   -> d_weight [Cout, Cin, 3, 3], d_gamma [Cout], d_beta [Cout], dx [N, Cin, H, W].  d_weight, d_gamma and d_beta have the
 *   same bits with and without dx.
 *
 * kp2d_vlad_backward_input: the gradient kp2d_vlad_backward does not form.  Arguments and scratch as kp2d_vlad_backward
 *   (kp2d_vlad_train_scratch_bytes); additionally C <= 128, and for K > C one more [64][K + 1] of LDS (else
 *   KP2D_ERR_UNSUPPORTED; for K <= C the tile takes kp2d_vlad_backward's LDS).  With dU, a and dz as kp2d_vlad_backward
 *   forms them per 64-pixel tile:
 *       dxh[s] = sum_k a[s,k] dU[k] + sum_k dz[s,k] W[k];  dx[:,s] = (dxh[s] - xh[s] <xh[s], dxh[s]>) / max(||x[:,s]||, 1e-12)
 *   -> dx [N, C, S].  It recomputes dU and the tile's softmax: it shares nothing in memory with kp2d_vlad_backward,
 *   whose results it leaves as they were.  A frame whose dvlad row is zero gets dx = 0 exactly.
 *
 *   Arithmetic: exact fp32 everywhere (no split-fp16).  The three convolution-shaped products are implicit GEMMs on
 *     v_mfma_f32_16x16x4_f32, bit for bit an fp32 fma chain; everything else runs on the vector ALU.
 *   Determinism: no float atomics.  An output tile is 8 x 16 pixels; the weight gradient is cut over the tiles (frame-major)
 *     into at most 128 slabs, a slab's sum runs over its tiles and pixels in order, the slabs are added in slab order, the
 *     BatchNorm sums per frame in a fixed order and then in frame order: the order depends on (N, H, W) alone, every output
 *     is bit-identical from run to run, and a frame whose dy is zero everywhere changes no bit of any gradient whatever its
 *     x, y and c hold. */
size_t kp2d_cbr_train_scratch_bytes(int N, int H, int W, int Cin, int Cout);
int kp2d_cbr_forward_train(const float* x, const float* w, const float* scale, const float* shift, double slope, int N, int H,
                           int W, int Cin, int Cout, float* y, float* c, void* scratch, size_t scratch_bytes, void* stream);
int kp2d_cbr_backward(const float* x, const float* w, const float* scale, const float* mean, const float* invstd, double slope,
                      const float* y, const float* c, const float* dy, int N, int H, int W, int Cin, int Cout, float* d_weight,
                      float* d_gamma, float* d_beta, float* dx /* may be NULL */, void* scratch, size_t scratch_bytes,
                      void* stream);
int kp2d_vlad_backward_input(const float* x, const float* weight, const float* centroids, const float* saved, const float* dvlad,
                             int N, int S, int C, int K, float* dx, void* scratch, size_t scratch_bytes, void* stream);

/* ---- The same layers as the reference's model.train() runs them: BatchNorm on the batch's own statistics, Dropout2d
 *      (nano-vs-slam_amd/csrc/vpr_head_train.hip) ----
 * train_visloc.py calls model.train() before its loop, so convlad1..3 normalise with the batch's mean and variance, move
 * their running statistics, and Dropout2d(0.2) zeroes whole channels of convlad1's output.  Shapes, slope, scratch
 * (kp2d_cbr_train_scratch_bytes; the per-frame partials take the area of the backward's BatchNorm sums), alignment, null and
 * stream rules are those of kp2d_cbr_forward_train / kp2d_cbr_backward above; everything is refused before the first launch.
 * M = N H W is the number of values per channel; M < 2 is KP2D_ERR_ARG in both calls (torch raises there too).
 *
 * kp2d_cbr_forward_batchnorm: gamma, beta [Cout]; drop [N, Cout] holding 0 or 1 / (1 - p), or NULL: no dropout;
 *   running_mean, running_var [Cout], updated in place, or NULL: not tracked; eps >= 0, 0 <= momentum <= 1 (else KP2D_ERR_ARG).
 *       c = conv3x3(x, w);  mean = sum c / M;  var = sum (c - mean)^2 / M  (BIASED);  invstd = 1 / sqrt(var + eps)
 *       y = act(gamma invstd (c - mean) + beta) drop[n, co]
 *       running_mean = (1 - m) running_mean + m mean;  running_var = (1 - m) running_var + m var M / (M - 1)  (UNBIASED)
 *   -> y, c [N, Cout, H, W], mean, invstd [Cout] (what kp2d_cbr_backward_batchnorm reads).  1 - m, m and m M / (M - 1) are
 *   formed on the host in double and rounded to fp32 once.  The variance is never formed as E[c^2] - mean^2: each (frame,
 *   channel) plane gives its mean and its sum of squared distances from that mean (two passes over the plane), and the planes,
 *   all of H W values, are merged by Chan's formula: mean = (sum_b mean_b) / N, M var = sum_b M2_b + H W sum_b (mean_b - mean)^2.
 *
 * kp2d_cbr_backward_batchnorm: mean, invstd, y, c from the forward, the same drop; per pixel, with xhat = (c - mean) invstd:
 *       g = dy drop[n, co] (y > 0 ? 1 : slope);  d_beta = sum g;  d_gamma = sum g xhat  (from c: right where gamma = 0)
 *       dc = gamma invstd (g - d_beta / M - xhat d_gamma / M)
 *   and d_weight, dx from dc as in kp2d_cbr_backward (dx may be NULL; d_weight, d_gamma, d_beta have the same bits either way).
 *   A dropped plane (drop = 0) has y = 0 and g = 0 exactly; its dc is not zero: the plane is part of the statistics.
 *
 * kp2d_dropout2d_mask: drop[n, c] = u >= p ? 1 / (1 - p) : 0, 0 <= p < 1 (else KP2D_ERR_ARG), N, C >= 1, N C < 2^31,
 *   0 <= step < 2^32, layer >= 0.  The draw is counter-based (mix = splitmix64's finaliser, nano-vs-slam_amd/csrc/mix64.h), all
 *   arithmetic modulo 2^64:
 *       h = mix(mix(mix(seed + 0x9E3779B97F4A7C15) ^ (step << 32 | layer)) ^ (n << 32 | c));  u = (h >> 11) 2^-53  (in double)
 *   It is this library's stream, not torch's: the stated deviation of kp2d_kmeans_* and kp2d_vpr_mine.  1 / (1 - p) is
 *   formed in double and rounded to fp32.
 *
 *   Determinism: no float atomics.  A plane's sums run over a thread's strided elements in order, then the wave's 64 lanes,
 *     then the four waves; the planes' partials are added in frame order; the order depends on (N, H, W) alone and every
 *     output is bit-identical from run to run.  Every frame enters mean and var, so here a frame whose dy is zero does change
 *     the other frames' gradients: that property belongs to the running-statistics calls alone. */
int kp2d_cbr_forward_batchnorm(const float* x, const float* w, const float* gamma, const float* beta, double eps, double slope,
                               const float* drop /* may be NULL */, double momentum, float* running_mean /* may be NULL */,
                               float* running_var /* may be NULL */, int N, int H, int W, int Cin, int Cout, float* y, float* c,
                               float* mean, float* invstd, void* scratch, size_t scratch_bytes, void* stream);
int kp2d_cbr_backward_batchnorm(const float* x, const float* w, const float* gamma, const float* mean, const float* invstd,
                                double slope, const float* drop /* may be NULL */, const float* y, const float* c, const float* dy,
                                int N, int H, int W, int Cin, int Cout, float* d_weight, float* d_gamma, float* d_beta,
                                float* dx /* may be NULL */, void* scratch, size_t scratch_bytes, void* stream);
int kp2d_dropout2d_mask(float* drop, int N, int C, double p, uint64_t seed, int64_t step, int layer, void* stream);

/* ---- The multitask place-recognition loss: batch-hard triplet on labelled embeddings (nano-vs-slam_amd/csrc/hard_triplet.hip) ----
 * The `vlad` term of the reference's train_multitask.py: HardTripletLoss (src/kp2dtiny/utils/losses.py:9-152) on
 * cat(vlad, vlad_aug) with the labels cat(arange(N), arange(N)) (KeypointNetwithIOLoss.py:572-583, :919-926), forward and
 * gradient in one call.  Stateless like the calls above: caller-owned device buffers, the caller's stream, no synchronisation,
 * no float atomics; every argument is checked on the host before the first launch and every output is fully written.
 *   emb [M, dim] fp32, labels [M] int32 on the device; 1 <= M (else KP2D_ERR_ARG), M <= 512 (else KP2D_ERR_UNSUPPORTED),
 *     dim >= 1; margin and weight finite, margin >= 0; flags: KP2D_HT_HARDEST | KP2D_HT_SQUARED, nothing else (else
 *     KP2D_ERR_ARG).  emb, labels, loss, demb 4-byte aligned, stats 8-byte, scratch 16-byte and at least
 *     kp2d_hard_triplet_scratch_bytes(M, dim) bytes (0: bad shape); a shorter one is KP2D_ERR_ARG.
 *   -> loss (one float), demb [M, dim] = d loss / d emb, stats [4] int64: anchors with a positive hinge (HARDEST) or hard
 *     triplets (batch-all), anchors without a positive, anchors without a negative, zero off-diagonal entries of the
 *     distance matrix (so a pair of equal rows counts twice).
 *
 * Distances: D2_ij = sum_k (x_ik - x_jk)^2, the differences of the widened operands (exact) squared and added in float64 in
 *   ascending k: the reference's max(0, n_i - 2 G_ij + n_j), G = X X^T, n_i = G_ii, without its cancellation.  Two bitwise-equal
 *   rows give exactly 0, and d_ij and d_ji are one number with one set of bits.  Without SQUARED d_ij = sqrt(D2_ij) where
 *   D2_ij > 0; a zero entry stays 0 and passes no gradient (the reference's mask trick; relu'(0) = 0 with SQUARED, d = D2);
 *   the diagonal is always a zero entry.  d_ij is rounded to fp32 once; [M, M] lives in scratch.
 * KP2D_HT_HARDEST (what the reference's multitask run uses), per anchor a:
 *       hp_a = max_j d_aj [j != a, label_j = label_a]           (no positive: 0, and no gradient)
 *       hn_a = min_j (d_aj + rowmax_a [label_j = label_a]),  rowmax_a = max_j d_aj
 *       loss = weight * mean_a relu(hp_a - hn_a + margin)
 *   Every max and min takes the lowest index among equal values.  When the minimum lands on a same-label column its gradient
 *   goes to d_aj and to the row maximum's column: an anchor without any negative has j = a and hn_a = rowmax_a, which is what
 *   autograd makes of the reference's lines.  (The reference's own hardest branch adds the literal 0.1 and never reads its
 *   margin; this call takes the margin it is given.)
 * Batch-all (no KP2D_HT_HARDEST): over triplets with a, p, n distinct and label_p = label_a != label_n,
 *       h = d_ap - d_an + margin;  loss = weight * sum relu(h) / (count(h > 1e-16) + 1e-16)
 *   the gradient flows where h > 0; no hard triplet: loss 0 and gradient 0.
 * Hinges are fp32 arithmetic on the fp32 distances, (d - d') + margin.  They are added in float64 and the loss is rounded once:
 *   HARDEST one hinge per anchor; batch-all per anchor and negative over the positives in ascending order, then the
 *   anchor's columns (thread t: columns t and t + 256; lanes by butterfly; the four waves); in both modes the anchors are
 *   then added the same way.  Counts are exact integers.
 * Gradient: both modes reduce to INTEGER coefficients c_ij with d loss / d d_ij = scale c_ij, scale = weight / M or
 *   weight / (count + 1e-16) formed in double and rounded to fp32 (HARDEST: at most three entries per row, +1 at the hardest
 *   positive, -1 at the minimum's column, -1 at the row maximum's when the minimum is a same-label column; batch-all: the
 *   active triplets a column takes part in as the positive minus those as the negative).  Then
 *       demb_i = sum_j s_ij (x_i - x_j),   s_ij = scale (c_ij + c_ji) / d_ij,   with SQUARED  2 scale (c_ij + c_ji)
 *   over j ascending in fp32 (fma), skipping the terms with c_ij + c_ji = 0, d_ij = 0 or s_ij = 0.  The receiving row scans
 *   (kp2d_keypoint_loss's rule): no atomics, and a row that no active triplet touches is exactly zero, as is everything
 *   when plus and minus cancel in c (M = 2 with equal labels: loss = weight * margin, demb = 0).
 * Edges, as the formulas give them: with SQUARED a D2 above FLT_MAX rounds to inf (so does a distance above it without);
 *   in batch-all mode hinges with 0 < h <= 1e-16 pass a gradient but are not counted, so when they are the only ones
 *   scale = weight / 1e-16 (the reference's own quotient).  labels are compared as int32.
 * Determinism: every sum has a fixed order that depends on (M, dim) alone; all outputs are bit-identical from run to run.
 *   The mean over anchors couples the rows: a pair run alone does not reproduce its bits of the larger batch.
 *
 * The view step of the trainers (nano_vs_slam_amd: NetVLADTrainer.step_views, VPRHeadTrainer.step_views) draws its two
 * Dropout2d masks with kp2d_dropout2d_mask's counter layout above: layer = 1 for the plain view, as every other step does,
 * and layer = 2 for the augmented view, at the same seed and step. */
#define KP2D_HT_HARDEST 1u
#define KP2D_HT_SQUARED 2u
size_t kp2d_hard_triplet_scratch_bytes(int M, int dim);
int kp2d_hard_triplet_loss(const float* emb /* [M, dim] */, const int32_t* labels /* [M], device */, int M, int dim, double margin,
                           uint32_t flags /* KP2D_HT_HARDEST | KP2D_HT_SQUARED */, double weight, float* loss /* 1 */,
                           float* demb /* [M, dim] */, int64_t* stats /* [4] */, void* scratch, size_t scratch_bytes, void* stream);

/* ---- Scores of the dense heads: segmentation counts and depth sums (nano-vs-slam_amd/csrc/dense_metrics.hip) -----
 * Replace what the reference's evaluate_segmentation takes from segmentation_models_pytorch (smp.metrics.get_stats,
 * src/evaluation/segmentation.py:42-48) and the reductions inside its compute_errors_torch
 * (src/evaluation/depth_estimation.py:58-83).  Stateless like kp2d_vpr_* and kp2d_kmeans_*: caller-owned device buffers,
 * the caller's stream, no synchronisation and no host round trip; every output is zeroed or fully written by the call
 * itself; arguments are checked before anything touches the device.  1 <= B <= 65535, n >= 1 elements per image.
 *
 * kp2d_seg_stats: per-image, per-class confusion counts.
 *   pred [B,n] int64 (what post_processing leaves in out["seg"]); target [B,n] of target_dtype KP2D_SEG_U8 / _I32 / _I64;
 *   1 <= num_classes = C <= 1024; ignore_index: any int64 except KP2D_SEG_NO_IGNORE, which means "ignore nothing".
 *   stats [B,C,4] int64 = (tp, fp, fn, tn); confusion [B,C,C] int64 or NULL (row = target class, column = predicted
 *   class; C <= 256, else KP2D_ERR_UNSUPPORTED); ignored [B] int64; stray [B] int64.
 *   Counting rule (this text is the definition):
 *     - a pixel whose target equals ignore_index is IGNORED: it adds to ignored[b] and to nothing else;
 *     - a pixel that is not ignored but whose target or prediction lies outside [0, C) is STRAY: it adds to stray[b]
 *       and to nothing else (valid data has none);
 *     - every other pixel is COUNTED, with target g and prediction p: g == p: tp[g] += 1 and confusion[g][g] += 1;
 *       otherwise fp[p] += 1, fn[g] += 1 and confusion[g][p] += 1;
 *     - tn[c] = counted - tp[c] - fp[c] - fn[c], so the four add up to n - ignored[b] - stray[b] for every class.
 *   With no stray pixel this is what smp.metrics.get_stats(mode="multiclass", ignore_index=...) returns.  That sentence
 *   was restated from smp's definition; smp was not available to run against.
 *   All counts are exact integers (integer LDS and global atomics only): outputs are bit-identical however the pixels are
 *   cut over workgroups.  The confusion matrix is gathered in an LDS tile for C <= kp2d_seg_conf_lds_max() and with one
 *   global add per pixel above it; the results do not differ.
 *
 * kp2d_depth_sums: the sums behind the nine depth metrics.
 *   gt, pred [B,n] fp32; valid [B,n] uint8 or NULL; min_depth / max_depth: limits on gt, a NaN turns that limit off.
 *   sums [B,KP2D_DEPTH_NSUMS] float64, per image: 0 count; 1-3 #(max(g/p, p/g) < 1.25, < 1.25^2, < 1.25^3);
 *   4 sum |g-p|/g; 5 sum (g-p)^2/g; 6 sum (g-p)^2; 7 sum (ln g - ln p)^2; 8 sum (ln p - ln g); 9 sum |log10 g - log10 p|;
 *   10 number of invalid pixels.  scratch: kp2d_depth_scratch_bytes(B, n) bytes (0: bad shape), 8-byte aligned; a shorter
 *   one is KP2D_ERR_ARG.
 *   Invalid-pixel rule: a pixel is invalid when gt or pred is non-finite or <= 0, or gt < min_depth, or gt > max_depth,
 *   or valid is 0.  Invalid pixels enter no sum and are tallied in slot 10; count + invalid = n.  (The reference has no
 *   such rule: one zero or NaN there poisons the mean of the whole batch.)
 *   Arithmetic: inputs are widened to float64; every term and every sum is float64 (the call is bound by reading two
 *   floats per pixel, the arithmetic is free).  The threshold counts use IEEE float64 division and equal numpy's float64
 *   counts exactly; slots 0-3 and 10 are exact integers.
 *   Determinism: no float atomics.  An image is cut into chunks of 4096 pixels; thread t of a chunk's 256 adds the terms
 *   of pixels t, t + 256, ... in that order, lanes are combined by a butterfly and the four waves in wave order; the
 *   chunk sums are then added the same way (thread t: chunks t, t + 256, ...).  The order depends on n alone, and no
 *   image's sum meets another's: a row of sums is bit-identical from run to run and whether the image is evaluated alone
 *   or inside a batch.
 *   Accuracy (u = 2^-53).  A term takes part in at most D(n) = 33 + ceil(ceil(n / 4096) / 256) rounded additions (15 in
 *   the thread, 6 + 3 in the workgroup, the same over the chunks), so a sum of exact terms is within D u sum|t_i|; on top
 *   comes each term's own rounding.  L is the error of the device library's double log / log10 in ulp: its
 *   documentation is not part of the installed ROCm tree, so L = 4 is an ASSUMPTION, not a documented figure.
 *   Against the float64 value of the same fp32 inputs, with d = ln g - ln p and d10 = log10 g - log10 p:
 *     slot 4: (D + 2) u sum |g-p|/g          slot 5: (D + 4) u sum (g-p)^2/g          slot 6: (D + 3) u sum (g-p)^2
 *     slot 7: (D + 3 + 4 L) u sum [ d^2 + |d| (|ln g| + |ln p|) ]
 *     slot 8: (D + 1 + 2 L) u sum [ |d| + |ln g| + |ln p| ]
 *     slot 9: (D + 1 + 2 L) u sum [ |d10| + |log10 g| + |log10 p| ]
 *   each times 1.001 for the second-order terms.  The log slots pay for the cancellation in ln g - ln p: each logarithm
 *   is wrong by up to 2 L u |ln x|, whatever is left of it in the difference.  tests/dense_ref.py restates these bounds;
 *   tests/test_dense_metrics_cpu.py checks that they hold for float64 sums in other orders, that one term evaluated in
 *   float32 breaks them, and that they stay below 2^-40 sum|t_i| on the test inputs. */
#define KP2D_SEG_U8 0
#define KP2D_SEG_I32 1
#define KP2D_SEG_I64 2
#define KP2D_SEG_NO_IGNORE INT64_MIN
#define KP2D_DEPTH_NSUMS 11
int kp2d_seg_conf_lds_max(void);
int kp2d_seg_stats(const int64_t* pred, const void* target, int target_dtype, int B, int64_t n, int num_classes,
                   int64_t ignore_index, int64_t* stats, int64_t* confusion, int64_t* ignored, int64_t* stray, void* stream);
size_t kp2d_depth_scratch_bytes(int B, int64_t n);
int kp2d_depth_sums(const float* gt, const float* pred, const uint8_t* valid, int B, int64_t n, double min_depth,
                    double max_depth, double* sums, void* scratch, size_t scratch_bytes, void* stream);

/* ---- Fine-tuning the segmentation head: the last layer, the dense loss, pooling and pixel shuffle
 *      (nano-vs-slam_amd/csrc/seg_train.hip; declared here because it uses KP2D_SEG_* above) ----
 * What the reference's train_multitask.py moves in its V2 SegmentationHead (modules/decoders/segmentation.py:8-157) under
 * _compute_segmentation_loss (KeypointNetwithIOLoss.py:880-884), next to the Conv + BatchNorm + (Leaky)ReLU layers of
 * kp2d_cbr_forward_train / kp2d_cbr_backward and kp2d_adam_step, which it reuses as they are.  The head runs as
 * seg_head.eval() under autograd: BatchNorm on its running statistics, no Dropout2d.  Stateless like those calls: caller-owned
 * device buffers, the caller's stream, no synchronisation, no host round trip; every argument is checked on the host before
 * the first launch.  Tensors are fp32 PLANAR [N, C, H, W]; 1 <= N <= 65535 and every extent >= 1 (else KP2D_ERR_ARG).
 *
 * kp2d_conv_bias_forward_train: y = conv3x3(x, w) (stride 1, padding 1) + bias, w [Cout, Cin, 3, 3], bias [Cout].
 *   Cin % 16 == 0, 16 <= Cin <= 128, 1 <= Cout <= 128 (ANY count, not only multiples of 16), H * W <= 2^30 (else
 *   KP2D_ERR_UNSUPPORTED).  scratch: kp2d_conv_bias_scratch_bytes(N, H, W, Cin, Cout) bytes (0: bad shape), 16-byte aligned.
 * kp2d_conv_bias_backward: dy [N, Cout, H, W] ->
 *       d_bias[co] = sum_{n,y,x} dy[n,co,y,x]      (a plane's sum, then the frames in frame order)
 *       d_weight[co,ci,ky,kx] = sum_{n,y,x} dy[n,co,y,x] x[n,ci,y+ky-1,x+kx-1]
 *       dx[n,ci,y,x] = sum_{co,ky,kx} dy[n,co,y-ky+1,x-kx+1] w[co,ci,ky,kx]      (skipped when dx is NULL)
 *   d_weight and d_bias have the same bits with and without dx.  The three products are the implicit GEMMs of
 *   kp2d_cbr_* on v_mfma_f32_16x16x4_f32 with Cout padded to the next multiple of 16 in the packed weights (which the call
 *   writes in full, zeros included, whatever scratch held): a padded channel reads no memory, contributes exact zeros and
 *   is never stored.  Tiles, slabs and their order are those of kp2d_cbr_backward.
 *
 * kp2d_seg_loss: logits [N, C, HW], labels [N, HW] of label_dtype KP2D_SEG_U8 / _I32 / _I64, 1 <= C <= 128, HW <= 2^30,
 *   ignore_index: any int64, KP2D_SEG_NO_IGNORE: ignore nothing; ce_weight, dice_weight finite and >= 0.
 *       loss = ce_weight CE + dice_weight Dice          (the reference: 0.5 and 1.5)
 *   A pixel whose label equals ignore_index is IGNORED; a pixel that is not ignored and whose label lies outside [0, C) is
 *   STRAY: it is treated as ignored and counted in *stray (valid data has none).  Every other pixel is VALID (*valid).
 *   With p = softmax(z) over the classes and t the one-hot label, both taken as 0 at pixels that are not valid:
 *       CE = (1 / valid) sum_valid -log p[label]                     torch.nn.CrossEntropyLoss(ignore_index), mean reduction
 *       I_c = sum p_c t_c;  S_c = sum (p_c + t_c)  (over the whole batch);  score_c = 2 I_c / max(S_c, 1e-7)
 *       Dice = (1 / C) sum_c [sum t_c > 0] (1 - score_c)
 *   A class absent from the labels adds 0 to the sum and stays in the divisor C.  Dice is smp.losses.DiceLoss(
 *   mode="multiclass", ignore_index=...) with smooth = 0, eps = 1e-7 as the reference constructs it, RESTATED from smp's
 *   definition: segmentation_models_pytorch was not available to run against, so it is not pinned; CE is pinned to torch.
 *   -> *loss, dlogits [N, C, HW] = d loss / d logits, *valid, *stray (int64).  Per valid pixel, with
 *   g_c = d Dice / d p_c = [present_c] (-2 t_c / (C S_c) + 2 I_c / (C S_c^2)):
 *       dlogits_j = (ce_weight / valid) (p_j - t_j) + dice_weight p_j (g_j - sum_c p_c g_c);  0 at every other pixel.
 *   Deviations: a batch without any valid pixel gives loss 0 and dlogits 0 (torch: NaN); a stray label is counted, not
 *   refused (torch raises).
 *   Two passes; the probabilities are never stored.  Pass 1 cuts the N HW pixels (frame-major) into chunks of 1024 and the
 *   chunks into at most 1024 runs, one workgroup each: per chunk a thread forms maximum, sum of exponentials and CE term
 *   of pixels t, t + 256, ...; wave w sums classes w, w + 4, ... (lane l: pixels l, l + 64, ... in order, then a butterfly);
 *   chunks are added in chunk order, the runs by one block in run order.  Pass 2 recomputes the softmax per pixel.
 *   scratch: kp2d_seg_loss_scratch_bytes(N, HW, C) bytes (0: bad shape), 16-byte aligned.
 *
 * kp2d_maxpool2_forward_train: y[n,c,i,j] = max of x[n,c,2i..2i+1,2j..2j+1], y [N, C, H / 2, W / 2] (floor), H, W >= 2.
 * kp2d_maxpool2_backward: dx [N, C, H, W] from dy [N, C, H / 2, W / 2] and the forward's x: the gradient goes to the
 *   window's maximum, found again from x (no index tensor).  Tie rule: the FIRST maximum in row-major order wins, torch's
 *   rule (a later element replaces the maximum only when it is greater or NaN).  A last odd row or column gets 0.
 * kp2d_shuffle_cat_forward: a [N, 4 C, h, w], b [N, Cb, 2 h, 2 w] (Cb >= 0) -> out [N, C + Cb, 2 h, 2 w]:
 *       out[n, c, 2 i + u, 2 j + v] = a[n, 4 c + 2 u + v, i, j]  (torch's pixel_shuffle(2));  out[n, C + cb] = b[n, cb]
 * kp2d_shuffle_cat_backward: da[n, 4 c + 2 u + v, i, j] = dout[n, c, 2 i + u, 2 j + v].  b's gradient is not formed: in the
 *   head b is a frozen backbone map.  Both tensors have at most 2^38 elements (else KP2D_ERR_UNSUPPORTED).
 *
 *   Arithmetic: exact fp32 everywhere (no split-fp16, expf / logf of the device library).  Determinism: no float atomics;
 *     every cut and every order of summation depends on the shapes alone, so all outputs are bit-identical from run to run. */
size_t kp2d_conv_bias_scratch_bytes(int N, int H, int W, int Cin, int Cout);
int kp2d_conv_bias_forward_train(const float* x, const float* w, const float* bias, int N, int H, int W, int Cin, int Cout, float* y,
                                 void* scratch, size_t scratch_bytes, void* stream);
int kp2d_conv_bias_backward(const float* x, const float* w, const float* dy, int N, int H, int W, int Cin, int Cout, float* d_weight,
                            float* d_bias, float* dx /* may be NULL */, void* scratch, size_t scratch_bytes, void* stream);
size_t kp2d_seg_loss_scratch_bytes(int N, int64_t HW, int C);
int kp2d_seg_loss(const float* logits, const void* labels, int label_dtype, int N, int64_t HW, int C, int64_t ignore_index,
                  double ce_weight, double dice_weight, float* loss, float* dlogits, int64_t* valid, int64_t* stray, void* scratch,
                  size_t scratch_bytes, void* stream);
int kp2d_maxpool2_forward_train(const float* x, int N, int C, int H, int W, float* y, void* stream);
int kp2d_maxpool2_backward(const float* x, const float* dy, int N, int C, int H, int W, float* dx, void* stream);
int kp2d_shuffle_cat_forward(const float* a, const float* b, int N, int C, int Cb, int h, int w, float* out, void* stream);
int kp2d_shuffle_cat_backward(const float* dout, int N, int C, int Cb, int h, int w, float* da, void* stream);

/* ---- Fine-tuning the depth head: the dense depth loss (nano-vs-slam_amd/csrc/depth_train.hip) ----
 * What the reference's train_multitask.py moves in depth_head under _compute_depth_loss (KeypointNetwithIOLoss.py:907-916):
 * SILogLoss (utils/losses.py:176-192) + huber_loss_factor torch.nn.HuberLoss().  In V2 non-attention models the head is the
 * SegmentationHead with one class: the layers are the calls above (kp2d_conv_bias_* at Cout = 1) and kp2d_cbr_*, the update is
 * kp2d_adam_step.  Stateless like those calls: caller-owned device buffers, the caller's stream, no synchronisation, no host
 * round trip; every argument is checked on the host before the first launch; every output is fully written.
 *
 * kp2d_depth_loss: logits [N, HW] BEFORE the sigmoid, gt [N, HW], both fp32; 1 <= N <= 65535 and HW >= 1 (else KP2D_ERR_ARG),
 *   HW <= 2^30 (else KP2D_ERR_UNSUPPORTED); silog_weight, huber_weight finite and >= 0 (the reference: 1 and 1).
 *   A pixel is VALID when gt is finite and > 0 and the logit is finite.  A pixel whose gt or logit is not finite is STRAY: it is
 *   treated as invalid and counted in *stray (kp2d_depth_sums' invalid-pixel rule; in torch one NaN poisons the batch).  Every
 *   other pixel (gt <= 0) is ignored: the reference's mask = gt > 0.  *valid = M, the number of valid pixels.
 *   Over the valid pixels, with p = sigmoid(z):
 *       g_i = log p_i - log gt_i = -softplus(-z_i) - log gt_i          finite for every finite z (torch's log(sigmoid(z)) is
 *                                                                      -inf in float32 beyond z = -104)
 *       SILog = KP2D_SILOG_SCALE sqrt(Dg),  Dg = var(g) + KP2D_SILOG_LAMBDA mean(g)^2     (torch.var: unbiased, M - 1)
 *       Huber = (1 / M) sum (0.5 d^2 if |d| < KP2D_HUBER_DELTA else KP2D_HUBER_DELTA (|d| - 0.5 KP2D_HUBER_DELTA)),  d = p - gt
 *       loss  = silog_weight SILog + huber_weight Huber
 *   -> *loss, parts[0] = SILog, parts[1] = Huber (unweighted), dlogits [N, HW] = d loss / d logits.  At a valid pixel
 *       dlogits_i = silog_weight (KP2D_SILOG_SCALE / 2 / sqrt(Dg)) (2 (g_i - mean) / (M - 1) + 2 KP2D_SILOG_LAMBDA mean / M) (1 - p_i)
 *                 + huber_weight (d_i if |d_i| < KP2D_HUBER_DELTA else sign(d_i) KP2D_HUBER_DELTA) / M  p_i (1 - p_i)
 *   and 0 at every other pixel.  The three constants are the reference's and are no arguments.
 *   Deviations: M = 0 gives loss 0 and dlogits 0 (torch: NaN); M = 1 gives SILog 0 with zero gradient, Huber stands alone
 *   (torch's unbiased variance of one value is NaN); Dg = 0 gives SILog 0 with zero gradient (torch: a NaN gradient).
 *   Two passes; nothing of size [N, HW] is stored besides dlogits.  Pass 1 cuts the N HW pixels (frame-major) into chunks of
 *   1024 and the chunks into at most 1024 runs, one workgroup each.  The variance is never formed as E[g^2] - mean^2: a chunk
 *   gives (count, mean, M2) - its sum of g, then its sum of (g - chunk mean)^2, each a float64 butterfly over a wave and the
 *   four waves in wave order - and these are merged by Chan's formula in chunk order, then the runs in run order.  Per-pixel
 *   arithmetic (g, p, d, the Huber term, dlogits) is fp32 with the device library's expf / logf / log1pf; the merge
 *   accumulators, the Huber sum and g_i - mean are float64.  Pass 2 recomputes g and p per pixel.  No float atomics; every
 *   cut depends on N and HW alone: all outputs are bit-identical from run to run.
 *   scratch: kp2d_depth_loss_scratch_bytes(N, HW) bytes (0: bad shape), 16-byte aligned; a shorter one is KP2D_ERR_ARG. */
#define KP2D_SILOG_SCALE 10.0
#define KP2D_SILOG_LAMBDA 0.15
#define KP2D_HUBER_DELTA 1.0
size_t kp2d_depth_loss_scratch_bytes(int N, int64_t HW);
int kp2d_depth_loss(const float* logits, const float* gt, int N, int64_t HW, double silog_weight, double huber_weight, float* loss,
                    float* parts, float* dlogits, int64_t* valid, int64_t* stray, void* scratch, size_t scratch_bytes, void* stream);

/* ---- Fine-tuning the keypoint heads: the self-supervised keypoint loss (nano-vs-slam_amd/csrc/keypoint_train.hip) ----
 * The first block of the reference's KeypointNetwithIOLoss.forward (KeypointNetwithIOLoss.py:423-541, build_descriptor_loss
 * :25-154) with with_io = False, over B pairs of a frame (the TARGET view, the reference's out) and its augmented view (the
 * SOURCE view, out_aug), with its gradient.  The heads' layers are kp2d_cbr_*, kp2d_conv_bias_* and kp2d_shuffle_cat_*, the
 * update is kp2d_adam_step.  Stateless like those calls: caller-owned device buffers, the caller's stream, no
 * synchronisation, no host round trip; every argument is checked on the host before the first launch; every output is
 * fully written.  Non-finite inputs are the caller's problem: nothing is read or written out of bounds because of them, but
 * the values are then undefined.
 *
 * kp2d_keypoint_loss: per view, fp32 planar, as the model's training forward returns them: score [B,1,Hc,Wc] after the
 *   sigmoid, shift [B,2,Hc,Wc] after the tanh (channel 0: x), feat [B,C,Hf,Wf], the raw descriptor map (Hf x Wf is free).
 *   homography [B,3,3] fp32, row-major, in NORMALISED coordinates ([-1, 1] over [0, W-1] x [0, H-1]): it maps source points
 *   to target points (the reference's _warp_homography_batch).  N = Hc Wc cells, numbered row-major; cell i is INTERIOR when
 *   it is not on the outermost ring; n = (Hc - 2)(Wc - 2) interior cells (0 if Hc < 3 or Wc < 3).
 *   Decode (post_processing in training mode), per view:  score' = score at interior cells, 0 on the ring;
 *       u = cell (col, row) + step + shift cross_ratio step,  step = (cell - 1) / 2;  coord = (clamp(u.x, 0, W-1), clamp(u.y, 0, H-1));
 *       the clamp's gradient is 1 where 0 <= u <= size - 1 (closed) and 0 elsewhere.  feat is not sampled here.
 *   Warp:  norm(c) = (c.x / ((W-1)/2) - 1, c.y / ((H-1)/2) - 1);  (X, Y, Z) = Hom (norm(coord_src_i), 1);
 *       wn_i = (X / Z, Y / Z);  w_i = ((wn_i.x + 1)(W-1)/2, (wn_i.y + 1)(H-1)/2).
 *   Location:  d_i = min_j |w_i - coord_tgt_j|_2 over ALL N target cells, a_i its argmin;  valid_i = d_i < KP2D_KEYPOINT_VALID_DIST
 *       and i interior;  M = the number of valid cells of the whole batch;  loc = (1 / M) sum_valid d_i.  d d_i / d w_i =
 *       (w_i - coord_tgt_a) / d_i = - d d_i / d coord_tgt_a, and 0 at d_i = 0 (torch's norm).
 *   USP:  S_i = score'_tgt[a_i] + score'_src[i];  usp = (1 / M) sum_valid S_i (d_i - loc);  d usp / d S_i = (d_i - loc) / M,
 *       d usp / d d_i = (S_i - mean_valid S) / M.
 *   Consistency:  v_i = bilinear sample of score'_tgt at wn_i (zeros outside, align_corners = True, the grid detached);
 *       con = 2 / (B n) sum_interior (v_i - score_src[i])^2  (0 when n = 0).
 *   Descriptor, per pair, only when n >= KP2D_KEYPOINT_MIN_ANCHORS, over the interior cells k (row-major) as anchors:
 *       ref_k = bilinear sample of feat_src at norm(coord_src_k), tar_k = of feat_tgt at wn_k (grids detached), each
 *       normalised as x / (|x + 1e-8|_2 + 1e-8);  dmat_kj = sqrt(2 - 2 clamp(ref_k . tar_j, -1, 1) + 1e-8);
 *       best_k = argmin_j dmat_kj;  hit_k = (w_best == w_k, both components exactly);
 *       neg_k = argmin_j dmat_kj over the columns with NOT (|w_j.x - w_k.x| <= relax_field and |w_j.y - w_k.y| <= relax_field);
 *       t_k = max(KP2D_KEYPOINT_MARGIN + |ref_k - tar_k + 1e-6|_2 - |ref_k - tar_neg + 1e-6|_2, 0)   (torch's triplet_margin_loss);
 *       metric = (1 / B) sum_pairs (1 / n) sum_k t_k.  Its gradient reaches ref_k, tar_k and tar_neg, then the two feat maps
 *       through the normalisation and the bilinear sampling; it reaches no coordinate.
 *   Total:  loss = keypoint_weight (loc_weight loc + descriptor_weight 2 metric + score_weight usp + score_weight con).
 *   -> *loss; parts[4] = (loc, metric, usp, con), unweighted; dscore_t, dshift_t, dfeat_t, dscore_s, dshift_s, dfeat_s shaped
 *   like the six maps: d loss / d map; counts[3] int64 = (M, n if the descriptor term ran else 0, sum over the pairs of hit_k);
 *   recall = counts[2] / (B n).
 *   Rules the reference leaves open:  every argmin takes the LOWEST index among equal values (a_i compares squared distances;
 *   torch's min and unstable sort define none);  an anchor with no admissible column takes best_k as neg_k (the reference's
 *   outcome under a stable sort);  M = 0 gives loc = usp = 0 with zero gradients (torch: NaN);  the IO-net term (with_io,
 *   InlierNet) is not built.
 *   Arithmetic: fp32 throughout, exact: the n x n x C products run on v_mfma_f32_16x16x4_f32 (an fmaf chain over the
 *   channels in ascending order) fused with both running argmins, nothing of size n x n is stored; the N x N nearest search
 *   is tiled through LDS.  The sums over cells behind M, loc, mean S, usp, con and the hinge sum are float64, per pair by a
 *   strided walk and a fixed butterfly, then over the pairs in pair order; so are the per-anchor reductions over the channels
 *   (the two norms of the normalisation and of the triplet term, sum g x of the normalisation's backward), O(n C) work.  No float atomics: where several anchors reach one
 *   target cell (through a_i, neg_k, or the bilinear backward onto score_tgt and the feat maps) the receiving side scans the
 *   anchors in ascending order.  Every order depends on the shapes alone: all outputs are bit-identical from run to run.
 *   Coupling between the pairs of a batch: M, loc and mean S (so dshift_*, and the usp part of dscore_*) are batch-wide; the
 *   descriptor term's dfeat_* carry the factor 1 / B and the consistency part of dscore_* the factor 1 / (B n), nothing else:
 *   a pair gives the same dfeat bits alone and in a batch of B = 2^k, up to that factor.
 *   Supported: 1 <= B <= 65535, N <= 65536, C a multiple of 16 in [16, 256], Hf Wf <= 2^24 (else KP2D_ERR_UNSUPPORTED);
 *   H, W >= 2, cell >= 1, cross_ratio, relax_field and the weights finite and >= 0 (else KP2D_ERR_ARG).
 *   scratch: kp2d_keypoint_loss_scratch_bytes(B, Hc, Wc, C, Hf, Wf) bytes (0: unsupported shape), 16-byte aligned. */
#define KP2D_KEYPOINT_VALID_DIST 4.0
#define KP2D_KEYPOINT_MARGIN 0.2
#define KP2D_KEYPOINT_MIN_ANCHORS 20
size_t kp2d_keypoint_loss_scratch_bytes(int B, int Hc, int Wc, int C, int Hf, int Wf);
int kp2d_keypoint_loss(const float* score_t, const float* shift_t, const float* feat_t, const float* score_s, const float* shift_s,
                       const float* feat_s, const float* homography, int B, int Hc, int Wc, int C, int Hf, int Wf, int H, int W,
                       int cell, double cross_ratio, double relax_field, double loc_weight, double descriptor_weight,
                       double score_weight, double keypoint_weight, float* loss, float* parts, float* dscore_t, float* dshift_t,
                       float* dfeat_t, float* dscore_s, float* dshift_s, float* dfeat_s, int64_t* counts, void* scratch,
                       size_t scratch_bytes, void* stream);

/* ---- View pairs: homography sampling, image warp, cross-view depth (nano-vs-slam_amd/csrc/augment.hip) ----
 * What the reference's dataset transforms do to make the second view of a training pair (src/data/dataset_utils.py:9-136 and
 * :198-266, nyuv2.py:183-257): sample_homography, then tgm.HomographyWarper(im_h, im_w, mode="nearest") on the image, the
 * labels and the depth, then a nearest Resize of the targets to 1 / d_f; and the one loss term that needs the warp, the
 * depth head's MSE(depth_aug, warp(depth, H)) (KeypointNetwithIOLoss.py:587-603).  Stateless like the calls above:
 * caller-owned device buffers, the caller's stream, no synchronisation, no host round trip, no float atomics; every argument
 * is checked on the host before the first launch; every output is fully written.
 *
 * THE COORDINATE MAP.  One definition, used by kp2d_warp, kp2d_warp_backward, kp2d_cross_view_mse and the numpy oracle
 * (tests/augment_ref.py).  Source map H x W (both >= 2), output Ho x Wo with stride s (Ho s == H, Wo s == W, else
 * KP2D_ERR_ARG; s = 1 is the plain warp).  For the output pixel (i, j) and the frame's homography h (row-major [3,3]):
 *       X = j s,  Y = i s                  (the pixel of the full-size grid that the reference's nearest Resize keeps)
 *       gx = 2 X / (W - 1) - 1,   gy = 2 Y / (H - 1) - 1
 *       u' = (h00 gx + h01 gy) + h02,   v' = (h10 gx + h11 gy) + h12,   w' = (h20 gx + h21 gy) + h22
 *       px = ((u' / w' + 1) / 2) (W - 1),   py = ((v' / w' + 1) / 2) (H - 1)
 *   all in IEEE double, the operations in the order written, none fused.  hom is [N,3,3] float32 (hom_f64 = 0; an entry is
 *   converted exactly) or float64 (hom_f64 = 1).  This is grid_sample(x, H grid, align_corners=True): warp(x, H)(q) = x(H q) in
 *   normalised coordinates, the convention of kp2d_keypoint_loss above (source = the augmented view).
 *   NEAREST: xi = rint(px), yi = rint(py), ties to even (torch's nearbyint); the pixel is INSIDE iff 0 <= xi <= W - 1 and
 *   0 <= yi <= H - 1; a non-finite coordinate is outside; an outside pixel gets fill.
 *   BILINEAR (float32 sources only): x0 = floor(px), fx = px - x0, the same in y; the four weights (1 - fx)(1 - fy), fx (1 - fy),
 *   (1 - fx) fy, fx fy are formed in double and rounded to fp32 once; a tap outside the map contributes zero whatever fill is
 *   (torch's padding_mode="zeros"); the blend is fp32, unfused: ((w00 a + w01 b) + w10 c) + w11 d.
 *
 * kp2d_warp: src [N, C, H, W] of dtype KP2D_WARP_F32 / _U8 / _I32 / _I64 -> dst [N, C, Ho, Wo] of the same type; mode
 *   KP2D_WARP_NEAREST or KP2D_WARP_BILINEAR (integer sources: nearest only, else KP2D_ERR_ARG); fill must be a value of the
 *   source's type (an integer in its range; |fill| <= 2^53 for int64; not NaN for float32), else KP2D_ERR_ARG.  A thread per
 *   output pixel, a workgroup per tile of KP2D_WARP_TILE_H rows x KP2D_WARP_TILE_W columns; the coordinates once, then the
 *   channels.  Limits: 1 <= N <= 65535, C >= 1, H, W >= 2 (else KP2D_ERR_ARG); H, W <= 32768 and C <= 4096 (else
 *   KP2D_ERR_UNSUPPORTED), so that C H W < 2^42 and every index is formed in 64 bits.
 *
 * kp2d_warp_backward: the gradient of the NEAREST warp.  dy [N, C, Ho, Wo] fp32 -> dx [N, C, H, W] fp32,
 *       dx[n,c,p] = sum of dy[n,c,q] over the output pixels q, in ascending row-major order, whose nearest source pixel is p
 *   (0 where there is none), the additions in fp32 in that order, no atomics: a thread per source pixel p maps the four
 *   corners of [p - 1/2 - g, p + 1/2 + g]^2 (g = 1/64) through the frame's inverse homography (adjugate over determinant in
 *   double), takes their bounding box in output pixels, widens it by one, clamps it, and tests every q of the box with the
 *   forward's own coordinate function.  When a corner's inverse w' is <= 0 or not finite, or the matrix is singular or not
 *   finite, that thread scans the WHOLE output: slow and correct.  Limits as kp2d_warp.  The bilinear warp has no backward.
 *
 * kp2d_homography_sample: the reference's sample_homography(shape = (H, W)), a thread per frame, all in double: the four
 *   corners (+-1, +-1) scaled by patch_ratio (y also by hw_ratio = H / W); perspective offsets z0, z1 (x) and z2, z3 (y) times
 *   amplitude / 2 (y: times hw_ratio), clipped to that; one scale about the centre; a translation inside the image; one of
 *   the n_angles + 1 candidate angles (0, then linspace(-max_angle, max_angle, n_angles)) whose rotated corners stay inside
 *   ([-1, 1) x [-hw_ratio, hw_ratio)); y / hw_ratio; the 8 x 8 system by elimination with partial pivoting (the reference's
 *   pinv of a square non-singular matrix).  -> hom64 [B,3,3] float64 and hom32 [B,3,3] float32, its rounding (either may be
 *   NULL, not both): it maps the first view's normalised coordinates to the second's, what kp2d_warp and the losses take.
 *   The randomness enters through draws [B, KP2D_HOMOGRAPHY_DRAWS] float64, per frame
 *       z0, z1, z2, z3    standard normals: the two x and the two y perspective offsets
 *       u_s in [0,1)      idx = floor(u_s n_scales); idx = 0: scale 1; else the scale is 1 + z_s scaling_amplitude / 2, clipped
 *       z_s               a standard normal (the reference draws n_scales of them and picks one; it never picks its last
 *                         draw, valid = np.arange(n_scales): the same range here)
 *       u_x, u_y in [0,1) the translation -t_min + u (t_max + t_min) per axis
 *       u_r in [0,1)      the rotation valid[floor(u_r len(valid))]; no valid candidate (the reference raises): no rotation
 *   so that the reference's own function, fed the same draws, pins the kernel.  perspective, scaling, rotation, translation
 *   are switches (reference: all 1); reference defaults n_scales 100, n_angles 100, scaling_amplitude 0.2,
 *   perspective_amplitude 0.2, patch_ratio 0.7, max_angle pi / 2.  B, H, W, n_scales >= 1, 1 <= n_angles <= 65536,
 *   0 <= scaling_amplitude < 2, perspective_amplitude >= 0, 0 < patch_ratio <= 1, max_angle >= 0 (else KP2D_ERR_ARG).
 * kp2d_homography_draws: fills draws from the library's own counter stream (not numpy's: a stated deviation, as in k-means,
 *   mining and dropout).  With mix = splitmix64's finaliser (csrc/mix64.h):
 *       h(slot, k) = mix(mix(mix(seed + 0x9E3779B97F4A7C15) ^ (step << 32 | frame)) ^ (slot << 32 | k)),  u(slot, k) = (h >> 11) 2^-53
 *   a uniform slot (4, 6, 7, 8) is u(slot, 0); a normal slot (0..3, 5) is Box-Muller in double:
 *   sqrt(-2 log(1 - u(slot, 0))) cos(2 pi u(slot, 1)).  B >= 1, 0 <= step < 2^32 (else KP2D_ERR_ARG).
 *
 * kp2d_cross_view_mse: depth, depth_aug [N, H, W] fp32 (after the sigmoid), hom as above.  The warp is nearest, at stride 1,
 *   and an outside pixel is 0, as the reference's warper makes it:
 *       diff = depth_aug - warp(depth, H)  (fp32);   loss = weight sum diff^2 / M;   M = N H W
 *       d_depth_aug = weight 2 diff / M;   d_depth = warp_backward(-d_depth_aug)
 *   *inside (int64) = the number of inside pixels.  inside_only = 1 restricts the sum, M (= *inside) and both gradients to the
 *   inside pixels; M = 0 then gives loss 0 and zero gradients.  inside_only = 0 is the reference: an outside pixel pulls
 *   depth_aug towards 0 (reproduced, not corrected).  The squares and their sum are float64: the N H W pixels (frame-major) in
 *   chunks of 1024, a chunk a butterfly over the wave and the four waves in wave order, the chunks of a run (at most 1024
 *   runs) in chunk order, the runs in run order; d_depth_aug = (float)((weight 2 / M) diff) with the product in double.
 *   Bit-identical from run to run.  weight finite and >= 0; shapes as kp2d_warp with C = 1.
 *   scratch: kp2d_cross_view_scratch_bytes(N, H W) bytes (0: bad shape), 16-byte aligned; a shorter one is KP2D_ERR_ARG. */
#define KP2D_WARP_F32 0
#define KP2D_WARP_U8 1
#define KP2D_WARP_I32 2
#define KP2D_WARP_I64 3
#define KP2D_WARP_NEAREST 0
#define KP2D_WARP_BILINEAR 1
#define KP2D_WARP_TILE_W 64
#define KP2D_WARP_TILE_H 4
#define KP2D_HOMOGRAPHY_DRAWS 9
int kp2d_homography_draws(double* draws, int B, uint64_t seed, int64_t step, void* stream);
int kp2d_homography_sample(const double* draws, int B, int H, int W, int perspective, int scaling, int rotation, int translation,
                           int n_scales, int n_angles, double scaling_amplitude, double perspective_amplitude, double patch_ratio,
                           double max_angle, double* hom64, float* hom32, void* stream);
int kp2d_warp(const void* src, int dtype, const void* hom, int hom_f64, int N, int C, int H, int W, int stride, int mode, double fill,
              void* dst, void* stream);
int kp2d_warp_backward(const float* dy, const void* hom, int hom_f64, int N, int C, int H, int W, int stride, float* dx, void* stream);
size_t kp2d_cross_view_scratch_bytes(int N, int64_t HW);
int kp2d_cross_view_mse(const float* depth, const float* depth_aug, const void* hom, int hom_f64, int N, int H, int W, double weight,
                        int inside_only, float* loss, float* d_depth, float* d_depth_aug, int64_t* inside, void* scratch,
                        size_t scratch_bytes, void* stream);

/* ---- Attention head training: the SegFormerAttentionModule's stages (nano-vs-slam_amd/csrc/attention_train.hip) ----
 * What the V2 SegmentationHeadATT needs beside the calls above: its two SegFormerAttentionModule (modules/segformer.py:209-220)
 * stage by stage, each with a forward that returns what its backward reads and a backward that returns every gradient.
 * Stateless: caller-owned device buffers, the caller's stream, no synchronisation; every argument is checked before the first
 * launch and every output is fully written.  Tensors are fp32 PLANAR [N, C, H, W]; 1 <= N <= 65535, H, W >= 1 (else
 * KP2D_ERR_ARG); every channel count is 48, 64, 96 or 128 and H W <= 2^24 (else KP2D_ERR_UNSUPPORTED).  Exact fp32; the matrix
 * products are chains of v_mfma_f32_16x16x4_f32 over the reduction index in ascending order (the attention logits: float64).  No float atomics: every sum's
 * order is fixed by the shapes, so a call is bit-identical from run to run.
 *   scratch: kp2d_att_train_scratch_bytes(N, H, W, Cin, Cout) bytes (0: bad shape), 16-byte aligned, of the call's own N, H, W
 *   and channel counts (patch2: Cin = C, Cout = 2 C; one-count calls: Cin = Cout = C); a shorter one is KP2D_ERR_ARG.
 *
 * kp2d_layernorm_forward_train: the reference's channel LayerNorm (segformer.py:63-73, not nn.LayerNorm): per pixel
 *   mean = sum_c x / C (channels in order), var = sum_c (x - mean)^2 / C, D = sqrt(var) + eps,
 *   y = (x - mean) / D * g + b; g, b [C].  Saved per pixel: mean [N, H W] and rinv = 1 / D [N, H W].
 * kp2d_layernorm_backward: with d = x - mean, s = sqrt(var) (formed again from x and the saved mean), D = s + eps, a = g dy:
 *   dx = (a - mean_c a) / D - d (sum_c a d) / (C s D^2);  a pixel with s = 0 takes the second term as 0 (torch: NaN).
 *   dg[c] = sum dy d rinv, db[c] = sum dy: per (frame, channel) plane thread t of 256 adds pixels t, t + 256, ... in order,
 *   a wave's 64 partials by butterfly, the four waves as (0 + 1) + (2 + 3); then the frames in frame order.
 * kp2d_pointwise_forward_train: y = conv1x1(x, w) (+ bias), w [Cout, Cin], bias [Cout] or NULL.  gelu != 0: pre receives that
 *   value and y = pre / 2 (1 + erf(pre / sqrt 2)) (nn.GELU()'s default, erff); otherwise pre may be NULL.
 * kp2d_gelu_backward: dpre = dy (Phi(pre) + pre phi(pre)), n elements.
 * kp2d_pointwise_backward: dy [N, Cout, H, W] -> dx [N, Cin, H, W] (NULL: not formed), d_weight [Cout, Cin], d_bias [Cout]
 *   (NULL: not formed; summed as db above).  d_weight: the N H W pixels in (frame, pixel) order are cut into at most 128 slabs
 *   of max(64, ceil(N H W / 128) rounded up to 4) pixels; a slab's partial is one chain over its pixels; the partials are added
 *   in slab order.
 * kp2d_patch2_forward_train: to_kv, a 2 x 2 stride-2 convolution without padding or bias, w [2 C, C, 2, 2], C in {48, 64},
 *   H, W >= 2: y [N, 2 C, H / 2, W / 2] (floor); the reduction index is 4 ci + 2 a + b.
 * kp2d_patch2_backward: dy [N, 2 C, H / 2, W / 2] -> dx [N, C, H, W] (NULL: not formed), d_weight as above over the patches.
 *   On an odd map the last row or column is in no patch: its dx is written as exact zeros.
 * kp2d_dwconv3_forward_train / _backward: depthwise 3 x 3, padding 1, bias: w [C, 1, 3, 3], taps in row-major order;
 *   dx [N, C, H, W] (NULL: not formed), d_weight [C, 1, 3, 3] and d_bias [C] summed per plane and then per frame as db above.
 * kp2d_attention_forward_train: 4 heads of dimension C / 4 (C in {48, 64}); q [N, C, H, W], head h owns channels h C/4 ...;
 *   kv [N, 2 C, H / 2, W / 2], keys in the first C channels, values in the second; S = H W queries, T = (H/2)(W/2) keys,
 *   H, W >= 2.  o [N, C, H, W] = softmax(scale q k^T) v with scale = (C / 4)^-0.5, by an online softmax over
 *   key tiles of 16 in ascending order; lse [2, N, 4, S]: lse[0] = max + log(sum exp) of each query's scaled logits rounded
 *   to fp32, lse[1] = (max - lse[0]) + log(sum exp), what that rounding dropped (near 60 an ulp is 4e-6, which every
 *   probability the backward forms again would carry).  Nothing of size S x T is stored; saturated rows stay finite (every
 *   exponent is <= 0).  The logits alone are formed in float64 (v_mfma_f64_16x16x4_f64 on the widened fp32 operands, scale
 *   = (C / 4)^-0.5 in double), with the running maximum and the log-sum-exp: an ulp of a float32 logit near 60 is 3.8e-6, which
 *   every probability the backward forms again would carry (measured with fp32 logits: dK, dV at 1.3 to 1.5 x 16 * 2^-24).
 *   Only the exponent's argument, logit - max or logit - lse, is rounded to fp32; the same function forms the logits in the
 *   forward and in both backward kernels.
 * kp2d_attention_backward: P = exp((scale q k^T - lse[0]) - lse[1]) again; delta = sum_c dO O; dV = P^T dO; dS = P (dO V^T - delta);
 *   dq = scale dS K [N, C, H, W]; dkv [N, 2 C, H / 2, W / 2] = (scale dS^T Q, dV).  dq belongs to tiles of 16 queries, which
 *   walk the keys in ascending order; dK and dV belong to tiles of 16 keys, which walk the queries in ascending order.  delta
 *   is the same chain over c as dO V^T, so with one key (P = 1, O = V) dS, dq and dK are exact zeros. */
size_t kp2d_att_train_scratch_bytes(int N, int H, int W, int Cin, int Cout);
int kp2d_layernorm_forward_train(const float* x, const float* g, const float* b, int N, int C, int H, int W, double eps, float* y,
                                 float* mean, float* rinv, void* stream);
int kp2d_layernorm_backward(const float* x, const float* g, const float* mean, const float* rinv, const float* dy, int N, int C, int H,
                            int W, double eps, float* dx, float* dg, float* db, void* scratch, size_t scratch_bytes, void* stream);
int kp2d_pointwise_forward_train(const float* x, const float* w, const float* bias, int N, int H, int W, int Cin, int Cout, int gelu,
                                 float* y, float* pre, void* stream);
int kp2d_gelu_backward(const float* pre, const float* dy, int64_t n, float* dpre, void* stream);
int kp2d_pointwise_backward(const float* x, const float* w, const float* dy, int N, int H, int W, int Cin, int Cout, float* dx,
                            float* d_weight, float* d_bias, void* scratch, size_t scratch_bytes, void* stream);
int kp2d_patch2_forward_train(const float* x, const float* w, int N, int C, int H, int W, float* y, void* stream);
int kp2d_patch2_backward(const float* x, const float* w, const float* dy, int N, int C, int H, int W, float* dx, float* d_weight,
                         void* scratch, size_t scratch_bytes, void* stream);
int kp2d_dwconv3_forward_train(const float* x, const float* w, const float* bias, int N, int C, int H, int W, float* y, void* stream);
int kp2d_dwconv3_backward(const float* x, const float* w, const float* dy, int N, int C, int H, int W, float* dx, float* d_weight,
                          float* d_bias, void* scratch, size_t scratch_bytes, void* stream);
int kp2d_attention_forward_train(const float* q, const float* kv, int N, int C, int H, int W, float* o, float* lse, void* stream);
int kp2d_attention_backward(const float* q, const float* kv, const float* o, const float* lse, const float* d_o, int N, int C, int H, int W,
                            float* dq, float* dkv, void* scratch, size_t scratch_bytes, void* stream);

/* ---- Keypoint scores: repeatability, localisation error, matching score (nano-vs-slam_amd/csrc/keypoint_metrics.hip) ----
 * The counts and sums behind the reference's compute_repeatability (src/evaluation/detector.py:67-113) and
 * compute_matching_score (src/evaluation/descriptor.py:112-170), for B image pairs per call.  Stateless like the calls
 * above: caller-owned device buffers, the caller's stream, no synchronisation, no host round trip; every output is fully
 * written by the call; arguments are checked before anything touches the device (bad shapes: KP2D_ERR_ARG).  The homography
 * fit (compute_homography: mutual matches + RANSAC) and the correctness / AUC values built on it are NOT part of this.
 *   pts0 [B,k0,3], pts1 [B,k1,3] fp32 rows (x, y, probability) of image 0 / image 1; cnt0, cnt1 [B] int32 rows that exist
 *   (clamped to [0, k]; the rest is padding and never read).  k0, k1 in [0, 65536] (a set may be empty: pts may then be
 *   NULL), 1 <= B <= 65535, keep_k >= 1.  hom [B,9] float64, row-major: maps image-0 pixels to image-1 pixels.
 *   scratch: kp2d_kp_scratch_bytes(B, k0, k1, C, keep_k) bytes (C = 0: repeatability only; 0 is returned for a bad shape),
 *   16-byte aligned; a shorter one is KP2D_ERR_ARG.
 *   Arithmetic: every coordinate is widened to float64 and all geometry is float64, as in the reference (its numpy code is
 *   float64 because warp_keypoints appends a float64 column of ones).  inv(hom) is the adjugate over the determinant in
 *   float64; the reference calls np.linalg.inv; the two agree to rounding.
 *   Selection ("the keep_k most probable rows"): row i ranks before row j when its probability is greater, or equal and
 *   i < j: among equal probabilities the LOWER row index is kept (numpy's argsort is unstable, so the reference defines no
 *   order there).  -0 and +0 are equal; probabilities are expected not to be NaN.
 *   The box quirk: the box test is 0 <= x < b0 and 0 <= y < b1, and the reference passes image_shape = (H, W) as (b0, b1):
 *   x is compared with the HEIGHT and y with the WIDTH (detector.py:41-46, keypoints.py:133).  Reproduced as is; pass the
 *   bounds the way the reference does to get its numbers.
 *
 * kp2d_kp_repeatability: set 1 keeps the rows whose warp by inv(hom) lies in the box; set 0 is warped by hom and keeps the
 *   rows whose warped point lies in the box; of each surviving set the keep_k most probable rows go on (N1 of set 0, N2 of
 *   set 1); every row's distance to the nearest row of the other set is taken in both directions, between the WARPED
 *   points of set 0 and the points of set 1.  counts [B,4] int64 = (N1, N2, count1, count2): count1 = rows of set 0 whose
 *   nearest distance is <= distance_thresh (NON-strict), count2 the same for set 1; le [B,2] float64 = (le1, le2), the sums
 *   of those distances.  An empty other set gives count = 0 and le = 0.  repeatability = (count1 + count2) / (N1 + N2) and
 *   loc_err = (le1 + le2) / (count1 + count2) are the caller's two divisions.
 *   Determinism: no float atomics.  The selected rows of a set are ordered by rank; thread t of a pair's workgroup adds the
 *   distances of ranks t, t + 256, ... in that order and the 256 partial sums are added by a fixed binary tree, so the order
 *   depends on the row ranks alone: outputs are bit-identical from run to run and whether a pair is scored alone or inside
 *   a batch, with any padding.
 *   Accuracy: le sums n <= 2 keep_k float64 terms, each <= distance_thresh, each carrying a few roundings of its own; any
 *   order of summation is within n^2 eps distance_thresh of the exact sum (eps = 2^-53): about 3e-10 at n = 1000 and
 *   distance_thresh = 3, which is why le1 and le2 are compared with the reference at 1e-9 absolute.  The counts are exact
 *   whenever no distance lies within rounding of distance_thresh and no warped coordinate within rounding of the box.
 *
 * kp2d_kp_matching_score: NO visibility filter (as in the reference): the keep_k most probable rows of each set, points and
 *   descriptors (desc0 [B,k0,C], desc1 [B,k1,C] fp32, 16-byte aligned, C in {32, 64, 128}), are gathered and matched in
 *   both directions by kp2d_match_descriptors_ex, whose nn_idx is cv2.BFMatcher(NORM_L2, crossCheck=False).match with the
 *   tie rule stated there.  Direction 1: the match in set 1 of every selected row of set 0 is warped by inv(hom); it is
 *   visible when 0 <= x <= b0 - 1 and 0 <= y <= b1 - 1, and correct when its distance to the row's own point is < 3
 *   (STRICT, a constant of the reference; compare the non-strict <= distance_thresh above).  Direction 2: the match in
 *   set 0 of every selected row of set 1, warped by hom.  counts [B,4] int64 = (vis1, hit1, vis2, hit2): visible matches and
 *   visible-and-correct matches per direction; the score is (hit1 / max(vis1, 1) + hit2 / max(vis2, 1)) / 2.  Either set
 *   empty: all four are 0 (the reference returns 0).  Integer counts: exact and order-free. */
size_t kp2d_kp_scratch_bytes(int B, int k0, int k1, int C, int keep_k);
int kp2d_kp_repeatability(const float* pts0, const int32_t* cnt0, const float* pts1, const int32_t* cnt1, const double* hom,
                          int B, int k0, int k1, double b0, double b1, int keep_k, double distance_thresh, int64_t* counts,
                          double* le, void* scratch, size_t scratch_bytes, void* stream);
int kp2d_kp_matching_score(const float* pts0, const int32_t* cnt0, const float* desc0, const float* pts1, const int32_t* cnt1,
                           const float* desc1, const double* hom, int B, int k0, int k1, int C, double b0, double b1,
                           int keep_k, int64_t* counts, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KP2D_H_ */
