// The model's part of the C ABI declared in include/kp2d.h (create / weights / forward / post / select / options / profiling;
// the stateless features hold their entry points next to their kernels): every entry point checks its arguments and hands over
// to the model description (model_desc.cpp), the launch plan (plan.cpp) or a kernel launcher.  All arithmetic happens in the HIP
// kernels of this directory; there is no CPU compute path here (a missing device or library is an error, never a fallback).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.h"
#include "device_guard.h"
#include "kp2d_kernels.h"
#include "plan.h"
#include "weight_upload.h"

using namespace kp2d;
using namespace kp2d::plan;

namespace {
thread_local std::string g_err;
}

// ================================================================================================
extern "C" {

const char* kp2d_last_error(void) { return g_err.c_str(); }
extern "C++" {
namespace kp2d { void set_last_error(const char* msg) { g_err = msg ? msg : ""; } }   // for the other API files
}
int32_t kp2d_abi_version(void) { return KP2D_ABI_VERSION; }

int kp2d_create(const kp2d_config* cfg, kp2d_model** out) {
  if (!cfg || !out) return fail(KP2D_ERR_ARG, "null argument");
  // ABI evolution: the struct grew by in_channels; the shorter form (everything up to upscale_method) means RGB
  constexpr int32_t kOldSize = (int32_t)offsetof(kp2d_config, in_channels);
  if (cfg->struct_size != (int32_t)sizeof(kp2d_config) && cfg->struct_size != kOldSize)
    return fail(KP2D_ERR_ARG, "kp2d_config.struct_size mismatch");
  const int cin0 = (cfg->struct_size == kOldSize || cfg->in_channels == 0) ? 3 : cfg->in_channels;
  if (cin0 != 3 && cin0 != 1) return fail(KP2D_ERR_UNSUPPORTED, "in_channels=%d (3 and 1 are built)", cin0);
  if (cin0 == 1 && cfg->version != 3) return fail(KP2D_ERR_ARG, "in_channels=1 is KP2DTinyV3(use_color=False); V2 reads RGB");
  if (cfg->global_descriptor < KP2D_GD_NETVLAD || cfg->global_descriptor > KP2D_GD_CONVAP) return fail(KP2D_ERR_ARG, "bad global_descriptor");
  if (cfg->version != 2 && cfg->version != 3) return fail(KP2D_ERR_ARG, "version must be 2 or 3");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(KP2D_ERR_HIP, "no HIP device visible: this library has no CPU path");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(KP2D_ERR_ARG, "device %d out of range (%d visible)", cfg->device, ndev);
  auto* m = new kp2d_model();
  std::memcpy(&m->cfg, cfg, (size_t)cfg->struct_size);
  m->cfg.struct_size = (int32_t)sizeof(kp2d_config);
  m->cfg.in_channels = cin0;
  if (cfg->channel_dims[0] % 16 || cfg->channel_dims[0] > 256) { delete m; return fail(KP2D_ERR_UNSUPPORTED, "channel_dims[0]=%d (conv1a kernels need a multiple of 16, <= 256)", cfg->channel_dims[0]); }
  if (cfg->nfeatures != 32 && cfg->nfeatures != 64 && cfg->nfeatures != 128) { delete m; return fail(KP2D_ERR_UNSUPPORTED, "nfeatures=%d (32, 64 and 128 are built)", cfg->nfeatures); }
  if (cfg->downsample != 2 && cfg->downsample != 3) { delete m; return fail(KP2D_ERR_UNSUPPORTED, "downsample=%d (2 and 3 are built)", cfg->downsample); }
  if (cfg->n_classes < 1 || cfg->n_classes > 32) { delete m; return fail(KP2D_ERR_UNSUPPORTED, "n_classes must be in [1,32]"); }
  int rc = describe(m);
  if (rc != KP2D_OK) { delete m; return rc; }
  options_from_env(*m, [](const char* name) -> const char* { return getenv(name); });
  *out = m;
  return KP2D_OK;
}

void kp2d_destroy(kp2d_model* m) {
  if (!m) return;
  if (m->blob) (void)hipFree(m->blob);
  for (auto& r : m->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  for (auto st : m->lane_streams) (void)hipStreamDestroy(st);
  for (auto ev : m->lane_events) (void)hipEventDestroy(ev);
  if (m->fork_event) (void)hipEventDestroy(m->fork_event);
  if (m->side_stream) (void)hipStreamDestroy(m->side_stream);
  if (m->side_fork) (void)hipEventDestroy(m->side_fork);
  if (m->side_join) (void)hipEventDestroy(m->side_join);
  delete m;
}

int kp2d_num_weights(const kp2d_model* m) { return m ? (int)m->specs.size() : 0; }

int kp2d_weight_info(const kp2d_model* m, int index, const char** key, int64_t shape[4], int* ndim) {
  if (!m || index < 0 || index >= (int)m->specs.size()) return fail(KP2D_ERR_ARG, "weight index out of range");
  weight_info(m->specs, index, key, shape, ndim, /*pad_shape=*/false);
  return KP2D_OK;
}

int kp2d_set_weight(kp2d_model* m, const char* key, const float* host, const int64_t* shape, int ndim) {
  if (!m || !key || !host || (!shape && ndim > 0)) return fail(KP2D_ERR_ARG, "null argument");
  std::string k(key);
  if (k.size() > 20 && k.compare(k.size() - 20, 20, ".num_batches_tracked") == 0) return KP2D_OK;      // BatchNorm's step counter
  const int rc = set_weight(m->specs, m->spec_index, m->host, key, host, shape, ndim);
  if (rc == KP2D_OK) m->finalized = false;
  return rc;
}

int kp2d_finalize_weights(kp2d_model* m) {
  if (!m) return fail(KP2D_ERR_ARG, "null model");
  std::vector<float> blob;
  int rc = pack(m, blob);
  if (rc == KP2D_OK) rc = upload_blob(m->cfg.device, &m->blob, blob);
  if (rc == KP2D_OK) m->finalized = true;
  return rc;
}

size_t kp2d_packed_bytes(const kp2d_model* m) { return m ? m->blob_floats * sizeof(float) : 0; }

int kp2d_export_packed(const kp2d_model* m, void* dev_dst, void* stream) {
  if (!m || !dev_dst) return fail(KP2D_ERR_ARG, "null argument");
  if (!m->finalized) return fail(KP2D_ERR_STATE, "weights not finalised");
  DeviceGuard guard(m->cfg.device);
  HIP_TRY(hipMemcpyAsync(dev_dst, m->blob, m->blob_floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return KP2D_OK;
}

int kp2d_import_packed(kp2d_model* m, const void* dev_src, void* stream) {
  if (!m || !dev_src) return fail(KP2D_ERR_ARG, "null argument");
  DeviceGuard guard(m->cfg.device);
  if (!m->blob) HIP_TRY(hipMalloc((void**)&m->blob, m->blob_floats * sizeof(float)));
  HIP_TRY(hipMemcpyAsync(m->blob, dev_src, m->blob_floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  m->finalized = true;
  return KP2D_OK;
}

size_t kp2d_vlad_dim(const kp2d_model* m, int H, int W) {
  if (!m) return 0;
  const kp2d_config& g = m->cfg;
  if (g.remove_netvlad) return (size_t)g.encoder_dim * (H >> g.downsample) * (W >> g.downsample);   // vpr.py:84
  if (g.global_descriptor != KP2D_GD_NETVLAD) return (size_t)g.encoder_dim * 16;
  return (size_t)g.num_clusters * g.encoder_dim;
}

size_t kp2d_workspace_bytes(const kp2d_model* m, int B, int H, int W) {
  if (!m || validate_shape(m, B, H, W) != KP2D_OK) return 0;
  kp2d_model* mm = const_cast<kp2d_model*>(m);
  // size for the largest lane count this handle may use (profiling toggles lanes to 1, which needs less)
  const bool prof = mm->profiling;
  mm->profiling = false;
  int nl, chunk;
  const size_t per = schedule(mm, B, H, W, &nl, &chunk);
  mm->profiling = true;
  int nl1, chunk1;
  const size_t per1 = schedule(mm, B, H, W, &nl1, &chunk1);
  mm->profiling = prof;
  return std::max(per * nl, per1);
}

static int forward_impl(kp2d_model* m, const float* x, const uint8_t* frames, int Hs, int Ws, int B, int H, int W,
                        uint32_t flags, float* score, float* shift, float* feat, float* seg, float* vlad, float* depth,
                        void* workspace, size_t workspace_bytes, void* stream) {
  const bool only_enc = (flags & KP2D_FWD_ONLY_ENCODER) != 0;
  if (!m || (!x && !frames) || !vlad || !workspace) return fail(KP2D_ERR_ARG, "null argument");
  if (frames && (Hs < 1 || Ws < 1)) return fail(KP2D_ERR_ARG, "bad source frame size %dx%d", Hs, Ws);
  if (frames && (m->cfg.in_channels != 3 || m->c1 != 16))
    return fail(KP2D_ERR_UNSUPPORTED, "kp2d_forward_frames needs an RGB model with a 16-channel first layer (use kp2d_preprocess + kp2d_forward)");
  if (!only_enc && (!score || !shift || !feat || !seg)) return fail(KP2D_ERR_ARG, "null argument");
  if (!only_enc && m->cfg.depth && !depth) return fail(KP2D_ERR_ARG, "depth=1 model needs the depth output");
  if (!m->finalized) return fail(KP2D_ERR_STATE, "weights not finalised (kp2d_finalize_weights / kp2d_import_packed)");
  int rc = validate_shape(m, B, H, W);
  if (rc != KP2D_OK) return rc;
  if ((uintptr_t)workspace % ALIGN) return fail(KP2D_ERR_WORKSPACE, "workspace must be %zu-byte aligned", ALIGN);
  if (m->seg_ids_dst && !only_enc && m->seg_ids_cap < (size_t)B * (2 * (H >> m->cfg.downsample)) * (2 * (W >> m->cfg.downsample)))
    return fail(KP2D_ERR_ARG, "kp2d_set_seg_ids: buffer of %zu ids is too small for this forward", m->seg_ids_cap);
  int nl, chunk;
  const size_t per = schedule(m, B, H, W, &nl, &chunk);
  if (per == 0) return KP2D_ERR_WORKSPACE;
  if (workspace_bytes < per * nl) return fail(KP2D_ERR_WORKSPACE, "workspace %zu B < required %zu B", workspace_bytes, per * nl);
  const kp2d_config& g = m->cfg;
  // cell grid (score / shift) and dense grid (feat / seg / depth: one pixel-shuffle above the cell grid)
  const size_t Hc = H >> g.downsample, Wc = W >> g.downsample, H2 = 2 * Hc, W2 = 2 * Wc;
  hipStream_t caller = (hipStream_t)stream;
  m->prof_used = 0;
  m->prof_stream = caller;
  DeviceGuard guard(g.device);
  // fork: lanes 1.. run on internal streams that start after everything already queued on the caller's stream
  if (nl > 1) {
    while ((int)m->lane_streams.size() < nl - 1) {
      hipStream_t st; hipEvent_t ev;
      if (m->lane_prio != 0) HIP_TRY(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, m->lane_prio));
      else HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      m->lane_streams.push_back(st); m->lane_events.push_back(ev);
    }
    if (!m->fork_event) HIP_TRY(hipEventCreateWithFlags(&m->fork_event, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(m->fork_event, caller));
    for (int k = 1; k < nl; ++k) HIP_TRY(hipStreamWaitEvent(m->lane_streams[k - 1], m->fork_event, 0));
  }
  int ci = 0;
  rc = KP2D_OK;
  for (int b0 = 0; b0 < B && rc == KP2D_OK; b0 += chunk, ++ci) {
    const int lane = ci % nl;
    Plan P{};
    P.m = m; P.stream = lane == 0 ? caller : m->lane_streams[lane - 1];
    P.ws = (char*)workspace + (size_t)lane * per;
    P.B = std::min(chunk, B - b0); P.H = H; P.W = W; P.b0 = b0;
    P.nlanes = std::min(nl, (B + chunk - 1) / chunk);      // (as schedule() sized the slice)
    P.arena.reset(per);
    FwdOut o{};
    o.x = x ? x + (size_t)b0 * g.in_channels * H * W : nullptr;
    o.frames = frames ? frames + (size_t)b0 * Hs * Ws * 3 : nullptr;
    o.Hs = Hs; o.Ws = Ws;
    o.score = score ? score + (size_t)b0 * Hc * Wc : nullptr;
    o.shift = shift ? shift + (size_t)b0 * 2 * Hc * Wc : nullptr;
    o.feat = feat ? feat + (size_t)b0 * g.nfeatures * H2 * W2 : nullptr;
    o.seg = seg ? seg + (size_t)b0 * g.n_classes * H2 * W2 : nullptr;
    P.seg_ptr = o.seg;
    P.seg_ids = (m->seg_ids_dst && o.seg && !only_enc) ? reinterpret_cast<long long*>(m->seg_ids_dst) + (size_t)b0 * H2 * W2 : nullptr;
    o.vlad = vlad + (size_t)b0 * (only_enc ? (size_t)g.encoder_dim * Hc * Wc : kp2d_vlad_dim(m, H, W));
    o.depth = depth ? depth + (size_t)b0 * H2 * W2 : nullptr;
    build(P, o, flags);
    rc = P.rc;
  }
  // join: the caller's stream continues only after every lane has drained.  This also runs when a launch failed
  // part-way: kernels already queued on the internal streams still write the caller's workspace and outputs, so the
  // caller's stream (and whoever frees those buffers in stream order after the error) must be ordered behind them.
  std::string first_err = rc != KP2D_OK ? g_err : std::string();
  for (int k = 1; k < nl; ++k) {
    hipError_t e = hipEventRecord(m->lane_events[k - 1], m->lane_streams[k - 1]);
    if (e == hipSuccess) e = hipStreamWaitEvent(caller, m->lane_events[k - 1], 0);
    if (e != hipSuccess && rc == KP2D_OK) rc = fail(KP2D_ERR_HIP, "lane join: %s", hipGetErrorString(e));
  }
  if (!first_err.empty()) g_err = first_err;
  return rc;
}

int kp2d_forward(kp2d_model* m, const float* x, int B, int H, int W, uint32_t flags, float* score, float* shift,
                 float* feat, float* seg, float* vlad, float* depth, void* workspace, size_t workspace_bytes,
                 void* stream) {
  if (!x) return fail(KP2D_ERR_ARG, "null argument");
  return forward_impl(m, x, nullptr, 0, 0, B, H, W, flags, score, shift, feat, seg, vlad, depth, workspace, workspace_bytes, stream);
}

int kp2d_forward_frames(kp2d_model* m, const uint8_t* frames, int B, int Hs, int Ws, int H, int W, uint32_t flags,
                        float* score, float* shift, float* feat, float* seg, float* vlad, float* depth, void* workspace,
                        size_t workspace_bytes, void* stream) {
  if (!frames) return fail(KP2D_ERR_ARG, "null argument");
  return forward_impl(m, nullptr, frames, Hs, Ws, B, H, W, flags, score, shift, feat, seg, vlad, depth, workspace, workspace_bytes, stream);
}

int kp2d_post(kp2d_model* m, const float* score, const float* shift, const float* feat, const float* seg, int B,
              int H, int W, int Hc, int Wc, int feat_c, int Hf, int Wf, int seg_c, int Hs, int Ws, float* score_out,
              float* coord, float* desc, int64_t* seg_ids, int sample_segmentation, void* stream) {
  if (!m || !score || !shift || !score_out || !coord) return fail(KP2D_ERR_ARG, "null argument");
  if (desc && !feat) return fail(KP2D_ERR_ARG, "desc requested without feat");
  // seg == NULL with seg_ids: the ids are already there (the forward wrote them, kp2d_set_seg_ids) and are left alone
  if (seg_ids && !seg && sample_segmentation) return fail(KP2D_ERR_ARG, "sampled class ids need the seg tensor");
  if (seg_ids && !seg) seg_ids = nullptr;
  DeviceGuard guard(m->cfg.device);
  PostArgs a{};
  a.score_in = score; a.shift = shift; a.feat = feat; a.score_out = score_out; a.coord = coord; a.desc = desc;
  a.B = B; a.C = feat_c; a.Hc = Hc; a.Wc = Wc; a.Hf = Hf; a.Wf = Wf; a.H = H; a.W = W;
  a.cell = 1 << m->cfg.downsample;
  a.cross_ratio = 2.0f;   // kp2dtiny.py:339
  if (!desc) a.C = 32;
  if (seg_ids && !sample_segmentation) {        // the dense argmax does not depend on the decoded coordinates: one launch
    const ArgmaxArgs g{seg, seg_ids, B, seg_c, Hs * Ws};
    const int e = launch_post_seg(a, g, (hipStream_t)stream);
    if (e) return fail(e < 0 ? KP2D_ERR_UNSUPPORTED : KP2D_ERR_HIP, "post / argmax kernel: %d (descriptor channels %d)", e, feat_c);
    return KP2D_OK;
  }
  int e = launch_post(a, (hipStream_t)stream);
  if (e) return fail(e < 0 ? KP2D_ERR_UNSUPPORTED : KP2D_ERR_HIP, "post kernel: %d (descriptor channels %d)", e, feat_c);
  if (seg_ids && sample_segmentation) {
    SegSampleArgs g{seg, coord, seg_ids, B, seg_c, Hs, Ws, Hc, Wc, H, W};
    e = launch_seg_sample_argmax(g, (hipStream_t)stream);
    if (e) return fail(KP2D_ERR_HIP, "sampled argmax kernel: %d", e);
  } else if (seg_ids) {
    ArgmaxArgs g{seg, seg_ids, B, seg_c, Hs * Ws};
    e = launch_seg_argmax(g, (hipStream_t)stream);
    if (e) return fail(KP2D_ERR_HIP, "argmax kernel: %d", e);
  }
  return KP2D_OK;
}

int kp2d_select_topk(const float* score, int B, int n, int k, float thr, int32_t* idx, float* val, int32_t* count,
                     void* stream) {
  if (!score || !idx || !count) return fail(KP2D_ERR_ARG, "null argument");
  if (B < 1 || n < 1) return fail(KP2D_ERR_ARG, "empty score map (B=%d, n=%d)", B, n);
  if (k < 1) return fail(KP2D_ERR_ARG, "k must be >= 1 (pass k = n for \"every cell above the threshold\")");
  DeviceGuard guard(score, (hipStream_t)stream);
  TopkArgs a{score, B, n, k, thr, idx, val, count};
  int e = launch_topk(a, (hipStream_t)stream);
  if (e) return fail(KP2D_ERR_HIP, "topk kernel: %d", e);
  return KP2D_OK;
}

int kp2d_select_keypoints(const float* score, const float* coord, const float* desc, int B, int C, int n, int k, float thr,
                          int32_t* idx, float* val, int32_t* count, float* pts, float* dsel, void* stream) {
  if (!score || !coord || !desc || !idx || !count || !pts || !dsel) return fail(KP2D_ERR_ARG, "null argument");
  if (B < 1 || n < 1 || C < 1) return fail(KP2D_ERR_ARG, "empty score map (B=%d, n=%d, C=%d)", B, n, C);
  if (k < 1) return fail(KP2D_ERR_ARG, "k must be >= 1 (pass k = n for \"every cell above the threshold\")");
  DeviceGuard guard(score, (hipStream_t)stream);
  // Two launches.  (The gather inside the top-k kernel — the sorted keys are still in LDS — was built and measured: one
  // workgroup per frame fetching k * C scattered values is 20 us slower at a single frame than the 250 workgroups of
  // the gather kernel, 0.276 -> 0.295 ms per frame.)
  const TopkArgs a{score, B, n, k, thr, idx, val, count};
  int e = launch_topk(a, (hipStream_t)stream);
  if (e) return fail(KP2D_ERR_HIP, "topk kernel: %d", e);
  const GatherArgs g{coord, desc, idx, pts, dsel, B, C, n, k};
  e = launch_gather(g, (hipStream_t)stream);
  if (e) return fail(KP2D_ERR_HIP, "gather kernel: %d", e);
  return KP2D_OK;
}

int kp2d_gather_keypoints(const float* coord, const float* desc, const int32_t* idx, int B, int C, int n, int k,
                          float* pts, float* dsel, void* stream) {
  if (!coord || !desc || !idx || !pts || !dsel) return fail(KP2D_ERR_ARG, "null argument");
  DeviceGuard guard(coord, (hipStream_t)stream);
  GatherArgs a{coord, desc, idx, pts, dsel, B, C, n, k};
  int e = launch_gather(a, (hipStream_t)stream);
  if (e) return fail(KP2D_ERR_HIP, "gather kernel: %d", e);
  return KP2D_OK;
}

int kp2d_preprocess(const uint8_t* frames, int B, int Hs, int Ws, float* x, int H, int W, void* stream) {
  if (!frames || !x || B < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1) return fail(KP2D_ERR_ARG, "bad preprocess arguments");
  DeviceGuard guard(x, (hipStream_t)stream);     // the OUTPUT is always device memory (frames may be pinned host memory)
  int e = launch_preprocess(frames, x, B, Hs, Ws, H, W, (hipStream_t)stream);
  if (e) return fail(KP2D_ERR_HIP, "preprocess kernel: %d", e);
  return KP2D_OK;
}

int kp2d_set_profiling(kp2d_model* m, int on) {
  if (!m) return fail(KP2D_ERR_ARG, "null model");
  m->profiling = on != 0;
  m->prof_used = 0;
  return KP2D_OK;
}

int kp2d_profile_count(kp2d_model* m) {
  if (!m) return fail(KP2D_ERR_ARG, "null model");
  if (!m->profiling) return fail(KP2D_ERR_STATE, "profiling is off");
  if (m->prof_used) {
    hipError_t e = hipEventSynchronize(m->prof[m->prof_used - 1].e1);
    if (e != hipSuccess) return fail(KP2D_ERR_HIP, "hipEventSynchronize: %s", hipGetErrorString(e));
  }
  return (int)m->prof_used;
}

int kp2d_profile_get(kp2d_model* m, int index, const char** layer, const char** kernel, float* ms, double* flops,
                     double* bytes) {
  if (!m || index < 0 || (size_t)index >= m->prof_used) return fail(KP2D_ERR_ARG, "profile index out of range");
  ProfRec& r = m->prof[index];
  if (layer) *layer = r.layer.c_str();
  if (kernel) *kernel = r.kernel.c_str();
  if (flops) *flops = r.flops;
  if (bytes) *bytes = r.bytes;
  if (ms) HIP_TRY(hipEventElapsedTime(ms, r.e0, r.e1));
  return KP2D_OK;
}

int kp2d_set_precision(kp2d_model* m, int mode) {
  if (!m || (mode != KP2D_PREC_FP32 && mode != KP2D_PREC_F16X3)) return fail(KP2D_ERR_ARG, "precision must be KP2D_PREC_FP32 or KP2D_PREC_F16X3");
  m->precision = mode;
  m->plan_cache.clear();      // (which layers run merged depends on the arithmetic mode: plan sizes are memoised per mode)
  return KP2D_OK;
}

int kp2d_get_precision(const kp2d_model* m) { return m ? m->precision : KP2D_ERR_ARG; }

int kp2d_set_tap(kp2d_model* m, const char* layer, float* dst, size_t capacity_floats) {
  if (!m) return fail(KP2D_ERR_ARG, "null model");
  if (!layer || !dst) { m->tap_name.clear(); m->tap_dst = nullptr; m->tap_cap = 0; return KP2D_OK; }
  m->tap_name = layer; m->tap_dst = dst; m->tap_cap = capacity_floats;
  return KP2D_OK;
}

int kp2d_set_option(kp2d_model* m, const char* key, long value) {
  if (!m || !key) return fail(KP2D_ERR_ARG, "bad argument");
  m->plan_cache.clear();      // (an option may change the plan: sizes are memoised per setting)
  const int rc = set_option(*m, key, value);
  if (rc == KP2D_OK && !m->side_overlap && m->side_stream) {      // give the stream (and the hardware queue it maps to) back
    DeviceGuard guard(m->cfg.device);
    (void)hipStreamSynchronize(m->side_stream);
    (void)hipStreamDestroy(m->side_stream);
    (void)hipEventDestroy(m->side_fork);
    (void)hipEventDestroy(m->side_join);
    m->side_stream = nullptr; m->side_fork = m->side_join = nullptr;
  }
  return rc;
}

int kp2d_get_option(const kp2d_model* m, const char* key, long* value) {
  if (!m || !key || !value) return fail(KP2D_ERR_ARG, "null argument");
  return get_option(*m, key, value);
}

int kp2d_option_name(int index, const char** key) {
  if (!key || !(*key = option_name(index))) return fail(KP2D_ERR_ARG, "option index out of range");
  return KP2D_OK;
}

int kp2d_set_seg_ids(kp2d_model* m, int64_t* ids, size_t capacity) {
  if (!m) return fail(KP2D_ERR_ARG, "null model");
  m->seg_ids_dst = ids;
  m->seg_ids_cap = ids ? capacity : 0;
  return KP2D_OK;
}

int kp2d_set_chunk_frames(kp2d_model* m, int frames) {
  if (!m || frames < 0) return fail(KP2D_ERR_ARG, "bad argument");
  m->chunk_frames = frames;
  return KP2D_OK;
}

}  // extern "C"
