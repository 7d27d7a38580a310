// The launch plan of one forward: a first-fit arena over the caller's workspace, the activations living in it, and Plan,
// which turns layer names into kernel launches.  build() (plan.cpp) is KP2DTinyV2 / V3.forward as a sequence of Plan calls;
// a dry run of the same sequence sizes the workspace.  kp2d_model is here because the plan reads its options and writes its
// profile; the C ABI around it is kp2d_api.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "api_common.h"
#include "kp2d_kernels.h"
#include "model_desc.h"
#include "options.h"

namespace kp2d {
namespace plan {

struct ProfRec {
  std::string layer, kernel;
  double flops = 0, bytes = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
};

}  // namespace plan
}  // namespace kp2d

struct kp2d_model : kp2d::ModelDesc, kp2d::Options {   // (options.h: the tuning options, their defaults and variables)
  float* blob = nullptr;
  bool finalized = false;
  int chunk_frames = 0;
  int precision = KP2D_PREC_F16X3;
  std::map<uint64_t, size_t> plan_cache;
  std::vector<hipStream_t> lane_streams;   // Options::lanes: independent sub-batches run concurrently on that many HIP streams; +3 %
  std::vector<hipEvent_t> lane_events;
  hipEvent_t fork_event = nullptr;
  // single frames (the level schedule of build()): NetVLAD's launches on a side stream beside the segmentation head's chain
  hipStream_t side_stream = nullptr;
  hipEvent_t side_fork = nullptr, side_join = nullptr;
  bool profiling = false;
  int64_t* seg_ids_dst = nullptr;   // kp2d_set_seg_ids: class ids [B,1,H2,W2] written by the forward's last segmentation layer
  size_t seg_ids_cap = 0;
  std::string tap_name;   // kp2d_set_tap: one intermediate activation copied out (planar) during forward
  float* tap_dst = nullptr;
  size_t tap_cap = 0;
  std::vector<kp2d::plan::ProfRec> prof;
  size_t prof_used = 0;
  hipStream_t prof_stream = nullptr;
};

namespace kp2d {
namespace plan {

// first-fit arena over the caller's workspace
struct Arena {
  struct Blk { size_t off, size; };
  std::vector<Blk> free_;
  size_t cap = 0, high = 0;
  void reset(size_t capacity) { cap = capacity; free_.assign(1, Blk{0, capacity}); high = 0; }
  size_t alloc(size_t bytes);   // (size_t)-1: exhausted
  void release(size_t off, size_t bytes);
};

// NHWC activation living in the workspace
struct Act {
  size_t off = 0, bytes = 0;
  int C = 0, H = 0, W = 0;
  int PS = 0, CO = 0;  // channel-slice view of a wider tensor: pixel stride (0 = C) and first channel; bytes = 0 (not owned)
  int fmt = 0;         // 1: an S16P tensor (kp2d_kernels.h: the fp16 halves of the split, planar rows; same bytes); a view is a run of whole chunks
};

// where a conv launch stores: pointer, pixel stride in channels, first channel (ConvArgs out / os / oo)
struct ConvOut {
  float* p = nullptr;
  int ps = 0, co = 0;
};

struct FwdOut {
  const uint8_t* frames = nullptr;   // kp2d_forward_frames: uint8 [B,Hs,Ws,3]; x is null then
  int Hs = 0, Ws = 0;
  const float* x;
  float *score, *shift, *feat, *seg, *vlad, *depth;
};

struct Plan {
  kp2d_model* m;
  hipStream_t stream;
  char* ws;
  Arena arena;
  bool dry = false;       // only size the arena: nothing is launched and ptr() is null
  int B, H, W;
  int b0 = 0;             // first frame of this sub-batch in the caller's batch
  const float* seg_ptr = nullptr;   // this sub-batch's slice of the caller's seg output and of the class-id map
  long long* seg_ids = nullptr;     // (kp2d_set_seg_ids): the layer that writes seg also writes its per-pixel argmax
  int nlanes = 1;         // stream lanes of this forward (conv3x3_wsm.hip sizes its grid by it)
  int rc = KP2D_OK;       // the first error; every later launch is skipped
  const float* stem_x = nullptr;   // the frames, when conv1b's launch computes conv1a itself (build())
  // Independent layers of one level as ONE launch (conv3x3_f16.hip::conv3x3_f16x3_multi_kernel; small grids only): between
  // group_begin() and group_end() the 3x3 split-fp16 launches are collected instead of enqueued.  Their inputs must not be
  // released — and no tap taken — before group_end(): the caller's job (build()).
  bool grouping = false;
  bool no_levels = false;   // dry runs: size the head-by-head schedule too (plan_bytes_uncached takes the larger)
  std::vector<ConvArgs> pending;
  std::vector<std::string> pending_names;

  // ---- primitives: the only readers of `dry` ----
  bool live() const { return !dry && rc == KP2D_OK; }
  float* ptr(const Act& a) const { return dry ? nullptr : reinterpret_cast<float*>(ws + a.off); }
  // THE launch path: enqueue() returns 0, a hipError_t, or a negative "unsupported shape" code of the launchers
  template <class F>
  void launch(const char* what, F&& enqueue) {
    if (live()) check(enqueue(), what);
  }
  // ... with one record of the per-layer profile around it (kp2d_set_profiling)
  template <class F>
  void launch(const std::string& layer, const char* kernel, double flops, double bytes, F&& enqueue) {
    launch(layer.c_str(), [&] {
      prof_begin(layer, kernel, flops, bytes);
      const int e = enqueue();
      prof_end();
      return e;
    });
  }
  void group_begin();
  void group_end();
  void tap(const std::string& name, const Act& a);   // kp2d_set_tap: copy `a` out when it is the tapped layer

  void check(int e, const char* what);
  void prof_begin(const std::string& layer, const char* kernel, double flops, double bytes);
  void prof_end();

  // ---- workspace ----
  Act alloc_bytes(size_t bytes);
  Act alloc(int C, int H_, int W_);
  void release(const Act& a) { if (a.bytes) arena.release(a.off, a.bytes); }
  static Act view(const Act& parent, int c, int o);   // channels [o, o + c) of parent; released by releasing the parent
  ConvOut out(const Act& a) const { return ConvOut{ptr(a), a.C, 0}; }

  // ---- the model's layers by name; a name it lacks sets rc (KP2D_ERR_ARG) and yields an empty one ----
  const ConvPack& layer(const std::string& name);
  const VecPack& vec(const std::string& name);

  // ---- launches ----
  static ConvSrc dense(const float* p, const Act& t, int c, int o);
  bool conv_args(const ConvPack& c, const ConvSrc& s0, const ConvSrc& s1, int act, int store, int nsplit, int Hc, int Wc,
                 ConvOut out, ConvOut second, ConvArgs& a);
  // core launch, sources already described.  `out` is the layer's output (the pooled tensor of a *_POOL store); `second`
  // the pooled tensor of a *_BOTH store, the S16P part of ST_MIX16, the channels from nsplit on of ST_NCHW.
  void conv_src(const std::string& name, const ConvSrc& s0, const ConvSrc& s1, int act, int store, int nsplit, int Hc, int Wc,
                ConvOut out, ConvOut second = {});
  // the same over dense NHWC activations: channels [o0, o0 + c0) of in0, then all of in1 (null: no concat)
  void conv(const std::string& name, const Act& in0, int c0, int o0, const Act* in1, int act, int store, int nsplit, int Hc, int Wc,
            ConvOut out, ConvOut second = {});
  void head_pair(const std::string& n0, const Act& in0, int act0, float* out0, const std::string& n1, const Act& in1, int act1,
                 float* out1, int Hc, int Wc);
  Act pw(const std::string& name, const Act& in, int act, int store = ST_NHWC);                          // 1x1 conv
  Act cbr(const std::string& name, const Act& in0, const Act* in1, int store, Act* pooled = nullptr);   // conv + BN + (Leaky)ReLU
  Act layernorm(const std::string& prefix, const Act& in);
  Act attention_module(const std::string& p, const Act& x, bool pool);
  bool mff_fusable(int C) const { return m->mff_fused && m->precision == KP2D_PREC_F16X3 && C == 64; }
  Act mff_tail(const std::string& p, const Act& f0, int C, int h, int w, bool pool);
};

// KP2DTinyV2.forward / KP2DTinyV3.forward as a launch sequence on P
void build(Plan& P, const FwdOut& o, uint32_t flags);

int validate_shape(const kp2d_model* m, int B, int H, int W);
// Sub-batch schedule shared by kp2d_workspace_bytes and kp2d_forward: `lanes` concurrent streams, each working
// through ceil(nchunks / lanes) sub-batches of `chunk` frames in its own slice of the workspace.  Returns the size of a
// slice: the plan of one sub-batch with the lanes that actually run side by side (fewer when there are fewer sub-batches).
size_t schedule(kp2d_model* m, int B, int H, int W, int* lanes, int* chunk);

}  // namespace plan
}  // namespace kp2d
