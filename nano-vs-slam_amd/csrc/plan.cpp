// Plan's members, build() and the workspace sizing around it: see plan.h.
#include "plan.h"

#include <algorithm>
#include <cmath>

#include "device_guard.h"
#include "netvlad_form.h"

namespace kp2d {
namespace plan {

size_t Arena::alloc(size_t bytes) {
  bytes = align_up(bytes);
  for (size_t i = 0; i < free_.size(); ++i) {
    if (free_[i].size >= bytes) {
      const size_t off = free_[i].off;
      free_[i].off += bytes;
      free_[i].size -= bytes;
      if (free_[i].size == 0) free_.erase(free_.begin() + i);
      high = std::max(high, off + bytes);
      return off;
    }
  }
  return (size_t)-1;
}

void Arena::release(size_t off, size_t bytes) {
  bytes = align_up(bytes);
  free_.push_back(Blk{off, bytes});
  std::sort(free_.begin(), free_.end(), [](const Blk& a, const Blk& b) { return a.off < b.off; });
  for (size_t i = 0; i + 1 < free_.size();) {
    if (free_[i].off + free_[i].size == free_[i + 1].off) {
      free_[i].size += free_[i + 1].size;
      free_.erase(free_.begin() + i + 1);
    } else {
      ++i;
    }
  }
}

namespace {

// What a store kind (conv_args.h Store) means for the plan: the shape and layout of the layer's output, whether a second
// tensor goes with it, and which of the launch's two output descriptors the layer's output travels in (a *_POOL store
// writes its only tensor through the second: ConvArgs::out1 is "the pooled activation" for *_POOL and *_BOTH alike).
enum Shape { SAME, HALVED, SHUFFLED };   // [cout, H, W], [cout, H / 2, W / 2], [cout / 4, 2 H, 2 W]
struct StoreKind { Shape shape; int fmt; bool two; bool out_in_second; };
const StoreKind kStore[] = {
    /* ST_NHWC         */ {SAME, 0, false, false},
    /* ST_NHWC_POOL    */ {HALVED, 0, false, true},
    /* ST_NHWC_BOTH    */ {SAME, 0, true, false},
    /* ST_SHUFFLE      */ {SHUFFLED, 0, false, false},
    /* ST_NCHW         */ {SAME, 0, true, false},
    /* ST_S16P         */ {SAME, 1, false, false},
    /* ST_S16P_POOL    */ {HALVED, 1, false, true},
    /* ST_S16P_BOTH    */ {SAME, 1, true, false},
    /* ST_S16P_SHUFFLE */ {SHUFFLED, 1, false, false},
    /* ST_MIX16        */ {SAME, 0, true, false},
    /* ST_IDS          */ {SAME, 0, false, false},
};
static_assert(ST_NHWC == 0 && ST_NHWC_POOL == 1 && ST_NHWC_BOTH == 2 && ST_SHUFFLE == 3 && ST_NCHW == 4 && ST_S16P == 5 &&
              ST_S16P_POOL == 6 && ST_S16P_BOTH == 7 && ST_S16P_SHUFFLE == 8 && ST_MIX16 == 9 && ST_IDS == 10, "kStore is indexed by Store");

// score / loc / depth heads: 1-4 output channels as an HBM-bound dot-product kernel (exact fp32 in both modes)
bool head_dot(const ConvPack& c, int store, int concat_channels, int act) {
  return c.head() && store == ST_NCHW && concat_channels == 0 && act != ACT_SOFTMAX_C;
}
void head_dot_args(const kp2d_model* m, const ConvPack& c, ConvArgs& a) {
  a.prec = 0;
  a.w = m->blob + c.wd_off;
  a.scale = m->blob + c.sc_off;
}

}  // namespace

void Plan::group_begin() {
  if (!live() || m->profiling || m->tap_dst || !m->multi_launch) return;      // (profiles and taps: one launch per layer)
  grouping = true;
}

void Plan::group_end() {
  grouping = false;
  if (pending.empty()) return;
  int e = -1000;      // (what the multi launcher answers when the layers are not all its kind: one launch each then)
  if (pending.size() >= 2)
    launch(pending_names[0].c_str(), [&] {
      e = launch_conv3x3_f16x3_multi(pending.data(), (int)pending.size(), stream);
      return e == -1000 ? 0 : e;
    });
  if (e == -1000)
    for (size_t i = 0; i < pending.size(); ++i)
      launch(pending_names[i].c_str(), [&] { return launch_conv3x3(pending[i], 16, stream); });
  pending.clear();
  pending_names.clear();
}

// copy activation `a` (this sub-batch's frames) to the caller's planar [B,C,H,W] buffer
void Plan::tap(const std::string& name, const Act& a) {
  if (!live() || !m->tap_dst || name != m->tap_name) return;
  const size_t per = (size_t)a.C * a.H * a.W;
  if (((size_t)b0 + B) * per > m->tap_cap) { rc = fail(KP2D_ERR_ARG, "tap '%s': buffer holds %zu floats, needs %zu", name.c_str(), m->tap_cap, ((size_t)b0 + B) * per); return; }
  float* dst = m->tap_dst + (size_t)b0 * per;
  const int ps = a.PS ? a.PS : a.C;
  launch(name.c_str(), [&] {
    return a.fmt == 1 ? launch_s16p_to_nchw(ptr(a), dst, B, a.C, a.H, a.W, ps, a.CO, stream)
                      : launch_nhwc_to_nchw(ptr(a), dst, B, a.C, a.H * a.W, ps, a.CO, stream);
  });
}

void Plan::check(int e, const char* what) {
  if (e != 0 && rc == KP2D_OK) rc = fail(KP2D_ERR_HIP, "%s: launch failed (%d: %s)", what, e,
                                         e > 0 ? hipGetErrorString((hipError_t)e) : "unsupported shape");
}

void Plan::prof_begin(const std::string& layer, const char* kernel, double flops, double bytes) {
  if (!m->profiling) return;
  if (m->prof_used == m->prof.size()) {
    ProfRec r;
    (void)hipEventCreate(&r.e0);
    (void)hipEventCreate(&r.e1);
    m->prof.push_back(r);
  }
  ProfRec& r = m->prof[m->prof_used];
  r.layer = layer; r.kernel = kernel; r.flops = flops; r.bytes = bytes;
  (void)hipEventRecord(r.e0, stream);
}

void Plan::prof_end() {
  if (!m->profiling) return;
  (void)hipEventRecord(m->prof[m->prof_used].e1, stream);
  ++m->prof_used;
}

Act Plan::alloc_bytes(size_t bytes) {
  Act a;
  a.bytes = bytes;
  a.off = arena.alloc(bytes);
  if (a.off == (size_t)-1 && rc == KP2D_OK) rc = fail(KP2D_ERR_WORKSPACE, "workspace exhausted");
  return a;
}

Act Plan::alloc(int C, int H_, int W_) {
  Act a = alloc_bytes((size_t)B * H_ * W_ * C * sizeof(float));
  a.C = C; a.H = H_; a.W = W_;
  return a;
}

Act Plan::view(const Act& parent, int c, int o) {
  Act v = parent;
  v.bytes = 0; v.C = c; v.PS = parent.PS ? parent.PS : parent.C; v.CO = parent.CO + o;
  return v;
}

const ConvPack& Plan::layer(const std::string& name) {
  static const ConvPack none;
  if (const ConvPack* c = m->conv(name)) return *c;
  if (rc == KP2D_OK) rc = fail(KP2D_ERR_ARG, "plan: the model has no layer '%s'", name.c_str());
  return none;
}

const VecPack& Plan::vec(const std::string& name) {
  static const VecPack none;
  const auto it = m->vecs.find(name);
  if (it != m->vecs.end()) return it->second;
  if (rc == KP2D_OK) rc = fail(KP2D_ERR_ARG, "plan: the model has no vector '%s'", name.c_str());
  return none;
}

ConvSrc Plan::dense(const float* p, const Act& t, int c, int o) {
  ConvSrc s{};
  const int ps = t.PS ? t.PS : t.C;
  s.p = p; s.c = c; s.o = o + t.CO;
  s.ps = ps; s.rs = (long)t.W * ps; s.bs = (long)t.H * t.W * ps;
  s.fmt = t.fmt;
  return s;
}

// arguments of one conv launch; false (rc set) when the plan and the layer disagree
bool Plan::conv_args(const ConvPack& c, const ConvSrc& s0, const ConvSrc& s1, int act, int store, int nsplit, int Hc, int Wc,
                     ConvOut out, ConvOut second, ConvArgs& a) {
  const ConvOut o0 = kStore[store].out_in_second ? ConvOut{} : out, o1 = kStore[store].out_in_second ? out : second;
  a = ConvArgs{};
  a.in0 = s0; a.in1 = s1; a.taps = c.taps;
  const bool split = m->precision == KP2D_PREC_F16X3;
  a.dbg = m->dbg;
  a.prec = split ? 1 : 0;
  a.ids_out = ((store == ST_NCHW || store == ST_IDS) && seg_ids && o0.p && o0.p == seg_ptr && nsplit == c.cout && c.npad == 32) ? seg_ids : nullptr;
  a.wsm_min = m->wsm_min;
  a.wsm_grid = m->wsm_grid;
  a.wsm_tr = m->wsm_tr;
  a.ws_min = m->ws_min;
  a.wsm_lanes = nlanes;
  a.s16_min = m->s16_min;
  // S16P tensors beyond the 32-channel stage are read and written by conv3x3_wsm.hip only: build() fixed the layout
  // after asking wsm_would_run (conv_policy.h), which then skips its item-count policy
  a.wsm_force = ((s0.fmt == 1 && !(c.cin == 32 && s1.c == 0) && store != ST_NCHW && store != ST_IDS) || store == ST_S16P_SHUFFLE || store == ST_MIX16 ||
                 (store == ST_S16P && c.npad >= 64)) ? 1 : 0;
  if (stem_x && c.name == "backbone.conv1b") {
    a.stem_x = stem_x; a.stem_w = m->blob + m->conv1a_w; a.stem_scale = m->blob + m->conv1a_sc; a.stem_shift = m->blob + m->conv1a_sh;
    a.stem_wscale = m->blob + m->conv1a_ws; a.stem_act = m->cfg.leaky_relu ? ACT_LEAKY : ACT_RELU;
  }
  a.w = m->blob + (split ? c.w16_off : c.w_off);
  a.w_tr = (split && c.w16t_off) ? m->blob + c.w16t_off : nullptr;
  a.tiles_x = (Wc + 15) / 16; a.tiles_y = (Hc + 15) / 16;
  if (split && s0.fmt == 0 && !a.wsm_force && use_ng32(B, Hc, Wc, c.npad, m->wsm_min)) {      // (S16P tensors: 64-channel groups)
    a.w = m->blob + c.w16n_off;
    a.ng32 = 1;
  }
  a.scale = m->blob + (split ? c.sc16_off : c.sc_off);
  a.shift = m->blob + c.sh_off;
  a.out0 = o0.p; a.os0 = o0.ps; a.oo0 = o0.co; a.out1 = o1.p; a.os1 = o1.ps; a.oo1 = o1.co;
  a.B = B; a.H = Hc; a.W = Wc; a.cin = c.cin; a.cout = c.cout; a.npad = c.npad;
  a.act = act; a.store = store; a.nsplit = nsplit;
  if (s0.c + s1.c != c.cin) { rc = fail(KP2D_ERR_ARG, "%s: plan feeds %d channels, layer expects %d", c.name.c_str(), s0.c + s1.c, c.cin); return false; }
  return true;
}

void Plan::conv_src(const std::string& name, const ConvSrc& s0, const ConvSrc& s1, int act, int store, int nsplit, int Hc, int Wc,
                    ConvOut out, ConvOut second) {
  const ConvPack& c = layer(name);
  const bool split = m->precision == KP2D_PREC_F16X3;
  const double px = (double)B * Hc * Wc;
  ConvArgs a;
  auto args = [&] { return conv_args(c, s0, s1, act, store, nsplit, Hc, Wc, out, second, a); };
  if (head_dot(c, store, s1.c, act)) {
    launch(name, "conv3x3_head", 2.0 * 9 * c.cin * c.cout * px, 4.0 * px * (c.cin + c.cout) + 4.0 * 9 * c.cin * c.cout, [&] {
      if (!args()) return 0;
      head_dot_args(m, c, a);
      return launch_head3x3(a, stream);
    });
  } else if (grouping && split && c.taps == 9 && pending.size() < 4) {
    if (live() && args()) {
      pending.push_back(a);
      pending_names.push_back(name);
    }
  } else {
    const char* fam = split ? (c.taps == 9 ? "conv3x3_f16x3" : "conv1x1_f16x3")
                            : (c.taps == 9 ? (c.kc == 16 ? "conv3x3_f32<16>" : "conv3x3_f32<8>") : "conv1x1_f32");
    // conv1a computed inside conv1b's launch: its products count, its input is the 3-channel frame
    const bool stem = stem_x && name == "backbone.conv1b";
    // (ST_IDS: the products are all there, the logits are not written — one int64 per pixel leaves)
    const double out_bytes = store == ST_IDS ? 8.0 * px : 4.0 * px * c.cout;
    launch(name, fam, stem ? 2.0 * 9 * (3.0 * 16 + c.cin * c.cout) * px : 2.0 * c.taps * c.cin * c.cout * px,
           stem ? 4.0 * px * (3 + c.cout / 4.0) + 4.0 * 9 * c.cin * c.cout : 4.0 * px * c.cin + out_bytes + 4.0 * c.taps * c.cin * c.cout, [&] {
      if (!args()) return 0;
      const int e = launch_conv3x3(a, split ? 16 : c.kc, stream);
      if (m->profiling) m->prof[m->prof_used].kernel += conv3x3_last_variant();      // which tile form ran
      return e;
    });
  }
}

void Plan::conv(const std::string& name, const Act& in0, int c0, int o0, const Act* in1, int act, int store, int nsplit, int Hc, int Wc,
                ConvOut out, ConvOut second) {
  conv_src(name, dense(ptr(in0), in0, c0, o0), in1 ? dense(ptr(*in1), *in1, in1->C, 0) : dense(ptr(in0), in0, 0, 0), act, store,
           nsplit, Hc, Wc, out, second);
}

// KP2DTinyV2's score head (-> 1 channel, sigmoid) and location head (-> 2, tanh): planar outputs, one launch for both
// when both run as dot-product kernels (per-layer profiling keeps them apart)
void Plan::head_pair(const std::string& n0, const Act& in0, int act0, float* out0, const std::string& n1, const Act& in1, int act1,
                     float* out1, int Hc, int Wc) {
  const ConvPack& c0 = layer(n0);
  const ConvPack& c1 = layer(n1);
  // few frames only: at 64 frames the two launches overlap their tails and the pair is 0.4 % of the step slower
  // (21.16k vs 21.24k frames/s, three alternating runs); at one frame it saves a 4-us launch (0.273 -> 0.265 ms)
  const bool pair_on = (long)((Wc + 15) / 16) * ((Hc + 3) / 4) * B < 1024;
  if (!pair_on || m->profiling || !head_dot(c0, ST_NCHW, 0, act0) || !head_dot(c1, ST_NCHW, 0, act1) || c0.cout != 1 || c1.cout != 2) {
    conv(n0, in0, in0.C, 0, nullptr, act0, ST_NCHW, c0.cout, Hc, Wc, {out0});
    conv(n1, in1, in1.C, 0, nullptr, act1, ST_NCHW, c1.cout, Hc, Wc, {out1});
    return;
  }
  launch(n0.c_str(), [&] {
    ConvArgs a0, a1;
    if (!conv_args(c0, dense(ptr(in0), in0, in0.C, 0), dense(ptr(in0), in0, 0, 0), act0, ST_NCHW, c0.cout, Hc, Wc, {out0}, {}, a0)) return 0;
    if (!conv_args(c1, dense(ptr(in1), in1, in1.C, 0), dense(ptr(in1), in1, 0, 0), act1, ST_NCHW, c1.cout, Hc, Wc, {out1}, {}, a1)) return 0;
    head_dot_args(m, c0, a0);
    head_dot_args(m, c1, a1);
    return launch_head3x3_pair(a0, a1, stream);
  });
}

// 1x1 conv -> NHWC activation (ST_NHWC_POOL: pooled)
Act Plan::pw(const std::string& name, const Act& in, int act, int store) {
  const ConvPack& c = layer(name);
  const bool pool = store == ST_NHWC_POOL;
  Act o = pool ? alloc(c.cout, in.H / 2, in.W / 2) : alloc(c.cout, in.H, in.W);
  conv(name, in, in.C, 0, nullptr, act, pool ? ST_NHWC_POOL : ST_NHWC, 0, in.H, in.W, out(o));
  tap(name, o);              // (pooled: the pooled tensor, as in cbr)
  return o;
}

Act Plan::layernorm(const std::string& prefix, const Act& in) {
  Act o = alloc(in.C, in.H, in.W);
  const VecPack &g = vec(prefix + ".g"), &b = vec(prefix + ".b");
  const double px = (double)B * in.H * in.W;
  launch(prefix, "channel_layernorm", 8.0 * px * in.C, 8.0 * px * in.C, [&] {
    LnArgs a{ptr(in), m->blob + g.off, m->blob + b.off, ptr(o), (long)B * in.H * in.W, in.C};
    return launch_channel_layernorm(a, stream);
  });
  return o;
}

// SegFormerAttentionModule.forward (modules/segformer.py:217-220); `pool` folds the following MaxPool2d(2,2)
Act Plan::attention_module(const std::string& p, const Act& x, bool pool) {
  const int C = x.C, h = x.H, w = x.W;
  Act ln1 = layernorm(p + ".att.norm", x);
  tap(p + ".att.norm", ln1);
  Act q = pw(p + ".att.fn.to_q", ln1, ACT_NONE);
  Act kv = alloc(2 * C, h / 2, w / 2);
  {
    // 2x2 stride-2 conv == 1x1 conv over [row 2Y | row 2Y+1], each row-view a 2C-channel "pixel" (x, x+1)
    ConvSrc s0{};
    s0.p = ptr(ln1); s0.c = 2 * C; s0.o = 0; s0.ps = 2 * C; s0.rs = 2L * w * C; s0.bs = (long)h * w * C;
    ConvSrc s1 = s0;
    if (s1.p) s1.p += (long)w * C;
    conv_src(p + ".att.fn.to_kv", s0, s1, ACT_NONE, ST_NHWC, 0, h / 2, w / 2, out(kv));
  }
  tap(p + ".att.fn.to_kv", kv);
  release(ln1);
  Act ao = alloc(C, h, w);
  {
    const int heads = 4;
    const int prec = m->precision == KP2D_PREC_F16X3 ? 1 : 0;
    const double st = (double)B * h * w * (h / 2) * (w / 2);
    launch(p + ".att.fn", (prec == 1 && C / heads <= 16) ? "attention_f16x3" : "attention", 4.0 * st * C,
           4.0 * B * ((double)2 * h * w * C + (h / 2) * (w / 2) * 2.0 * C), [&] {
      AttnArgs a{ptr(q), ptr(kv), ptr(ao), B, h * w, (h / 2) * (w / 2), C, heads, 1.0f / std::sqrt((float)(C / heads))};
      a.prec = prec;
      return launch_attention(a, stream);
    });
  }
  tap(p + ".att.fn", ao);      // the attention output in front of to_out
  release(q);
  release(kv);
  Act t = pw(p + ".att.fn.to_out", ao, ACT_NONE);
  release(ao);
  tap(p + ".att", t);
  Act ln2 = layernorm(p + ".mff.norm", t);
  tap(p + ".mff.norm", ln2);
  release(t);
  Act f0 = pw(p + ".mff.fn.net.0", ln2, ACT_NONE);
  release(ln2);
  if (mff_fusable(C) && f0.C == 128) {
    Act f3 = mff_tail(p, f0, C, h, w, pool);
    release(f0);
    tap(p + ".mff", f3);
    return f3;
  }
  Act f1 = alloc(f0.C, h, w);
  {
    const VecPack &dw = vec(p + ".mff.fn.net.1.net.0.weight"), &db = vec(p + ".mff.fn.net.1.net.0.bias");
    const double px = (double)B * h * w;
    launch(p + ".mff.fn.net.1.net.0", "dwconv3x3", 18.0 * px * f0.C, 8.0 * px * f0.C, [&] {
      DwArgs a{ptr(f0), m->blob + dw.off, m->blob + db.off, ptr(f1), B, h, w, f0.C};
      return launch_dwconv3x3(a, stream);
    });
  }
  release(f0);
  tap(p + ".mff.fn.net.1.net.0", f1);      // (three-launch path only: the fused tail never writes this tensor)
  Act f2 = pw(p + ".mff.fn.net.1.net.1", f1, ACT_GELU);
  release(f1);
  Act f3 = pw(p + ".mff.fn.net.3", f2, ACT_NONE, pool ? ST_NHWC_POOL : ST_NHWC);
  release(f2);
  tap(p + ".mff", f3);         // pooled when the module folds the following MaxPool2d
  return f3;
}

// the same module with MixFeedForward's tail as ONE launch (mff_tail.hip): f16x3 arithmetic, 64 -> 128 -> 64 widths
Act Plan::mff_tail(const std::string& p, const Act& f0, int C, int h, int w, bool pool) {
  Act f3 = alloc(C, pool ? h / 2 : h, pool ? w / 2 : w);
  const ConvPack& c1 = layer(p + ".mff.fn.net.1.net.1");
  const ConvPack& c3 = layer(p + ".mff.fn.net.3");
  const VecPack &dw = vec(p + ".mff.fn.net.1.net.0.weight"), &db = vec(p + ".mff.fn.net.1.net.0.bias");
  const double px = (double)B * h * w;
  launch(p + ".mff.fn.net.1-3", "mff_tail", px * (18.0 * 128 + 2.0 * 128 * 128 + 2.0 * 128 * 64), 4.0 * px * (128 + (pool ? 16 : 64)), [&] {
    MffTailArgs a{};
    a.h = ptr(f0);
    a.wdw = m->blob + dw.off;
    a.bdw = m->blob + db.off;
    a.w1 = m->blob + c1.w16_off; a.sc1 = m->blob + c1.sc16_off; a.sh1 = m->blob + c1.sh_off;
    a.w3 = m->blob + c3.w16_off; a.sc3 = m->blob + c3.sc16_off; a.sh3 = m->blob + c3.sh_off;
    a.out = ptr(f3); a.B = B; a.H = h; a.W = w; a.pool = pool ? 1 : 0;
    return launch_mff_tail(a, stream);
  });
  return f3;
}

// CBR -> NHWC activation (optionally pooled / pooled + full / pixel-shuffled / S16P: kStore)
Act Plan::cbr(const std::string& name, const Act& in0, const Act* in1, int store, Act* pooled) {
  const ConvPack& c = layer(name);
  const StoreKind& k = kStore[store];
  const int Hc = in0.H, Wc = in0.W;
  Act o = k.shape == HALVED ? alloc(c.cout, Hc / 2, Wc / 2) : k.shape == SHUFFLED ? alloc(c.cout / 4, Hc * 2, Wc * 2) : alloc(c.cout, Hc, Wc);
  o.fmt = k.fmt;
  if (k.two) {
    *pooled = alloc(c.cout, Hc / 2, Wc / 2);
    pooled->fmt = k.fmt;
  }
  conv(name, in0, in0.C, 0, in1, m->cfg.leaky_relu ? ACT_LEAKY : ACT_RELU, store, 0, Hc, Wc, out(o), k.two ? out(*pooled) : ConvOut{});
  tap(name, o);              // ST_NHWC_POOL: the pooled tensor (the full-resolution one is never written)
  return o;
}

// KP2DTinyV2.forward (kp2dtiny.py:552-591) / KP2DTinyV3.forward (:906-957) as a launch sequence
void build(Plan& P, const FwdOut& o, uint32_t flags) {
  kp2d_model* m = P.m;
  const kp2d_config& g = m->cfg;
  const bool v3 = g.version == 3;
  const int lk = g.leaky_relu ? ACT_LEAKY : ACT_RELU;
  const int H = P.H, W = P.W, B = P.B;
  const int cus = device_cu_count();      // (conv_policy.h: the persistent forms' grids, CUs / lanes)

  // ---- backbone (encoders.py:105-129) ----
  // Big grids: conv1a inside conv1b's launch (conv3x3_f16.hip STEM) — its output, the largest tensor of the forward after
  // `skip`, is never written.  Float frames, RGB, 16 -> 32 first stage, split-fp16 arithmetic, a pooled conv1b on the
  // warp-specialised form; a tap on conv1a keeps the two launches (the fused layer has no output to copy).
  // The first layer in the split-fp16 arithmetic (RGB frames, 16 channels): one set of bits whether it runs fused, as its own
  // launch, or straight from uint8 frames — so a forward's results do not depend on the grid size that picks the form.
  const bool c1a_split = m->stem_fusion != 0 && m->precision == KP2D_PREC_F16X3 && g.in_channels == 3 && m->c1 == 16;
  const bool stem = c1a_split && m->stem_fusion == 1 && !o.frames && m->c2 == 32 && g.downsample >= 2 && ws_map_ok(B, H, W, m->ws_min) &&
                    !(m->tap_dst && m->tap_name == "backbone.conv1a");
  Act t1a = P.alloc(m->c1, H, W);      // (allocated either way: the workspace size must not depend on the input kind or on a tap)
  if (stem) {
    P.stem_x = o.x;
  } else {
    const std::string name = "backbone.conv1a";
    const double px = (double)B * H * W;
    auto args = [&] {
      Conv1aArgs a{};
      a.x = o.x; a.w = m->blob + m->conv1a_w; a.scale = m->blob + m->conv1a_sc; a.shift = m->blob + m->conv1a_sh;
      a.out = P.ptr(t1a); a.B = B; a.H = H; a.W = W; a.cout = m->c1; a.act = lk; a.cin = g.in_channels;
      return a;
    };
    if (c1a_split)
      P.launch(name, o.frames ? "conv1a_mfma_u8" : "conv1a_mfma", 2.0 * 27 * m->c1 * px,
               (o.frames ? 3.0 * B * o.Hs * o.Ws : 12.0 * px) + 4.0 * px * m->c1,
               [&] { return launch_conv1a_mfma(args(), m->blob + m->conv1a_ws, o.frames, o.Hs, o.Ws, P.stream); });
    else if (o.frames)
      P.launch(name, "conv1a_u8", 2.0 * 27 * m->c1 * px, 3.0 * B * o.Hs * o.Ws + 4.0 * px * m->c1,
               [&] { return launch_conv1a_u8(args(), o.frames, o.Hs, o.Ws, P.stream); });
    else
      P.launch(name, "conv1a", 2.0 * 9 * g.in_channels * m->c1 * px, 4.0 * px * (g.in_channels + m->c1),
               [&] { return launch_conv1a(args(), P.stream); });
  }
  P.tap("backbone.conv1a", t1a);
  // The 32-channel stage conv1b -> conv2a -> conv2b -> conv3a -> conv3b with its four inner tensors kept SPLIT (S16P,
  // kp2d_kernels.h): the consumers copy their operand images HBM -> LDS without a vector instruction (conv3x3_s16.hip; these
  // layers are bound by HBM and by their staging, not by the matrix cores).  Same values bit for bit.  Decided here, for
  // the whole chain, because the layout has exactly one reader and two writers: S configs (16 -> 32 -> 32 -> 32 -> 64, two
  // pools), split-fp16 arithmetic, and a grid big enough for the persistent forms of both ends.
  const bool s16 = m->precision == KP2D_PREC_F16X3 && g.downsample == 2 && m->c1 == 16 && m->c2 == 32 && m->c3 == 32 && m->c4 == 64 &&
                   ws_map_ok(B, H, W, m->ws_min) && s16_would_run(B, H / 2, W / 2, cus, P.nlanes, m->s16_min, m->wsm_grid);
  Act p1 = P.cbr("backbone.conv1b", t1a, nullptr, s16 ? ST_S16P_POOL : (g.downsample >= 2 ? ST_NHWC_POOL : ST_NHWC));
  P.release(t1a);
  Act t2a = P.cbr("backbone.conv2a", p1, nullptr, s16 ? ST_S16P : ST_NHWC);
  P.release(p1);
  Act t2b = P.cbr("backbone.conv2b", t2a, nullptr, s16 ? ST_S16P : (g.downsample >= 3 ? ST_NHWC_POOL : ST_NHWC));
  P.release(t2a);
  Act t3a = P.cbr("backbone.conv3a", t2b, nullptr, s16 ? ST_S16P : ST_NHWC);
  P.release(t2b);
  const bool only_enc = (flags & KP2D_FWD_ONLY_ENCODER) != 0;   // only_encoder(): skip every head but the VPR encoder
  // First CBR of every head in one launch ("heads.first", see describe()); first(name) hands out its channel slices.
  // Where a head's own launch would be a small grid (a frame or two per call) the five launches are five serial latencies
  // (0.42 -> 0.37 ms per frame).  On big grids the merged layer is ONE launch of the warp-specialised form with five times
  // the rounds (its start-up and drain paid once: conv family 333 -> 343 TFLOP/s at 64 x 240 x 320) against strided slice
  // reads in the five consumers: +0.1 ... +0.6 % at 64 frames, +1.4 % at 32, +0.9 % at 16, +0.6 % at 480 x 640, +0.9 % N
  // (profiles/r4_ab_merged_heads.txt); V3 (three parts), fp32 arithmetic and 30 x 40 head maps measured -0.2 ... -0.8 %
  // and keep their own launches.
  const int Hc = H >> g.downsample, Wc = W >> g.downsample;      // the cell grid (backbone output)
  const bool small_heads = small_grid(B, Hc, Wc, 1);
  // (round 5: 30 x 40 head maps too once the merged layer — five times the work items of one head's — runs on the
  // warp-specialised form: 64 frames of 120 x 160: five launches of 0.031 ms -> one of 0.102, +0.5 ... +2 % end to end)
  const int merged_groups = m->conv("heads.first") ? m->conv("heads.first")->npad / 64 : 0;
  const bool big_wsm = m->precision == KP2D_PREC_F16X3 && !v3 && m->wsm_min >= 0 &&
                       ((long)Hc * Wc >= 60 * 80 ||
                        ((long)Hc * Wc >= 30 * 40 && merged_groups >= 2 &&
                         wsm_would_run(B, Hc, Wc, merged_groups, cus, P.nlanes, m->wsm_min, m->wsm_grid, 2)));
  const bool merged = (small_heads || big_wsm) && !only_enc && m->conv("heads.first");
  // Big grids of the plain V2 S configuration: S16P is the layout of EVERY tensor a split-fp16 3x3 layer of the warp-specialised
  // form reads — conv3b's two outputs, conv4a / 4b, the merged first layer's desc / seg / vlad slices, both pixel-shuffled
  // tensors, convs.5, convlad2 — so those layers' staging waves only issue LDS-DMA copies (conv3x3_wsm.hip IN16).  fp32 NHWC
  // stays where another kernel reads: the score / location slices (exact dot products, head3x3.hip), convs.1's pooled output
  // and convs.2 / .3 (30 x 40 maps: general kernels), confAa's and convs.7's outputs (confBb / convs.8, planar outputs),
  // convlad3's (NetVLAD).  Same values bit for bit (a consumer multiplies the halves its own staging would have produced).
  // Decided once, on the form running for the smallest converted layer (conv4a); a tap keeps its layer readable either way.
  const int Hq = H / 4, Wq = W / 4;
  const bool s16_all = s16 && m->s16_all && !v3 && !only_enc && !g.use_attention && !g.depth &&
                       g.upscale_method != KP2D_UP_CONVTRANSPOSE && m->c5 == 64 && m->d1 == 128 && g.encoder_dim == 64 &&
                       m->wsm_min >= 0 && m->wsm_tr == 0 && merged &&
                       Wq / 2 >= 32 &&      // (convs.4 writes its pixel-shuffled S16P output from a W / 8 map: the form's least width
                       (long)((Wq / 2 + 31) / 32) * ((Hq / 2 + 15) / 16) * B * 2 >= 8 &&      //  and its least grid, eight work items)
                       wsm_would_run(B, Hq, Wq, 1, cus, P.nlanes, m->wsm_min, m->wsm_grid, 1);
  Act xp{};
  Act skip = P.cbr("backbone.conv3b", t3a, nullptr, s16_all ? ST_S16P_BOTH : ST_NHWC_BOTH, &xp);   // downsample >= 1 always
  P.release(t3a);
  Act t4a = P.cbr("backbone.conv4a", xp, nullptr, s16_all ? ST_S16P : ST_NHWC);
  P.release(xp);
  Act xb = P.cbr("backbone.conv4b", t4a, nullptr, s16_all ? ST_S16P : ST_NHWC);
  P.release(t4a);
  const int H2 = skip.H, W2 = skip.W;
  if (xb.H != Hc || xb.W != Wc) { P.rc = fail(KP2D_ERR_ARG, "plan: cell grid %dx%d, expected %dx%d", xb.H, xb.W, Hc, Wc); return; }

  // the two planar outputs behind a 64-channel S16P tensor (conv3x3_s16.hip's planar form: cout <= 32 plain logits)
  // (not the class logits when the forward also writes the dense class map: the argmax over channels that sit in 32 different
  // lanes — DPP rotations per pixel — made that layer 0.147 -> 0.189 ms; the general kernel finds it in its LDS tile)
  auto s16_planar = [&](int cout, bool with_ids = false) {
    return s16_all && !with_ids && cout <= 32 && m->c4 == 64 && m->c5 == 64 && !(W2 & 3);
  };
  // KP2D_FWD_NO_SEG_LOGITS: the caller reads the class ids this forward writes (kp2d_set_seg_ids) and never the logits.
  // Without the planar logits store the constraint above is gone: the last segmentation layer runs the TRANSPOSED products
  // of conv3x3_s16.hip, where a lane holds eight channels of ONE pixel, finds the argmax in registers and stores 8 bytes
  // per pixel instead of 4 n_classes (ST_IDS; 138 MB less per 64 frames of 240 x 320).  Same logits bit for bit, compared
  // in the same order, so the ids are those of the other path.  Everything else — V3 / softmax, a tap (one launch per
  // layer as planned without it), fp32 arithmetic, small grids, a layer the form does not take, KP2D_SEG_IDS_ONLY=0 (the
  // A/B switch and the way back) — keeps writing both.
  const ConvPack* seg_last = m->conv("seg_head.convs.8");
  const bool seg_ids_only = (flags & KP2D_FWD_NO_SEG_LOGITS) && tuning().seg_ids_only && P.seg_ids && o.seg && !m->tap_dst && s16_planar(g.n_classes) &&
                            g.n_classes >= 1 && seg_last && seg_last->npad == 32 && seg_last->cin == 64 && seg_last->cout == g.n_classes;
  Act mx{}, mxs{};
  int mx_split = 1 << 30;      // first channel of the merged layer kept in the S16P tensor mxs (s16_all: behind score | loc)
  if (merged && s16_all) {
    const ConvPack& cf = P.layer("heads.first");
    mx_split = cf.parts[0].second + cf.parts[1].second;
    mx = P.alloc(mx_split, Hc, Wc);
    mxs = P.alloc(cf.cout - mx_split, Hc, Wc);
    mxs.fmt = 1;
    P.conv("heads.first", xb, xb.C, 0, nullptr, lk, ST_MIX16, mx_split, Hc, Wc, P.out(mx), P.out(mxs));
  } else if (merged) {
    mx = P.cbr("heads.first", xb, nullptr, ST_NHWC);
  }
  auto first = [&](const std::string& name) -> Act {
    if (merged) {
      int o = 0;
      for (const auto& pt : P.layer("heads.first").parts) {
        if (pt.first == name) {
          Act v = o < mx_split ? Plan::view(mx, pt.second, o) : Plan::view(mxs, pt.second, o - mx_split);
          P.tap(name, v);
          return v;
        }
        o += pt.second;
      }
    }
    return P.cbr(name, xb, nullptr, ST_NHWC);
  };
  // NetVLAD / GeM / ConvAP / encoder map behind vlad_head.convlad3 (vpr.py:78-89, netvlad.py:79-106)
  // (keep: when the tail runs on the side stream its scratch must outlive the plan's next allocations — released by the caller)
  auto vlad_tail = [&](const Act& v3a, std::vector<Act>* keep = nullptr) {
    const int S = Hc * Wc, K = g.num_clusters, C = g.encoder_dim;
    if (only_enc || g.remove_netvlad) {
      // vpr.py:84-87: remove_netvlad (to_export) returns the encoder map itself whatever the pooler;
      // only_encoder=True returns l2(map).  Both leave as the NCHW map.
      if (!g.remove_netvlad) P.launch("vlad_head.l2", [&] { return launch_l2norm_channels(P.ptr(v3a), (long)B * S, C, P.stream); });
      P.launch("vlad_head (encoder map)", [&] { return launch_nhwc_to_nchw(P.ptr(v3a), o.vlad, B, C, S, C, 0, P.stream); });
    } else if (g.global_descriptor == KP2D_GD_GEM) {
      const VecPack& p = P.vec("vlad_head.netvlad.p");
      P.launch("vlad_head.netvlad", "gem", 4.0 * B * S * C, 4.0 * B * S * C, [&] {
        PoolArgs a{P.ptr(v3a), m->blob + p.off, o.vlad, B, C, Hc, Wc};
        return launch_gem(a, P.stream);
      });
    } else if (g.global_descriptor == KP2D_GD_CONVAP) {
      Act cp = P.pw("vlad_head.netvlad.channel_pool", v3a, ACT_NONE);
      P.launch("vlad_head.netvlad", "convap_pool", 1.0 * B * S * C, 4.0 * B * S * C, [&] {
        PoolArgs a{P.ptr(cp), nullptr, o.vlad, B, C, Hc, Wc};
        return launch_convap_pool(a, P.stream);
      });
      if (keep) keep->push_back(cp);
      else P.release(cp);
    } else {
      const int ns = netvlad_nsplit(S);
      const int tps = netvlad_tiles_per_slab(S, B);
      Act part = P.alloc_bytes((size_t)B * (ns * tps + (tps > 1 ? 1 : 0)) * ((size_t)K * C + K) * sizeof(float));   // tile mode: + the ordered sums
      const int prec = m->precision == KP2D_PREC_F16X3 ? 1 : 0;
      // the profile's kernel string spells the launch form (netvlad_form.h; tests/test_gpu_pooler_fp64.py reads it)
      char form[96] = "netvlad";      // (kept for a shape the launcher refuses; only a profiled forward reads the string)
      VladForm vf;
      if (m->profiling && choose_netvlad(K, C, prec, tuning().vlad_split, vf) == 0) netvlad_form_name(vf, ns, tps, form, sizeof form);
      P.launch("vlad_head.netvlad", form, 2.0 * 2 * K * C * (double)B * S, 4.0 * B * ((double)S * C + K * C), [&] {
        VladArgs a{};
        a.x = P.ptr(v3a); a.wa = m->blob + m->vlad_wa; a.cent = m->blob + m->vlad_cent;
        a.part = P.ptr(part); a.out = o.vlad; a.B = B; a.S = S; a.C = C; a.K = K; a.nsplit = ns; a.tps = tps;
        a.prec = prec;
        return launch_netvlad(a, P.stream);
      });
      if (keep) keep->push_back(part);
      else P.release(part);
    }
  };
  // Small grids, the plain V2 configuration (PixelShuffle upsampling, no attention, no depth head): the heads level by
  // level instead of head by head.  A frame's forward is a chain of dependent launches of ~8-10 us each whatever they compute;
  // the layers of different heads that wait for the same predecessor go out as ONE launch (Plan::group_begin / group_end),
  // so the heads cost the length of the longest chain (the segmentation head's eight layers), not the sum of all chains:
  // 17 launches -> 12 behind the merged first layer.  Same kernels, same arithmetic, per layer.
  // (a dry run sizes the workspace for whichever schedule keeps more tensors alive — P.no_levels picks; profiles and taps
  // take the layers one launch at a time)
  const bool levels = merged && small_heads && !v3 && !g.use_attention && !g.depth && g.upscale_method != KP2D_UP_CONVTRANSPOSE &&
                      m->precision == KP2D_PREC_F16X3 && m->multi_launch && !P.no_levels && !s16_all &&
                      (P.dry || (!m->profiling && !m->tap_dst));
  if (levels) {
    const std::string L = "seg_head.convs.";
    Act s1 = first("score_head.convDa"), l1 = first("loc_head.convDa"), d1 = first("desc_head.convA");
    Act g0 = first(L + "0"), v1 = first("vlad_head.convlad1");
    P.head_pair("score_head.convDb", s1, ACT_SIGMOID, o.score, "loc_head.convDb", l1, ACT_TANH, o.shift, Hc, Wc);
    const ConvPack& cB = P.layer("desc_head.convB");
    // level 1
    Act d2 = P.alloc(cB.cout / 4, H2, W2);
    P.group_begin();
    P.conv("desc_head.convB", d1, d1.C, 0, nullptr, ACT_NONE, ST_SHUFFLE, 0, Hc, Wc, P.out(d2));
    Act g1 = P.cbr(L + "1", g0, nullptr, ST_NHWC_POOL);
    Act v2 = P.cbr("vlad_head.convlad2", v1, nullptr, ST_NHWC);
    P.group_end();
    // level 2
    P.group_begin();
    Act d3 = P.cbr("desc_head.confAa", d2, &skip, ST_NHWC);
    Act g2 = P.cbr(L + "2", g1, nullptr, ST_NHWC);
    Act v3a = P.cbr("vlad_head.convlad3", v2, nullptr, ST_NHWC);
    P.group_end();
    P.release(d2);
    P.release(g1);
    P.release(v2);
    // The VPR head is done with its convolutions two launches before the descriptor head and six before the segmentation
    // head: its pooling (NetVLAD: three launches, ~25 us of a frame's ~230) goes to a side stream and runs BESIDE the rest
    // (fork / join by events).  Its input and scratch stay allocated until the join (the dry run sizes the workspace the
    // same way).
    // Not under stream capture: replayed as graphs with several frames in flight (pipeline.FrameStream) the extra branch
    // costs the overlap BETWEEN frames — 10.3k -> 4.6k frames/s (profiles/r5_ab_side_stream.txt); a plain forward gains 5 %.
    std::vector<Act> vlad_keep;
    // The stream is created on first use, not with the model: HIP spreads a process's streams over four hardware queues,
    // and a stream that exists — used or not — took one from pipeline.BatchStream's two (64-frame batches, two steps in
    // flight: 25.0k -> 23.6k frames/s with an idle side stream in the process, back at 24.9k with GPU_MAX_HW_QUEUES=8).
    bool side = m->side_overlap && P.live();
    if (side) {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(P.stream, &cs) != hipSuccess) { (void)hipGetLastError(); side = false; }
      else if (cs != hipStreamCaptureStatusNone) side = false;
    }
    if (side && !m->side_stream) {
      if (hipStreamCreateWithFlags(&m->side_stream, hipStreamNonBlocking) != hipSuccess ||
          hipEventCreateWithFlags(&m->side_fork, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&m->side_join, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (m->side_stream) (void)hipStreamDestroy(m->side_stream);
        m->side_stream = nullptr;
        m->side_overlap = false;
        side = false;
      }
    }
    hipStream_t main_stream = P.stream;
    if (side) {
      P.check((int)hipEventRecord(m->side_fork, main_stream), "side stream fork");
      P.check((int)hipStreamWaitEvent(m->side_stream, m->side_fork, 0), "side stream fork");
      P.stream = m->side_stream;
    }
    vlad_tail(v3a, &vlad_keep);
    if (side) {
      P.check((int)hipEventRecord(m->side_join, m->side_stream), "side stream join");
      P.stream = main_stream;
    }
    // level 3
    P.group_begin();
    P.conv("desc_head.confBb", d3, d3.C, 0, nullptr, ACT_NONE, ST_NCHW, g.nfeatures, H2, W2, {o.feat});
    Act g3 = P.cbr(L + "3", g2, nullptr, ST_NHWC);
    P.group_end();
    P.release(d3);
    P.release(g2);
    // the rest of the segmentation head is the critical path: one layer per launch
    Act g4 = P.cbr(L + "4", g3, nullptr, ST_SHUFFLE);
    P.release(g3);
    Act g5 = P.cbr(L + "5", g4, &xb, ST_NHWC);
    P.release(g4);
    Act g6 = P.cbr(L + "6", g5, nullptr, ST_SHUFFLE);
    P.release(g5);
    Act g7 = P.cbr(L + "7", g6, &skip, ST_NHWC);
    P.release(g6);
    P.conv(L + "8", g7, g7.C, 0, nullptr, ACT_NONE, ST_NCHW, g.n_classes, H2, W2, {o.seg});
    P.release(g7);
    if (side) P.check((int)hipStreamWaitEvent(main_stream, m->side_join, 0), "side stream join");
    for (const Act& k : vlad_keep) P.release(k);
    P.release(v3a);
    P.release(mx);
    P.release(xb);
    P.release(skip);
    return;
  }
  // ---- score / location heads (heads.py:28-35; sigmoid/tanh kp2dtiny.py:574-575, :927-935) ----
  if (only_enc) {
  } else if (v3) {
    Act s1 = first("score_loc_head.convDa");
    P.conv("score_loc_head.convDb", s1, s1.C, 0, nullptr, ACT_SIGMOID0_TANH, ST_NCHW, 1, Hc, Wc, {o.score}, {o.shift});
    P.release(s1);
  } else {
    Act s1 = first("score_head.convDa");
    Act l1 = first("loc_head.convDa");
    P.head_pair("score_head.convDb", s1, ACT_SIGMOID, o.score, "loc_head.convDb", l1, ACT_TANH, o.shift, Hc, Wc);
    P.release(s1);
    P.release(l1);
    // ---- descriptor head (heads.py:91-104) ----
    Act d1 = first("desc_head.convA");
    const ConvPack& cB = P.layer("desc_head.convB");
    Act d2 = P.alloc(cB.cout / 4, H2, W2);
    if (g.upscale_method == KP2D_UP_CONVTRANSPOSE) {
      // convB at the cell grid, then the transposed-conv upsampler as a pixel-shuffled 3x3 conv (heads.py:96-98)
      Act db = P.alloc(cB.cout, Hc, Wc);
      P.conv("desc_head.convB", d1, d1.C, 0, nullptr, ACT_NONE, ST_NHWC, 0, Hc, Wc, P.out(db));
      P.conv("desc_head.upsample", db, db.C, 0, nullptr, lk, ST_SHUFFLE, 0, Hc, Wc, P.out(d2));
      P.release(db);
    } else {
      if (s16_all) d2.fmt = 1;
      P.conv("desc_head.convB", d1, d1.C, 0, nullptr, ACT_NONE, s16_all ? ST_S16P_SHUFFLE : ST_SHUFFLE, 0, Hc, Wc, P.out(d2));
    }
    P.release(d1);
    P.tap("desc_head.convB", d2);     // the pixel-shuffled / transposed-conv upsampled tensor (heads.py:96-98)
    Act d3 = P.cbr("desc_head.confAa", d2, &skip, s16_planar(g.nfeatures) ? ST_S16P : ST_NHWC);
    P.release(d2);
    P.conv("desc_head.confBb", d3, d3.C, 0, nullptr, ACT_NONE, ST_NCHW, g.nfeatures, H2, W2, {o.feat});
    P.release(d3);
  }

  // ---- segmentation head: segmentation.py:126-157 (V2), :321-347 (V3), :442-466 (V2 att), :588-619 (V3 att) ----
  // trunk(prefix) runs everything up to the last CBR(c_exp -> width) and returns it plus the name of the final conv
  // CBR(ch -> d1) + 2x upsampling: PixelShuffle folded into the store, or (to_mcu) the CBR at its own resolution
  // followed by TransposedConvUpsampleModel as a second, pixel-shuffled conv (segmentation.py:139-147)
  auto upconv = [&](const std::string& cname, const std::string& uname, const Act& in) -> Act {
    if (g.upscale_method != KP2D_UP_CONVTRANSPOSE) return P.cbr(cname, in, nullptr, s16_all ? ST_S16P_SHUFFLE : ST_SHUFFLE);
    Act t = P.cbr(cname, in, nullptr, ST_NHWC);
    Act u = P.cbr(uname, t, nullptr, ST_SHUFFLE);
    P.release(t);
    return u;
  };
  auto trunk = [&](const std::string& hp, std::string* last) -> Act {
    const std::string L = hp + ".convs.";
    Act g5{};
    int i;   // index of the second-to-last shuffle CBR
    if (g.use_attention) {
      Act g0 = P.cbr(L + "0", xb, nullptr, ST_NHWC);
      Act a1 = P.attention_module(L + "1", g0, /*pool=*/true);
      P.release(g0);
      Act a2 = P.attention_module(L + "2", a1, false);
      P.release(a1);
      Act g4 = upconv(L + "3", hp + ".upsample", a2);
      P.release(a2);
      g5 = P.cbr(L + "4", g4, &xb, ST_NHWC);
      P.release(g4);
      i = 5;
    } else {
      Act g0 = first(L + "0");
      Act g1 = P.cbr(L + "1", g0, nullptr, ST_NHWC_POOL);
      P.release(g0);
      Act g2 = P.cbr(L + "2", g1, nullptr, ST_NHWC);
      P.release(g1);
      Act g3 = P.cbr(L + "3", g2, nullptr, ST_NHWC);
      P.release(g2);
      Act g4 = upconv(L + "4", hp + ".upsample", g3);
      P.release(g3);
      g5 = P.cbr(L + "5", g4, &xb, s16_all ? ST_S16P : ST_NHWC);
      P.release(g4);
      i = 6;
    }
    Act g6 = upconv(L + std::to_string(i), hp + ".upsample2", g5);
    P.release(g5);
    Act g7 = P.cbr(L + std::to_string(i + 1), g6, &skip, (hp == "seg_head" && (seg_ids_only || s16_planar(g.n_classes, P.seg_ids != nullptr))) ? ST_S16P : ST_NHWC);
    P.release(g6);
    *last = L + std::to_string(i + 2);
    return g7;
  };
  if (!only_enc) {
    std::string last;
    Act g7 = trunk("seg_head", &last);
    if (v3) {
      const int half = m->c5 / 2;   // dim_split = c_hidden // 2 (segmentation.py:190, :339-343)
      P.conv("seg_head.featB", g7, half, 0, nullptr, ACT_NONE, ST_NCHW, g.nfeatures, H2, W2, {o.feat});
      if (g.depth)   // depth = featD(seg[:, half:2*half]).sigmoid()  (segmentation.py:340-341, kp2dtiny.py:956)
        P.conv("seg_head.featD", g7, half, half, nullptr, ACT_SIGMOID, ST_NCHW, 1, H2, W2, {o.depth});
      const bool sm = (flags & KP2D_FWD_EVAL) && !g.remove_softmax;
      P.conv(last, g7, half, g7.C - half, nullptr, sm ? ACT_SOFTMAX_C : ACT_NONE, ST_NCHW, g.n_classes, H2, W2, {o.seg});
    } else {
      P.conv(last, g7, g7.C, 0, nullptr, ACT_NONE, (seg_ids_only && last == "seg_head.convs.8") ? ST_IDS : ST_NCHW, g.n_classes, H2, W2, {o.seg});
    }
    P.release(g7);
  }
  if (!only_enc && !v3 && g.depth) {   // depth = depth_head(x, skip).sigmoid()  (kp2dtiny.py:588-590)
    std::string last;
    Act g7 = trunk("depth_head", &last);
    P.conv(last, g7, g7.C, 0, nullptr, ACT_SIGMOID, ST_NCHW, 1, H2, W2, {o.depth});
    P.release(g7);
  }

  // ---- VPR head (vpr.py:78-89) + NetVLAD (netvlad.py:79-106) ----
  {
    Act v1 = first("vlad_head.convlad1");
    Act v2 = P.cbr("vlad_head.convlad2", v1, nullptr, s16_all ? ST_S16P : ST_NHWC);
    P.release(v1);
    Act v3a = P.cbr("vlad_head.convlad3", v2, nullptr, ST_NHWC);
    P.release(v2);
    vlad_tail(v3a);
    P.release(v3a);
  }
  if (merged) P.release(mx);
  if (merged) P.release(mxs);
  P.release(xb);
  P.release(skip);
}

int validate_shape(const kp2d_model* m, int B, int H, int W) {
  if (B < 1) return fail(KP2D_ERR_ARG, "B must be >= 1");
  // the segmentation head pools the cell grid once more (segmentation.py:134): H, W divisible by 2 * cell
  const int q = 2 << m->cfg.downsample;
  if (H < 16 || W < 16 || (H % q) || (W % q)) return fail(KP2D_ERR_ARG, "H and W must be multiples of %d and >= 16 (got %dx%d)", q, H, W);
  return KP2D_OK;
}

namespace {
size_t plan_bytes(kp2d_model* m, int Bc, int H, int W, int lanes);
}

// Frames per internal sub-batch.  Measured on MI355X (profiles/r1_*): the path is compute-bound, so bigger
// launches win (64 frames at once: 5.4k frames/s vs 3.7k with 10-frame sub-batches that keep intermediates
// inside the Infinity Cache but leave the 30x40 layers with 60 workgroups for 256 CUs).  The automatic
// choice therefore only caps the workspace (4 GiB), it does not chase cache residency.
int auto_chunk(const kp2d_model* m, int B, int H, int W) {
  if (m->chunk_frames > 0) return std::min(B, m->chunk_frames);
  const size_t per_frame = plan_bytes(const_cast<kp2d_model*>(m), 1, H, W, 1);
  if (per_frame == 0) return 1;
  const size_t cap = (size_t)4 << 30;
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)B, cap / per_frame));
}

namespace {

size_t plan_bytes_uncached(kp2d_model* m, int Bc, int H, int W, int lanes);

// dry-run planning costs ~0.1 ms of host time; the result only depends on (frames, H, W, lanes) — the lane count sizes the
// persistent forms' grids, which fix activation layouts (conv_policy.h) — so it is memoised
size_t plan_bytes(kp2d_model* m, int Bc, int H, int W, int lanes) {
  const uint64_t key = ((uint64_t)lanes << 60) ^ ((uint64_t)Bc << 40) ^ ((uint64_t)H << 20) ^ (uint64_t)W;
  auto it = m->plan_cache.find(key);
  if (it != m->plan_cache.end()) return it->second;
  const size_t v = plan_bytes_uncached(m, Bc, H, W, lanes);
  m->plan_cache[key] = v;
  return v;
}

size_t plan_bytes_uncached(kp2d_model* m, int Bc, int H, int W, int lanes) {
  Plan P{};
  P.m = m; P.stream = nullptr; P.ws = nullptr; P.dry = true; P.B = Bc; P.H = H; P.W = W; P.nlanes = lanes;
  P.arena.reset((size_t)1 << 46);
  FwdOut o{};
  build(P, o, 0);
  if (P.rc != KP2D_OK) return 0;
  // the level-by-level schedule of small grids and the head-by-head one keep different tensors alive: room for either
  Plan Q{};
  Q.m = m; Q.stream = nullptr; Q.ws = nullptr; Q.dry = true; Q.B = Bc; Q.H = H; Q.W = W; Q.nlanes = lanes; Q.no_levels = true;
  Q.arena.reset((size_t)1 << 46);
  build(Q, o, 0);
  return Q.rc == KP2D_OK ? std::max(P.arena.high, Q.arena.high) : 0;
}

}  // namespace

size_t schedule(kp2d_model* m, int B, int H, int W, int* lanes, int* chunk) {
  int nl = m->profiling ? 1 : std::max(1, m->lanes);
  nl = std::min(nl, B);
  int c = std::max(1, std::min(auto_chunk(m, B, H, W), (B + nl - 1) / nl));
  *lanes = nl;
  *chunk = c;
  return align_up(plan_bytes(m, c, H, W, std::min(nl, (B + c - 1) / c)));
}

}  // namespace plan
}  // namespace kp2d
