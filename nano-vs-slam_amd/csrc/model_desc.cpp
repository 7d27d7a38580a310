// Model description (which tensors a configuration has, under the reference's state_dict names and shapes) and weight
// packing (BatchNorm folding, the kernels' weight layouts).  Pure host code, no HIP: hipcc compiles it into the library,
// g++ into the driver of tests/test_model_desc.py.
#include "model_desc.h"

#include <algorithm>
#include <cmath>

#include "api_common.h"
#include "f16_host.h"

namespace kp2d {

namespace {

// ------------------------------------------------------------------------------------------------
// model description (state-dict layout: SURVEY.md App. C; constructors kp2dtiny.py:347-449 / :732-803)
// ------------------------------------------------------------------------------------------------
void add_spec(ModelDesc* m, const std::string& key, std::vector<int64_t> shape) {
  m->spec_index[key] = (int)m->specs.size();
  m->specs.push_back(WeightSpec{key, std::move(shape)});
}

void add_cbr(ModelDesc* m, const std::string& p, int ci, int co, bool shuffle = false) {
  add_spec(m, p + ".conv.weight", {co, ci, 3, 3});
  add_spec(m, p + ".bn.weight", {co});
  add_spec(m, p + ".bn.bias", {co});
  add_spec(m, p + ".bn.running_mean", {co});
  add_spec(m, p + ".bn.running_var", {co});
  ConvPack c;
  c.name = p; c.bn = true; c.shuffle = shuffle; c.cin = ci; c.cout = co;
  m->conv_index[p] = (int)m->convs.size();
  m->convs.push_back(c);
}

void add_conv(ModelDesc* m, const std::string& p, int ci, int co, bool shuffle = false) {
  add_spec(m, p + ".weight", {co, ci, 3, 3});
  add_spec(m, p + ".bias", {co});
  ConvPack c;
  c.name = p; c.bn = false; c.shuffle = shuffle; c.cin = ci; c.cout = co;
  m->conv_index[p] = (int)m->convs.size();
  m->convs.push_back(c);
}

// TransposedConvUpsampleModel(c) (base.py:80-117): ConvTranspose2d(c, c/4, k3, s2, p1, output_padding 1, no bias)
// -> BatchNorm2d(c/4) -> (Leaky)ReLU.  Output pixel (2y+a, 2x+b) only sees inputs (y..y+1, x..x+1):
//   a = 0: in[y] * w[ky=1];   a = 1: in[y] * w[ky=2] + in[y+1] * w[ky=0]      (same along x)
// so it IS a 3x3 convolution c -> 4*(c/4) with the dy = -1 / dx = -1 taps zero, followed by PixelShuffle(2)
// (virtual channel 4*co + 2a + b), and runs through the pixel-shuffle store of the conv kernel unchanged.
void add_tconv(ModelDesc* m, const std::string& p, int c) {
  add_spec(m, p + ".transposed_conv.weight", {c, c / 4, 3, 3});
  add_spec(m, p + ".bn.weight", {c / 4});
  add_spec(m, p + ".bn.bias", {c / 4});
  add_spec(m, p + ".bn.running_mean", {c / 4});
  add_spec(m, p + ".bn.running_var", {c / 4});
  ConvPack k;
  k.name = p; k.bn = true; k.shuffle = true; k.tconv = true; k.cin = c; k.cout = c;
  m->conv_index[p] = (int)m->convs.size();
  m->convs.push_back(k);
}

// 1x1 conv (kind 1) or 2x2 stride-2 conv (kind 2) routed through the MFMA conv kernel with taps = 1
void add_pw(ModelDesc* m, const std::string& p, int ci, int co, bool bias, int kind) {
  const int k = kind == 2 ? 2 : 1;
  add_spec(m, p + ".weight", {co, ci, k, k});
  if (bias) add_spec(m, p + ".bias", {co});
  ConvPack c;
  c.name = p; c.bn = false; c.bias = bias; c.kind = kind; c.taps = 1;
  c.cin = kind == 2 ? 4 * ci : ci; c.cout = co;
  m->conv_index[p] = (int)m->convs.size();
  m->convs.push_back(c);
}

// SegFormerAttentionModule(c) (modules/segformer.py:209-220); PreNorm registers fn before norm
void add_attention_module(ModelDesc* m, const std::string& p, int c) {
  add_pw(m, p + ".att.fn.to_q", c, c, false, 1);
  add_pw(m, p + ".att.fn.to_kv", c, 2 * c, false, 2);
  add_pw(m, p + ".att.fn.to_out", c, c, false, 1);
  add_spec(m, p + ".att.norm.g", {1, c, 1, 1});
  add_spec(m, p + ".att.norm.b", {1, c, 1, 1});
  const int h = 2 * c;
  add_pw(m, p + ".mff.fn.net.0", c, h, true, 1);
  add_spec(m, p + ".mff.fn.net.1.net.0.weight", {h, 1, 3, 3});
  add_spec(m, p + ".mff.fn.net.1.net.0.bias", {h});
  add_pw(m, p + ".mff.fn.net.1.net.1", h, h, true, 1);
  add_pw(m, p + ".mff.fn.net.3", h, c, true, 1);
  add_spec(m, p + ".mff.norm.g", {1, c, 1, 1});
  add_spec(m, p + ".mff.norm.b", {1, c, 1, 1});
  m->vecs[p + ".att.norm.g"].n = c;
  m->vecs[p + ".att.norm.b"].n = c;
  m->vecs[p + ".mff.norm.g"].n = c;
  m->vecs[p + ".mff.norm.b"].n = c;
  m->vecs[p + ".mff.fn.net.1.net.0.weight"].n = 9 * h;   // repacked [9][h]
  m->vecs[p + ".mff.fn.net.1.net.0.bias"].n = h;
}

}  // namespace

int describe(ModelDesc* m) {
  const kp2d_config& g = m->cfg;
  const int c1 = m->c1 = g.channel_dims[0], c2 = m->c2 = g.channel_dims[1], c3 = m->c3 = g.channel_dims[2];
  const int c4 = m->c4 = g.channel_dims[3], c5 = m->c5 = g.channel_dims[4], d1 = m->d1 = g.channel_dims[5];
  const bool v3 = g.version == 3;
  // backbone (encoders.py:20-99).  conv1a is packed separately (Cin = 3, or 1 for use_color=False).
  add_spec(m, "backbone.conv1a.conv.weight", {c1, g.in_channels, 3, 3});
  add_spec(m, "backbone.conv1a.bn.weight", {c1});
  add_spec(m, "backbone.conv1a.bn.bias", {c1});
  add_spec(m, "backbone.conv1a.bn.running_mean", {c1});
  add_spec(m, "backbone.conv1a.bn.running_var", {c1});
  add_cbr(m, "backbone.conv1b", c1, c2);
  add_cbr(m, "backbone.conv2a", c2, c2);
  add_cbr(m, "backbone.conv2b", c2, c3);
  add_cbr(m, "backbone.conv3a", c3, c3);
  add_cbr(m, "backbone.conv3b", c3, c4);
  add_cbr(m, "backbone.conv4a", c4, c4);
  add_cbr(m, "backbone.conv4b", c4, c4);
  if (v3) {
    add_cbr(m, "score_loc_head.convDa", c4, c4);
    add_conv(m, "score_loc_head.convDb", c4, 3);
  } else {
    add_cbr(m, "score_head.convDa", c4, c4);
    add_conv(m, "score_head.convDb", c4, 1);
    add_cbr(m, "loc_head.convDa", c4, c4);
    add_conv(m, "loc_head.convDb", c4, 2);
    const bool tc0 = g.upscale_method == KP2D_UP_CONVTRANSPOSE;
    if (tc0) add_tconv(m, "desc_head.upsample", c3 * 4);   // registered first (heads.py:55-56)
    add_cbr(m, "desc_head.convA", c4, c4);
    add_conv(m, "desc_head.convB", c4, c3 * 4, /*shuffle=*/!tc0);
    add_cbr(m, "desc_head.confAa", c3 + c4, c4);
    add_conv(m, "desc_head.confBb", c4, g.nfeatures);
  }
  const int ch = c5, cexp = c4 + c3;
  const int last_in = v3 ? ch / 2 : ch;
  // V3 depth: the last CBR is half a width wider and a third 3x3 conv (featD, no bias) reads the middle slice
  const int trunk_out = (v3 && g.depth) ? ch + ch / 2 : ch;
  if (g.use_attention && (ch > 256 || (ch % 16)))
    return fail(KP2D_ERR_UNSUPPORTED, "attention width %d (built for <= 256, multiple of 16)", ch);
  const bool tc = g.upscale_method == KP2D_UP_CONVTRANSPOSE;
  if (tc && (d1 % 16)) return fail(KP2D_ERR_UNSUPPORTED, "convtranspose upsampling needs channel_dims[5] %% 16 == 0");
  auto seg_like_head = [&](const std::string& P_, int c_out, int width) {
    const std::string L = P_ + ".convs.";
    if (g.use_attention) {
      add_cbr(m, L + "0", c4, ch);
      add_attention_module(m, L + "1", ch);
      add_attention_module(m, L + "2", ch);
      add_cbr(m, L + "3", ch, d1, !tc);
      add_cbr(m, L + "4", ch + d1 / 4, ch);
      add_cbr(m, L + "5", ch, d1, !tc);
      add_cbr(m, L + "6", cexp, width);
      add_conv(m, L + "7", P_ == "seg_head" ? last_in : ch, c_out);
    } else {
      add_cbr(m, L + "0", c4, ch);
      add_cbr(m, L + "1", ch, ch);
      add_cbr(m, L + "2", ch, ch);
      add_cbr(m, L + "3", ch, ch);
      add_cbr(m, L + "4", ch, d1, !tc);
      add_cbr(m, L + "5", ch + d1 / 4, ch);
      add_cbr(m, L + "6", ch, d1, !tc);
      add_cbr(m, L + "7", cexp, width);
      add_conv(m, L + "8", P_ == "seg_head" ? last_in : ch, c_out);
    }
  };
  auto upsamplers = [&](const std::string& P_) {   // registered after convs / featB / featD (segmentation.py:113-118)
    if (tc) { add_tconv(m, P_ + ".upsample", d1); add_tconv(m, P_ + ".upsample2", d1); }
  };
  seg_like_head("seg_head", g.n_classes, trunk_out);
  if (!v3) upsamplers("seg_head");
  if (v3) {
    add_conv(m, "seg_head.featB", ch / 2, g.nfeatures);
    if (g.depth) {   // Conv2d(dim_split, 1, bias=False): segmentation.py:281-284
      add_spec(m, "seg_head.featD.weight", {1, ch / 2, 3, 3});
      ConvPack c;
      c.name = "seg_head.featD"; c.bn = false; c.bias = false; c.cin = ch / 2; c.cout = 1;
      m->conv_index[c.name] = (int)m->convs.size();
      m->convs.push_back(c);
    }
    upsamplers("seg_head");
  } else if (g.depth) {
    seg_like_head("depth_head", 1, ch);   // kp2dtiny.py:402-437: a second full segmentation head with one output
    upsamplers("depth_head");
  }
  add_cbr(m, "vlad_head.convlad1", c4, g.encoder_dim);
  add_cbr(m, "vlad_head.convlad2", g.encoder_dim, g.encoder_dim);
  add_cbr(m, "vlad_head.convlad3", g.encoder_dim, g.encoder_dim);
  {
    // The first CBR of every head reads the same backbone map: one launch computes them all (rows of the parts
    // back to back), the heads then read channel slices of its output.  The attention seg heads keep their own
    // launch (their first CBR feeds a LayerNorm, which wants a dense tensor).
    ConvPack mg;
    mg.name = "heads.first"; mg.bn = true; mg.cin = c4;
    auto part = [&](const std::string& n) { mg.parts.emplace_back(n, m->conv(n)->cout); mg.cout += mg.parts.back().second; };
    if (v3) part("score_loc_head.convDa");
    else { part("score_head.convDa"); part("loc_head.convDa"); part("desc_head.convA"); }
    if (!g.use_attention && m->conv_index.count("seg_head.convs.0")) part("seg_head.convs.0");
    part("vlad_head.convlad1");
    if (mg.parts.size() >= 2) { m->conv_index[mg.name] = (int)m->convs.size(); m->convs.push_back(mg); }
  }
  const bool has_vlad = g.global_descriptor == KP2D_GD_NETVLAD && !g.remove_netvlad;
  if (has_vlad) {
    add_spec(m, "vlad_head.netvlad.centroids", {g.num_clusters, g.encoder_dim});
    add_spec(m, "vlad_head.netvlad.conv.weight", {g.num_clusters, g.encoder_dim, 1, 1});
  } else if (g.global_descriptor == KP2D_GD_GEM) {
    add_spec(m, "vlad_head.netvlad.p", {1});
    m->vecs["vlad_head.netvlad.p"].n = 1;
  } else if (g.global_descriptor == KP2D_GD_CONVAP) {
    add_pw(m, "vlad_head.netvlad.channel_pool", g.encoder_dim, g.encoder_dim, true, 1);
  }

  // blob layout
  size_t off = 0;
  auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats, ALIGN / 4); return o; };
  m->conv1a_w = take((size_t)9 * g.in_channels * c1);
  m->conv1a_sc = take(c1);
  m->conv1a_sh = take(c1);
  m->conv1a_ws = take(1);
  for (auto& c : m->convs) {
    if (c.cin % 4) return fail(KP2D_ERR_UNSUPPORTED, "%s: input channels %d not a multiple of 4", c.name.c_str(), c.cin);
    if (c.shuffle && (c.cout % 16)) return fail(KP2D_ERR_UNSUPPORTED, "%s: pixel-shuffle conv needs cout %% 16 == 0", c.name.c_str());
    c.kc = (c.cin % 16 == 0) ? 16 : ((c.cin % 8 == 0) ? 8 : 16);
    c.npad = c.cout <= 32 ? 32 : (c.cout + 63) / 64 * 64;
    c.w_off = take(c.w_floats());
    c.sc_off = take(c.npad);
    c.sh_off = take(c.npad);
    c.w16_off = take(c.w16_floats());
    if (c.npad >= 64) c.w16n_off = take(c.w16_floats());
    if (c.npad >= 64 && c.kind == 0 && c.taps == 9) c.w16t_off = take(c.w16_floats());
    c.sc16_off = take(c.npad);
    if (c.head()) c.wd_off = take(c.wd_floats());
  }
  for (auto& kv : m->vecs) kv.second.off = take(kv.second.n);
  if (has_vlad) {
    m->vlad_wa = take((size_t)g.num_clusters * g.encoder_dim);
    m->vlad_cent = take((size_t)g.num_clusters * g.encoder_dim);
  }
  m->blob_floats = off;
  return KP2D_OK;
}

namespace {

const std::vector<float>* host_get(const ModelDesc* m, const std::string& key) {
  auto it = m->host.find(key);
  return it == m->host.end() ? nullptr : &it->second;
}

// BatchNorm2d eval: y = (x - mean) / sqrt(var + 1e-5) * gamma + beta  ->  y = x * scale + shift
void bn_fold(const ModelDesc* m, const std::string& p, int co, float* scale, float* shift) {
  const auto& g = *host_get(m, p + ".weight");
  const auto& b = *host_get(m, p + ".bias");
  const auto& mu = *host_get(m, p + ".running_mean");
  const auto& var = *host_get(m, p + ".running_var");
  for (int c = 0; c < co; ++c) {
    const float s = g[c] / std::sqrt(var[c] + 1e-5f);
    scale[c] = s;
    shift[c] = b[c] - mu[c] * s;
  }
}

}  // namespace

int pack(const ModelDesc* m, std::vector<float>& blob) {
  for (const auto& s : m->specs)
    if (!host_get(m, s.key)) return fail(KP2D_ERR_WEIGHT, "missing tensor '%s'", s.key.c_str());
  blob.assign(m->blob_floats, 0.f);
  const int c1 = m->c1;
  {
    const auto& w = *host_get(m, "backbone.conv1a.conv.weight");   // [c1][cin][3][3]
    const int nk = 9 * m->cfg.in_channels;
    for (int co = 0; co < c1; ++co)
      for (int k = 0; k < nk; ++k) blob[m->conv1a_w + (size_t)k * c1 + co] = w[(size_t)co * nk + k];
    bn_fold(m, "backbone.conv1a.bn", c1, &blob[m->conv1a_sc], &blob[m->conv1a_sh]);
    // the fused first layer splits these weights as w 2^e (conv3x3_f16.hip STEM): e as for every other layer
    float wmax = 0.f;
    for (float v : w) wmax = std::max(wmax, std::fabs(v));
    int e16 = 11;
    while (e16 > -96 && wmax * std::ldexp(1.0f, e16) > 32768.0f) --e16;
    blob[m->conv1a_ws] = std::ldexp(1.0f, e16);
  }
  for (const auto& c : m->convs) {
    std::vector<float> wvirt;
    if (c.tconv) {
      // virtual 3x3 weight [4*co + 2a + b][ci][ty][tx] of the transposed convolution (see add_tconv)
      const auto& wt = *host_get(m, c.name + ".transposed_conv.weight");   // [ci][co][ky][kx]
      const int cq4 = c.cout / 4;
      wvirt.assign((size_t)c.cout * c.cin * 9, 0.f);
      auto kmap = [](int par, int t) { return par == 0 ? (t == 1 ? 1 : -1) : (t == 1 ? 2 : (t == 2 ? 0 : -1)); };
      for (int co = 0; co < cq4; ++co)
        for (int a = 0; a < 2; ++a)
          for (int b = 0; b < 2; ++b)
            for (int ci = 0; ci < c.cin; ++ci)
              for (int ty = 0; ty < 3; ++ty)
                for (int tx = 0; tx < 3; ++tx) {
                  const int ky = kmap(a, ty), kx = kmap(b, tx);
                  if (ky < 0 || kx < 0) continue;
                  wvirt[((size_t)(4 * co + 2 * a + b) * c.cin + ci) * 9 + ty * 3 + tx] =
                      wt[(((size_t)ci * cq4 + co) * 3 + ky) * 3 + kx];
                }
    }
    std::vector<float> sc(c.cout), sh(c.cout);
    if (!c.parts.empty()) {   // rows of the parts, back to back
      wvirt.reserve((size_t)c.cout * c.cin * 9);
      int row = 0;
      for (const auto& pt : c.parts) {
        const auto& wp = *host_get(m, pt.first + ".conv.weight");
        wvirt.insert(wvirt.end(), wp.begin(), wp.end());
        bn_fold(m, pt.first + ".bn", pt.second, sc.data() + row, sh.data() + row);
        row += pt.second;
      }
    }
    const auto& w = (c.tconv || !c.parts.empty()) ? wvirt : *host_get(m, c.name + (c.bn ? ".conv.weight" : ".weight"));   // [cout][ci][k][k]
    if (!c.parts.empty()) {
    } else if (c.tconv) {
      std::vector<float> s4(c.cout / 4), h4(c.cout / 4);
      bn_fold(m, c.name + ".bn", c.cout / 4, s4.data(), h4.data());
      for (int i = 0; i < c.cout; ++i) { sc[i] = s4[i / 4]; sh[i] = h4[i / 4]; }
    } else if (c.bn) {
      bn_fold(m, c.name + ".bn", c.cout, sc.data(), sh.data());
    } else {
      const std::vector<float>* b = c.bias ? host_get(m, c.name + ".bias") : nullptr;
      for (int i = 0; i < c.cout; ++i) { sc[i] = 1.f; sh[i] = b ? (*b)[i] : 0.f; }
    }
    const int ng = c.npad <= 32 ? 32 : 64;          // channels per workgroup group
    const int ngroups = c.npad / ng;
    const int nchunk = (c.cin + c.kc - 1) / c.kc;
    const int cq = c.cout / 4;
    for (int q = 0; q < c.npad; ++q) {
      // packed position q -> original output channel (PixelShuffle: out[c,2h+i,2w+j] = in[4c+2i+j,h,w])
      int co = -1;
      if (q < c.cout) co = c.shuffle ? 4 * (q % cq) + (q / cq) : q;
      blob[c.sc_off + q] = co >= 0 ? sc[co] : 0.f;
      blob[c.sh_off + q] = co >= 0 ? sh[co] : 0.f;
      if (co < 0) continue;
      const int grp = q / ng, n = q % ng;
      for (int ci = 0; ci < c.cin; ++ci) {
        const int chk = ci / c.kc, kk = ci % c.kc;
        if (c.kind == 0) {
          for (int tap = 0; tap < 9; ++tap) {
            const size_t dst = c.w_off + ((((size_t)grp * nchunk + chk) * 9 + tap) * ng + n) * c.kc + kk;
            blob[dst] = w[((size_t)co * c.cin + ci) * 9 + tap];
          }
        } else {
          const size_t dst = c.w_off + (((size_t)grp * nchunk + chk) * ng + n) * c.kc + kk;
          if (c.kind == 1) {
            blob[dst] = w[(size_t)co * c.cin + ci];
          } else {
            // GEMM k = dy*2C + dx*C + cc  <-  weight[co][cc][dy][dx]   (C = cin/4)
            const int Cq = c.cin / 4, dy = ci / (2 * Cq), dx = (ci / Cq) & 1, cc = ci % Cq;
            blob[dst] = w[(((size_t)co * Cq + cc) * 2 + dy) * 2 + dx];
          }
        }
      }
    }
    (void)ngroups;
    if (c.head())   // dot-product form of the head layers: [chunk][tap][4][16], zero rows / columns as padding
      for (int co = 0; co < c.cout; ++co)
        for (int ci = 0; ci < c.cin; ++ci)
          for (int tap = 0; tap < 9; ++tap)
            blob[c.wd_off + ((((size_t)(ci / 16) * 9 + tap) * 4 + co) * 16) + ci % 16] = w[((size_t)co * c.cin + ci) * 9 + tap];
    // split-fp16 pack (conv3x3.hip PREC 1): K walked in chunks of 16; each row is 16 hi halves then 16 lo
    // halves of w * 2^e; the epilogue scale carries the 2^-e.  e = 11 keeps the lo half of ordinary weights a normal
    // fp16; a layer with large weights (|w| * 2^11 would pass the fp16 range: |w| >= 16) takes the largest e that keeps
    // |w| * 2^e <= 2^15, so no checkpoint can turn a weight into inf (hi) / -inf (lo) silently.  Powers of two: the
    // products and the fp32 accumulation are the same bits up to the exponent, whatever e is.
    {
      float wmax = 0.f;
      for (float v : w) {
        if (!std::isfinite(v)) return fail(KP2D_ERR_WEIGHT, "%s: non-finite weight value", c.name.c_str());
        wmax = std::max(wmax, std::fabs(v));
      }
      int e16 = 11;
      while (e16 > -96 && wmax * std::ldexp(1.0f, e16) > 32768.0f) --e16;
      const float wscale = std::ldexp(1.0f, e16), wunscale = std::ldexp(1.0f, -e16);
      uint16_t* h16 = reinterpret_cast<uint16_t*>(&blob[c.w16_off]);
      const int nchunk16 = (c.cin + 15) / 16;
      for (int q = 0; q < c.npad; ++q) {
        int co = -1;
        if (q < c.cout) co = c.shuffle ? 4 * (q % cq) + (q / cq) : q;
        blob[c.sc16_off + q] = co >= 0 ? sc[co] * wunscale : 0.f;
        if (co < 0) continue;
        const int grp = q / ng, n = q % ng;
        for (int ci = 0; ci < c.cin; ++ci) {
          const int chk = ci / 16, kk = ci % 16;
          for (int tap = 0; tap < c.taps; ++tap) {
            float wv;
            if (c.kind == 0) wv = w[((size_t)co * c.cin + ci) * 9 + tap];
            else if (c.kind == 1) wv = w[(size_t)co * c.cin + ci];
            else {
              const int Cq = c.cin / 4, dy = ci / (2 * Cq), dx = (ci / Cq) & 1, cc = ci % Cq;
              wv = w[(((size_t)co * Cq + cc) * 2 + dy) * 2 + dx];
            }
            wv *= wscale;
            const uint16_t hi = f16_bits(wv);
            const uint16_t lo = f16_bits(wv - f16_value(hi));
            // 3x3 layers: the nine taps of a chunk sit in slot order {0,1,3,4,2,5,6,7,8} (conv3x3_f16.hip pairs
            // slots (0,1) (2,3) (4,5) (6,7) into one K = 32 MFMA each; slot 8 is the single)
            static const int kSlot[9] = {0, 1, 4, 2, 3, 5, 6, 7, 8};
            const int slot = c.kind == 0 ? kSlot[tap] : tap;
            const size_t row = ((((size_t)grp * nchunk16 + chk) * c.taps + slot) * ng + n) * 32;   // in halves
            h16[row + kk] = hi;
            h16[row + 16 + kk] = lo;
            if (c.npad >= 64) {   // 32-channel groups of the same rows
              uint16_t* n16 = reinterpret_cast<uint16_t*>(&blob[c.w16n_off]);
              const size_t rown = ((((size_t)(q / 32) * nchunk16 + chk) * c.taps + slot) * 32 + (q % 32)) * 32;
              n16[rown + kk] = hi;
              n16[rown + 16 + kk] = lo;
            }
            if (c.w16t_off) {     // tap (dy, dx) in the slot of tap (dx, dy): what a tile that walks the map transposed multiplies
              uint16_t* t16 = reinterpret_cast<uint16_t*>(&blob[c.w16t_off]);
              const int slot_t = kSlot[3 * (tap % 3) + tap / 3];
              const size_t rowt = ((((size_t)grp * nchunk16 + chk) * c.taps + slot_t) * ng + n) * 32;
              t16[rowt + kk] = hi;
              t16[rowt + 16 + kk] = lo;
            }
          }
        }
      }
    }
  }
  for (const auto& kv : m->vecs) {
    const auto& src = *host_get(m, kv.first);
    const std::string& key = kv.first;
    if (key.size() > 13 && key.compare(key.size() - 13, 13, ".net.0.weight") == 0 && key.find(".net.1.") != std::string::npos) {
      const int h = kv.second.n / 9;                       // depthwise [h][1][3][3] -> [9][h]
      for (int c = 0; c < h; ++c)
        for (int t = 0; t < 9; ++t) blob[kv.second.off + (size_t)t * h + c] = src[(size_t)c * 9 + t];
    } else {
      std::copy(src.begin(), src.end(), blob.begin() + kv.second.off);
    }
  }
  if (m->cfg.global_descriptor == KP2D_GD_NETVLAD && !m->cfg.remove_netvlad) {
    const auto& wa = *host_get(m, "vlad_head.netvlad.conv.weight");
    const auto& ce = *host_get(m, "vlad_head.netvlad.centroids");
    std::copy(wa.begin(), wa.end(), blob.begin() + m->vlad_wa);
    std::copy(ce.begin(), ce.end(), blob.begin() + m->vlad_cent);
  }
  return KP2D_OK;
}

}  // namespace kp2d
