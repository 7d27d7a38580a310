// LightGlue's description (which tensors a configuration has, under the reference's state_dict names and shapes), weight
// packing (the kernels' layouts of the linear layers) and workspace walk.  Pure host code, no HIP: hipcc compiles it into
// the library, g++ into the driver of tests/test_lightglue_desc.py.
#include "lightglue_desc.h"

#include <algorithm>
#include <cmath>

#include "api_common.h"
#include "f16_host.h"

namespace kp2d {

namespace {

int pad32(int n) { return (n + 31) / 32 * 32; }

void add_spec(LgDesc* m, const std::string& k, std::vector<int64_t> shape) {
  m->index[k] = (int)m->specs.size();
  m->specs.push_back(WeightSpec{k, std::move(shape)});
}
void add_linear(LgDesc* m, const std::string& p, int out, int in) {
  add_spec(m, p + ".weight", {out, in});
  add_spec(m, p + ".bias", {out});
}
void add_ffn(LgDesc* m, const std::string& p, int d) {
  add_linear(m, p + ".0", 2 * d, 2 * d);
  add_spec(m, p + ".1.weight", {2 * d});
  add_spec(m, p + ".1.bias", {2 * d});
  add_linear(m, p + ".3", d, 2 * d);
}

// the widths the kernels are built for
int check_config(const kp2d_lg_config* cfg) {
  const int d = cfg->descriptor_dim;
  if (d % 32 || d < 32 || d > 64) return fail(KP2D_ERR_UNSUPPORTED, "descriptor_dim=%d (32 and 64 are built)", d);
  if (cfg->num_heads < 1 || d % cfg->num_heads || (d / cfg->num_heads) % 4 || d / cfg->num_heads > 16)
    return fail(KP2D_ERR_UNSUPPORTED, "num_heads=%d: head dim must be a multiple of 4, <= 16", cfg->num_heads);
  if (cfg->input_dim < 1 || cfg->input_dim > 128) return fail(KP2D_ERR_UNSUPPORTED, "input_dim=%d (<= 128)", cfg->input_dim);
  if (cfg->n_layers < 1 || cfg->n_layers > 32) return fail(KP2D_ERR_ARG, "n_layers=%d", cfg->n_layers);
  return KP2D_OK;
}

}  // namespace

// registration order of LightGlue.__init__ (lightglue.py:444-470)
int describe(LgDesc* m) {
  const int rc = check_config(&m->cfg);
  if (rc != KP2D_OK) return rc;
  const int d = m->cfg.descriptor_dim, din = m->cfg.input_dim, n = m->cfg.n_layers, hd = d / m->cfg.num_heads;
  if (din != d) add_linear(m, "input_proj", d, din);
  add_spec(m, "posenc.Wr.weight", {hd / 2, 2});
  for (int i = 0; i < n; ++i) {
    const std::string s = "transformers." + std::to_string(i) + ".self_attn";
    add_linear(m, s + ".Wqkv", 3 * d, d);
    add_linear(m, s + ".out_proj", d, d);
    add_ffn(m, s + ".ffn", d);
    const std::string c = "transformers." + std::to_string(i) + ".cross_attn";
    add_linear(m, c + ".to_qk", d, d);
    add_linear(m, c + ".to_v", d, d);
    add_linear(m, c + ".to_out", d, d);
    add_ffn(m, c + ".ffn", d);
  }
  for (int i = 0; i < n; ++i) {
    add_linear(m, "log_assignment." + std::to_string(i) + ".matchability", 1, d);
    add_linear(m, "log_assignment." + std::to_string(i) + ".final_proj", d, d);
  }
  for (int i = 0; i + 1 < n; ++i) add_linear(m, "token_confidence." + std::to_string(i) + ".token.0", 1, d);

  size_t off = 0;
  auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats, ALIGN / 4); return o; };
  auto lin = [&](int K, int nout) {
    Lin l; l.K = K; l.nout = pad32(nout); l.w = take((size_t)K * l.nout); l.b = take(l.nout);
    if (K % 32 == 0) l.mf = take((size_t)K * l.nout);
    return l;
  };
  auto ffn = [&]() { Ffn f; f.l0 = lin(2 * d, 2 * d); f.g = take(2 * d); f.be = take(2 * d); f.l3 = lin(2 * d, d); return f; };
  if (din != d) m->input_proj = lin(din, d);
  m->wr = take(hd);
  m->layers.resize(n);
  for (auto& L : m->layers) {
    L.qkv = lin(d, 3 * d); L.out_proj = lin(d, d); L.fs = ffn();
    L.qkv_x = lin(d, 2 * d); L.to_out = lin(d, d); L.fc = ffn();
  }
  m->final = lin(d, d + 1);
  for (int i = 0; i + 1 < n; ++i) m->prune_w.push_back(take((size_t)d + 1));      // appended: no earlier offset moves
  m->blob_floats = off;
  return KP2D_OK;
}

namespace {

const std::vector<float>& H(const LgDesc* m, const std::string& k) { return m->host.at(k); }

// W [nout][K] (torch Linear layout) -> W^T [K][nout_pad] at column offset c0, rows optionally permuted / scaled
void put_linear(std::vector<float>& blob, const Lin& l, const std::vector<float>& w, const std::vector<float>* b,
                int rows, int c0, float scale, const std::vector<int>* perm = nullptr) {
  for (int r = 0; r < rows; ++r) {
    const int c = c0 + (perm ? (*perm)[r] : r);
    for (int k = 0; k < l.K; ++k) blob[l.w + (size_t)k * l.nout + c] = w[(size_t)r * l.K + k] * scale;
    if (b) blob[l.b + c] = (*b)[r] * scale;
  }
}

// W^T [K][nout] (already in the blob) -> the A operands of v_mfma_f32_16x16x32_f16 for Y^T = W X^T, one 2-KB block
// per (16-feature tile t, 32-wide k step s): [hi | lo][lane][8 halves].  Lane l = (feature 16t + l%16, group g = l/16);
// its element j multiplies input feature 32s + 4g + j (j < 4) or 32s + 16 + 4g + (j - 4): the order in which the lanes
// of the PREVIOUS product's accumulator tiles (feature 16t' + 4g + r of row l%16) hold a row — a product's output is
// the next product's B operand without leaving its registers (lightglue.hip lg_tail_kernel).
void mfma_image(std::vector<float>& blob, const Lin& l) {
  if (!l.mf) return;
  uint16_t* img = reinterpret_cast<uint16_t*>(blob.data() + l.mf);
  const int KS = l.K / 32;
  for (int t = 0; t < l.nout / 16; ++t)
    for (int s = 0; s < KS; ++s)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int n = 16 * t + (lane & 15), g = lane >> 4;
          const int k = 32 * s + (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4));
          const float w = blob[l.w + (size_t)k * l.nout + n];
          const uint16_t hi = f16_bits(w);
          const uint16_t lo = f16_bits(w - f16_value(hi));
          uint16_t* blk = img + (size_t)(t * KS + s) * 1024;
          blk[lane * 8 + j] = hi;
          blk[512 + lane * 8 + j] = lo;
        }
}

}  // namespace

int pack(const LgDesc* m, std::vector<float>& blob) {
  for (const auto& s : m->specs)
    if (!m->host.count(s.key)) return fail(KP2D_ERR_WEIGHT, "missing tensor '%s'", s.key.c_str());
  blob.assign(m->blob_floats, 0.f);
  const int d = m->cfg.descriptor_dim, n = m->cfg.n_layers, h = m->cfg.num_heads, hd = d / h;
  if (m->cfg.input_dim != d) put_linear(blob, m->input_proj, H(m, "input_proj.weight"), &H(m, "input_proj.bias"), d, 0, 1.f);
  { const auto& wr = H(m, "posenc.Wr.weight"); std::copy(wr.begin(), wr.end(), blob.begin() + m->wr); }
  // Wqkv rows: reference channel h*(3*hd) + dd*3 + t (unflatten(-1, (heads, -1, 3)), lightglue.py:254-255) -> t*d + h*hd + dd
  std::vector<int> perm(3 * d);
  for (int hh = 0; hh < h; ++hh)
    for (int dd = 0; dd < hd; ++dd)
      for (int t = 0; t < 3; ++t) perm[hh * 3 * hd + dd * 3 + t] = t * d + hh * hd + dd;
  auto put_ffn = [&](const Ffn& f, const std::string& p) {
    put_linear(blob, f.l0, H(m, p + ".0.weight"), &H(m, p + ".0.bias"), 2 * d, 0, 1.f);
    std::copy(H(m, p + ".1.weight").begin(), H(m, p + ".1.weight").end(), blob.begin() + f.g);
    std::copy(H(m, p + ".1.bias").begin(), H(m, p + ".1.bias").end(), blob.begin() + f.be);
    put_linear(blob, f.l3, H(m, p + ".3.weight"), &H(m, p + ".3.bias"), d, 0, 1.f);
  };
  for (int i = 0; i < n; ++i) {
    const Layer& L = m->layers[i];
    const std::string s = "transformers." + std::to_string(i) + ".self_attn";
    put_linear(blob, L.qkv, H(m, s + ".Wqkv.weight"), &H(m, s + ".Wqkv.bias"), 3 * d, 0, 1.f, &perm);
    put_linear(blob, L.out_proj, H(m, s + ".out_proj.weight"), &H(m, s + ".out_proj.bias"), d, 0, 1.f);
    put_ffn(L.fs, s + ".ffn");
    const std::string c = "transformers." + std::to_string(i) + ".cross_attn";
    put_linear(blob, L.qkv_x, H(m, c + ".to_qk.weight"), &H(m, c + ".to_qk.bias"), d, 0, 1.f);
    put_linear(blob, L.qkv_x, H(m, c + ".to_v.weight"), &H(m, c + ".to_v.bias"), d, d, 1.f);
    put_linear(blob, L.to_out, H(m, c + ".to_out.weight"), &H(m, c + ".to_out.bias"), d, 0, 1.f);
    put_ffn(L.fc, c + ".ffn");
  }
  // MatchAssignment of the LAST layer (lightglue.py:572): final_proj / d^0.25 (:389-390) and the matchability logit
  const std::string a = "log_assignment." + std::to_string(n - 1);
  put_linear(blob, m->final, H(m, a + ".final_proj.weight"), &H(m, a + ".final_proj.bias"), d, 0, 1.f / std::pow((float)d, 0.25f));
  put_linear(blob, m->final, H(m, a + ".matchability.weight"), &H(m, a + ".matchability.bias"), 1, d, 1.f);
  for (const Layer& L : m->layers)
    for (const Lin* l : {&L.qkv, &L.out_proj, &L.qkv_x, &L.to_out, &L.fs.l0, &L.fs.l3, &L.fc.l0, &L.fc.l3}) mfma_image(blob, *l);
  mfma_image(blob, m->final);
  // get_matchability of the layers that prune (lightglue.py:395-396, :566 / :573)
  for (int i = 0; i + 1 < n; ++i) {
    const std::string q = "log_assignment." + std::to_string(i) + ".matchability";
    std::copy(H(m, q + ".weight").begin(), H(m, q + ".weight").end(), blob.begin() + m->prune_w[i]);
    blob[m->prune_w[i] + d] = H(m, q + ".bias")[0];
  }
  return KP2D_OK;
}

Ws layout(void* workspace, const LgDesc* m, int B, int M, int N) {
  const size_t R = (size_t)B * (M + N), d = m->cfg.descriptor_dim, hd = d / m->cfg.num_heads;
  Carve c(workspace);
  Ws w{};
  w.x = c.take<float>(R * d); w.t3 = c.take<float>(R * 3 * d); w.ctx = c.take<float>(R * d); w.msg = c.take<float>(R * d);
  w.hb = c.take<float>(R * 2 * d); w.cs = c.take<float>(R * hd); w.fz = c.take<float>(R * (d + 32));
  const size_t rp = (size_t)B * ((N + 63) / 64) * M, cp = (size_t)B * ((M + 63) / 64) * N;      // per-tile partials
  w.rp_m = c.take<float>(rp); w.rp_s = c.take<float>(rp); w.cp_m = c.take<float>(cp); w.cp_s = c.take<float>(cp);
  w.rmax = c.take<float>(rp); w.rarg = c.take<int>(rp); w.cmax = c.take<float>(cp); w.carg = c.take<int>(cp);
  w.cnt = c.take<int32_t>((size_t)2 * B);
  w.total = c.bytes();
  return w;
}

}  // namespace kp2d
