// The launch sequence of one LightGlue.forward (lightglue/lightglue.py:484-614) over the packed blob and the workspace walk of
// lightglue_desc.cpp.  No CPU compute path.
#include "lightglue_plan.h"

#include <hip/hip_runtime.h>

#include <cmath>

#include "api_common.h"
#include "device_guard.h"
#include "kp2d_kernels.h"
#include "lightglue_form.h"
#include "options.h"

namespace kp2d {

// the launch sequence of one forward (lightglue.py:484-614)
int run_forward(kp2d_lg* m, const float* kpts0, const float* kpts1, const float* desc0, const float* desc1,
                const float* size0, const float* size1, const int32_t* n0, const int32_t* n1, int B, int M, int N,
                float filter_threshold, float* log_assignment, int64_t* matches0, int64_t* matches1,
                float* mscores0, float* mscores1, float* ref_desc0, float* ref_desc1, const PruneIO* pr, void* workspace,
                size_t workspace_bytes, void* stream) {
  if ((n0 == nullptr) != (n1 == nullptr)) return fail(KP2D_ERR_ARG, "keypoint counts must be given for both sets or neither");
  if (n0 && (!size0 || !size1)) return fail(KP2D_ERR_ARG, "padded keypoint sets need the image sizes (the default derives them from every row)");
  if (!m || !kpts0 || !kpts1 || !desc0 || !desc1 || !log_assignment || !workspace) return fail(KP2D_ERR_ARG, "null argument");
  if (!matches0 || !matches1 || !mscores0 || !mscores1) return fail(KP2D_ERR_ARG, "null match outputs");
  if (!m->finalized) return fail(KP2D_ERR_STATE, "weights not finalised (kp2d_lg_finalize_weights)");
  if (B < 1 || M < 1 || N < 1) return fail(KP2D_ERR_ARG, "B, M, N must be >= 1");
  if ((long)B * (M + N) > (1l << 24)) return fail(KP2D_ERR_ARG, "too many keypoints in one call");
  if ((uintptr_t)workspace % ALIGN) return fail(KP2D_ERR_WORKSPACE, "workspace must be %zu-byte aligned", ALIGN);
  const Ws w = layout(workspace, m, B, M, N);
  if (workspace_bytes < w.total) return fail(KP2D_ERR_WORKSPACE, "workspace %zu B < required %zu B", workspace_bytes, w.total);
  kp2d::DeviceGuard guard(m->cfg.device);
  hipStream_t st = (hipStream_t)stream;
  const int d = m->cfg.descriptor_dim, din = m->cfg.input_dim, heads = m->cfg.num_heads, hd = d / heads;
  const int R = B * (M + N), R0 = B * M;
  float *X = w.x, *T3 = w.t3, *CTX = w.ctx, *MSG = w.msg, *HB = w.hb, *CS = w.cs, *FZ = w.fz;
  // padded keypoint sets: [n0 | n1] as the key counts of the 2B sequences the attention launches walk
  // (point pruning: the counts always exist — they are what shrinks between the layers)
  int32_t* CNT = n0 || pr ? w.cnt : nullptr;
  if (n0 && !pr) {
    HIP_TRY(hipMemcpyAsync(CNT, n0, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(CNT + B, n1, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
  }
  const float* blob = m->blob;
  int e;
#define LG_CHECK(call, what)                                                                                    \
  do {                                                                                                          \
    e = (call);                                                                                                 \
    if (e) return fail(e < 0 ? KP2D_ERR_UNSUPPORTED : KP2D_ERR_HIP, "%s: launch failed (%d)", what, e);         \
  } while (0)

  LgPruneArgs pa{};
  if (pr) {
    pa.x = X; pa.cs = CS; pa.cnt = CNT; pa.ind0 = pr->keep0; pa.ind1 = pr->keep1; pa.prune0 = pr->prune0; pa.prune1 = pr->prune1;
    pa.B = B; pa.M = M; pa.N = N; pa.D = d; pa.hd = hd; pa.thr = pr->thr;
    LG_CHECK(launch_lg_prune_init(pa, n0, n1, st), "prune init");
  }

  {
    LgPosArgs a{kpts0, kpts1, size0, size1, blob + m->wr, CS, B, M, N, hd};
    LG_CHECK(launch_lg_posenc(a, st), "posenc");
  }
  auto linear = [&](const Lin& l, const float* x0, int k0, int xs0, const float* x1, int k1, int xs1, float* out, int os,
                    int rows, int nvalid, int epi) {
    LgLinArgs a{};
    a.x0 = x0; a.x1 = x1; a.k0 = k0; a.k1 = k1; a.xs0 = xs0; a.xs1 = xs1;
    a.w = blob + l.w; a.bias = blob + l.b; a.out = out; a.os = os; a.oo = 0;
    a.rows = rows; a.nout = l.nout; a.nvalid = nvalid; a.epi = epi;
    return a;
  };
  if (din != d) {
    LgLinArgs a = linear(m->input_proj, desc0, din, din, nullptr, 0, 0, X, d, R0, d, LG_EPI_NONE);
    LG_CHECK(launch_lg_linear(a, st), "input_proj");
    a = linear(m->input_proj, desc1, din, din, nullptr, 0, 0, X + (size_t)R0 * d, d, B * N, d, LG_EPI_NONE);
    LG_CHECK(launch_lg_linear(a, st), "input_proj");
  } else {
    HIP_TRY(hipMemcpyAsync(X, desc0, (size_t)R0 * d * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(X + (size_t)R0 * d, desc1, (size_t)B * N * d * 4, hipMemcpyDeviceToDevice, st));
  }
  auto ffn = [&](const Ffn& f, const char* what) -> int {
    // x + ffn(cat[x, message]) (lightglue.py:261 / :325-326): Linear -> LayerNorm -> GELU, then Linear + residual in place
    LgLinArgs a = linear(f.l0, X, d, d, MSG, d, d, HB, 2 * d, R, 2 * d, LG_EPI_LNGELU);
    a.ln_g = blob + f.g; a.ln_b = blob + f.be;
    LG_CHECK(launch_lg_linear(a, st), what);
    a = linear(f.l3, HB, 2 * d, 2 * d, nullptr, 0, 0, X, d, R, d, LG_EPI_RESID);
    a.res = X; a.rs = d;
    LG_CHECK(launch_lg_linear(a, st), what);
    return KP2D_OK;
  };
  // D = 32 (configs S, A): out_proj / to_out + ffn + residual as ONE row-local kernel (lightglue.hip lg_tail_kernel).
  // `next`: the token-wise projection that follows the block (the cross block's [to_qk | to_v], the next layer's Wqkv
  // with rotary, the final projection) runs in the tail's launch on the rows it has just updated: 8 launches fewer
  // per forward than one lg_linear per projection (the matcher is a chain of ~35 dependent launches of ~10 us)
  const LgForm form = choose_lg_form(d, tuning().lg_fuse, tuning().lg_fuse_next);      // (lightglue_form.h)
  const bool fuse_tail = form.fuse_tail, fused = form.fused;
  auto tail = [&](const Lin& proj, const Ffn& f, const char* what, const Lin* next, float* nout, int nos, int nvalid,
                  bool rotary) -> int {
    LgTailArgs t{};
    t.x = X; t.ctx = CTX; t.io = blob + proj.mf; t.bo = blob + proj.b; t.i1 = blob + f.l0.mf; t.b1 = blob + f.l0.b;
    t.ln_g = blob + f.g; t.ln_b = blob + f.be; t.i2 = blob + f.l3.mf; t.b2 = blob + f.l3.b; t.rows = R; t.D = d;
    if (next) {
      t.in = blob + next->mf; t.bn = blob + next->b; t.on = nout; t.nn = next->nout; t.nos = nos; t.nvalid = nvalid;
      if (rotary) { t.cs = CS; t.hd = hd; t.rot_cols = 2 * d; }
      if (next == &m->final) t.wz = blob + next->w;      // the matchability logit (column d) as an fp32 dot product
    }
    LG_CHECK(launch_lg_tail(t, st), what);
    return KP2D_OK;
  };
  // the sequences of one attention launch (lightglue_form.h): q / k rows of T3 with `cols` columns, keys counted by CNT
  auto attention = [&](const LgAttLaunch& l, int cols, int k_off, int v_off, const char* what) -> int {
    const size_t rq = l.q_set ? (size_t)R0 : 0, rk = l.k_set ? (size_t)R0 : 0;
    AttnArgs t{T3 + rq * cols, T3 + rk * cols, CTX + rq * d, l.B, l.S, l.T, d, heads, 1.f / std::sqrt((float)hd)};
    t.q_stride = cols; t.kv_stride = cols; t.k_off = k_off; t.v_off = v_off; t.out_stride = d;
    t.prec = 1;      // split-fp16 MFMA (fp32-grade, attention.hip): 3x faster than the fp32 16x16x4 kernel at head dim 8
    t.kv_bshift = l.kv_bshift;
    t.tcount = CNT ? CNT + (l.k_set ? B : 0) : nullptr;      // the counts of the set the KEYS come from
    LG_CHECK(launch_attention(t, st), what);
    return KP2D_OK;
  };
  LgAttLaunch att[2];
  for (int i = 0; i < m->cfg.n_layers; ++i) {
    const Layer& L = m->layers[i];
    // ---- SelfBlock (lightglue.py:247-261), both images in one launch per token-wise layer ----
    {
      LgLinArgs a = linear(L.qkv, X, d, d, nullptr, 0, 0, T3, 3 * d, R, 3 * d, LG_EPI_ROTARY);
      a.cs = CS; a.hd = hd; a.rot_cols = 2 * d;
      // (point pruning: the rows are compacted between a cross block and the next Wqkv, so every layer projects here)
      if (fused && (i == 0 || pr)) {   // the tail kernel's projection-only mode: same arithmetic as every later Wqkv
        LgTailArgs t{};
        t.x = X; t.rows = R; t.D = d;
        t.in = blob + L.qkv.mf; t.bn = blob + L.qkv.b; t.on = T3; t.nn = L.qkv.nout; t.nos = 3 * d; t.nvalid = 3 * d;
        t.cs = CS; t.hd = hd; t.rot_cols = 2 * d;
        LG_CHECK(launch_lg_tail(t, st), "self_attn.Wqkv");
      } else if (!fused) {             // (fused, i > 0: done by the previous tail)
        LG_CHECK(launch_lg_linear(a, st), "self_attn.Wqkv");
      }
      // rows of T3: [q | k | v].  M == N: both images as one batch of 2B sequences
      for (int j = 0, n = lg_attention_launches(B, M, N, false, att); j < n; ++j) {
        int rc = attention(att[j], 3 * d, d, 2 * d, "self_attn.inner_attn");
        if (rc != KP2D_OK) return rc;
      }
      if (fuse_tail && d == 32) {
        int rc = tail(L.out_proj, L.fs, "self_attn tail", fused ? &L.qkv_x : nullptr, T3, 2 * d, 2 * d, false);
        if (rc != KP2D_OK) return rc;
      } else {
        a = linear(L.out_proj, CTX, d, d, nullptr, 0, 0, MSG, d, R, d, LG_EPI_NONE);
        LG_CHECK(launch_lg_linear(a, st), "self_attn.out_proj");
        int rc = ffn(L.fs, "self_attn.ffn");
        if (rc != KP2D_OK) return rc;
      }
    }
    // ---- CrossBlock (lightglue.py:303-327): [to_qk | to_v] in one layer, attention both ways ----
    {
      LgLinArgs a = linear(L.qkv_x, X, d, d, nullptr, 0, 0, T3, 2 * d, R, 2 * d, LG_EPI_NONE);
      if (!fused) LG_CHECK(launch_lg_linear(a, st), "cross_attn.to_qk/to_v");
      // rows of T3: [qk | v], the keys are the OTHER set's rows.  M == N: both directions in one launch, sequence b
      // attends to sequence (b + B) mod 2B
      for (int j = 0, n = lg_attention_launches(B, M, N, true, att); j < n; ++j) {
        int rc = attention(att[j], 2 * d, 0, d, "cross_attn");
        if (rc != KP2D_OK) return rc;
      }
      if (fuse_tail && d == 32) {
        const bool last = i + 1 == m->cfg.n_layers;
        const Lin* nx = !fused || (pr && !last) ? nullptr : (last ? &m->final : &m->layers[i + 1].qkv);
        int rc = last ? tail(L.to_out, L.fc, "cross_attn tail", nx, FZ, d + 32, d + 1, false)
                      : tail(L.to_out, L.fc, "cross_attn tail", nx, T3, 3 * d, 3 * d, true);
        if (rc != KP2D_OK) return rc;
      } else {
        a = linear(L.to_out, CTX, d, d, nullptr, 0, 0, MSG, d, R, d, LG_EPI_NONE);
        LG_CHECK(launch_lg_linear(a, st), "cross_attn.to_out");
        int rc = ffn(L.fc, "cross_attn.ffn");
        if (rc != KP2D_OK) return rc;
      }
    }
    // ---- point pruning after every layer but the last (lightglue.py:553-556, :564-579) ----
    if (pr && i + 1 < m->cfg.n_layers) {
      pa.w = blob + m->prune_w[i];
      LG_CHECK(launch_lg_prune(pa, st), "point pruning");
    }
  }
  {
    LgLinArgs a = linear(m->final, X, d, d, nullptr, 0, 0, FZ, d + 32, R, d + 1, LG_EPI_NONE);
    if (!fused || m->cfg.n_layers == 0) LG_CHECK(launch_lg_linear(a, st), "log_assignment.final_proj");
    LgAssignArgs g{};
    g.fz = FZ; g.fs = d + 32; g.D = d; g.B = B; g.M = M; g.N = N; g.scores = log_assignment;
    g.rp_m = w.rp_m; g.rp_s = w.rp_s; g.cp_m = w.cp_m; g.cp_s = w.cp_s;
    g.rmax = w.rmax; g.cmax = w.cmax; g.rarg = w.rarg; g.carg = w.carg;
    g.th = filter_threshold;
    g.cnt0 = n0; g.cnt1 = n1;
    if (pr) {      // survivors' matches go back to original indices; pruned and padding rows keep -1 / 0 (:586-594)
      g.cnt0 = CNT; g.cnt1 = CNT + B; g.ind0 = pr->keep0; g.ind1 = pr->keep1;
      HIP_TRY(hipMemsetAsync(matches0, 0xff, (size_t)R0 * 8, st));
      HIP_TRY(hipMemsetAsync(matches1, 0xff, (size_t)B * N * 8, st));
      HIP_TRY(hipMemsetAsync(mscores0, 0, (size_t)R0 * 4, st));
      HIP_TRY(hipMemsetAsync(mscores1, 0, (size_t)B * N * 4, st));
    }
    g.matches0 = matches0; g.matches1 = matches1; g.mscores0 = mscores0; g.mscores1 = mscores1;
    LG_CHECK(launch_lg_assign(g, st), "log_assignment");
  }
  if (pr) {
    HIP_TRY(hipMemcpyAsync(pr->nkeep0, CNT, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(pr->nkeep1, CNT + B, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
  }
  if (ref_desc0 && ref_desc1 == ref_desc0 + (size_t)R0 * d) {      // one buffer behind both outputs: one copy
    HIP_TRY(hipMemcpyAsync(ref_desc0, X, (size_t)R * d * 4, hipMemcpyDeviceToDevice, st));
    return KP2D_OK;
  }
  if (ref_desc0) HIP_TRY(hipMemcpyAsync(ref_desc0, X, (size_t)R0 * d * 4, hipMemcpyDeviceToDevice, st));
  if (ref_desc1) HIP_TRY(hipMemcpyAsync(ref_desc1, X + (size_t)R0 * d, (size_t)B * N * d * 4, hipMemcpyDeviceToDevice, st));
#undef LG_CHECK
  return KP2D_OK;
}

}  // namespace kp2d
