// Internal launch interface between the host code (plan.cpp, kp2d_api.cpp, lightglue_plan.cpp) and the HIP kernels: only what
// crosses files (match.hip, keypoint_metrics.hip, dense_metrics.hip keep their argument structs and entry points to themselves).
// Not part of the public ABI (that is include/kp2d.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_policy.h"

namespace kp2d {

struct Conv1aArgs {                   // backbone.conv1a: NCHW frame in -> NHWC out, Cin = 3 (RGB) or 1 (use_color=False)
  const float* x;                     // [B,cin,H,W]
  const float* w;                     // [9*cin][cout]  (k = ci*9 + dy*3 + dx)
  int cin;
  const float* scale; const float* shift;
  float* out; int B, H, W, cout, act;
};

int launch_conv3x3(const ConvArgs& a, int kc, hipStream_t s);
// tile form the calling thread's last launch_conv3x3* call chose ("<2,1,16>", "ws", "wsm", ...; "" for the fp32 / 1x1 kernels):
// kp2d_profile_get reports it behind the kernel family, so a test can assert WHICH kernel it covered
const char* conv3x3_last_variant();
void conv3x3_note_variant(const char* v);
int launch_conv1a(const Conv1aArgs& a, hipStream_t s);
int launch_conv1a_u8(const Conv1aArgs& a, const unsigned char* frames, int Hs, int Ws, hipStream_t s);   // frame front-end fused in
// conv3x3_f16.hip: conv1a in the split-fp16 arithmetic of the fused first layer (STEM), bit-identical to it; frames != null: uint8 frames in
int launch_conv1a_mfma(const Conv1aArgs& a, const float* wscale_dev, const unsigned char* frames, int Hs, int Ws, hipStream_t s);
int launch_head3x3_pair(const ConvArgs& a0, const ConvArgs& a1, hipStream_t s);   // a 1-channel and a 2-channel head, one launch
int launch_head3x3(const ConvArgs& a, hipStream_t s);         // head3x3.hip: taps = 9, cout <= 4, planar outputs (exact fp32 dot products)
int launch_conv3x3_f16x3(const ConvArgs& a, hipStream_t s);   // conv3x3_f16.hip: taps = 9, prec = 1, the form conv_policy.h chooses
// 2-4 independent small-grid layers as one launch; -1000: not all of them are layers of the single-frame form
int launch_conv3x3_f16x3_multi(const ConvArgs* list, int n, hipStream_t s);
// conv3x3_wsm.hip / conv3x3_s16.hip: the persistent forms, launched as conv_policy.h chose them
int launch_conv3x3_f16x3_wsm(const ConvArgs& a, const ConvChoice& c, hipStream_t s);
int launch_conv3x3_f16x3_s16(const ConvArgs& a, const ConvChoice& c, hipStream_t s);
int launch_conv3x3_f16x3_s16_ids(const ConvArgs& a, int grid, long nitems, hipStream_t s);   // its ST_IDS form (conv3x3_s16_ids.hip)
// kp2d_set_tap on an S16P tensor: channels [c0, c0 + C) of a Ct-channel tensor -> planar fp32
int launch_s16p_to_nchw(const float* in, float* out, int B, int C, int H, int W, int Ct, int c0, hipStream_t s);

// ---- NetVLAD (modules/aggregators/netvlad.py:79-106) ---------------------------------------
struct VladArgs {
  const float* x;        // encoder output, NHWC [B][S][C]
  const float* wa;       // soft-assign 1x1 conv weight [K][C]
  const float* cent;     // centroids [K][C]
  float* part;           // workspace [B][nsplit][K*C + K]
  float* out;            // [B][K*C]
  int B, S, C, K, nsplit;
  int tps = 1;           // > 1: one workgroup per 64-pixel tile, tps tiles per slab (netvlad_tiles_per_slab); part holds nsplit*tps rows
  int prec = 0;          // 1: the soft-assignment logits as split-fp16 products (f16x3 mode); the aggregation is exact fp32 in both
};
int launch_netvlad(const VladArgs& a, hipStream_t s);
struct PoolArgs { const float* x; const float* p; float* out; int B, C, Hc, Wc; };   // GeM (p = exponent) / ConvAP pooling
int launch_gem(const PoolArgs& a, hipStream_t s);
int launch_convap_pool(const PoolArgs& a, hipStream_t s);
int netvlad_nsplit(int S);
int netvlad_tiles_per_slab(int S, int B);

// ---- post-processing (models/kp2dtiny.py:593-647 / 959-1015) -------------------------------
struct PostArgs {
  const float* score_in;  // [B,1,Hc,Wc] sigmoid score
  const float* shift;     // [B,2,Hc,Wc] tanh shift
  const float* feat;      // [B,C,Hf,Wf] dense descriptors (NCHW)
  float* score_out;       // [B,1,Hc,Wc]
  float* coord;           // [B,2,Hc,Wc] pixels, ch0 = x
  float* desc;            // [B,C,Hc,Wc] sampled + L2 normalised (nullptr: training mode, no sampling)
  int B, C, Hc, Wc, Hf, Wf, H, W, cell;
  float cross_ratio;
};
int launch_post(const PostArgs& a, hipStream_t s);

struct ArgmaxArgs { const float* seg; int64_t* ids; int B, C, HW; };
int launch_seg_argmax(const ArgmaxArgs& a, hipStream_t s);
int launch_post_seg(const PostArgs& a, const ArgmaxArgs& g, hipStream_t s);      // both in one launch when shapes allow
struct SegSampleArgs { const float* seg; const float* coord; int64_t* ids; int B, C, Hs, Ws, Hc, Wc, H, W; };
int launch_seg_sample_argmax(const SegSampleArgs& a, hipStream_t s);

// ---- keypoint selection (callers K1/K2/K3) ----------------------------------
struct TopkArgs {
  const float* score;   // [B][n]
  int B, n, k;
  float thr;            // keep score > thr; pass -inf for plain top-k
  int32_t* idx;         // [B][k] flat cell indices, score desc / index asc on ties; -1 padded
  float* val;           // [B][k] scores (0 padded), may be nullptr
  int32_t* count;       // [B]
};
int launch_topk(const TopkArgs& a, hipStream_t s);

struct GatherArgs {     // gather coords / descriptors of selected cells into [B][k][2] / [B][k][C]
  const float* coord; const float* desc; const int32_t* idx;
  float* pts; float* dsel; int B, C, n, k;
};
int launch_gather(const GatherArgs& a, hipStream_t s);

// ---- SegFormerAttentionModule pieces (modules/segformer.py:63-220) ---------------------------
struct LnArgs { const float* x; const float* g; const float* b; float* y; long npix; int C; };
int launch_channel_layernorm(const LnArgs& a, hipStream_t s);

struct DwArgs { const float* x; const float* w; const float* bias; float* y; int B, H, W, C; };   // w: [9][C]
int launch_dwconv3x3(const DwArgs& a, hipStream_t s);

// MixFeedForward's tail fused (mff_tail.hip): depthwise 3x3 + bias -> 1x1 (128 -> 128) + bias -> GELU -> 1x1 (128 -> 64) + bias [-> MaxPool2d(2,2)]
struct MffTailArgs {
  const float* h;                                       // net.0's output, NHWC [B][H][W][128]
  const float* wdw; const float* bdw;                   // depthwise weights [9][128], bias [128]
  const float* w1; const float* sc1; const float* sh1;  // net.1.net.1: split-fp16 pack (64-channel groups), scale (2^-e), bias
  const float* w3; const float* sc3; const float* sh3;  // net.3
  float* out;                                           // [B][H][W][64], or pooled [B][H/2][W/2][64]
  int B, H, W, pool;
};
int launch_mff_tail(const MffTailArgs& a, hipStream_t s);

struct AttnArgs {
  const float* q;      // [B][S][C]   (to_q output, NHWC)
  const float* kv;     // [B][T][2C]  (to_kv output: k = channels [0,C), v = [C,2C))
  float* out;          // [B][S][C]
  int B, S, T, C, heads;
  float scale;         // (C/heads)^-0.5
  // row strides / channel offsets in floats; 0 = the dense defaults above (q_stride C, kv_stride 2C, k_off 0,
  // v_off C, out_stride C).  The LightGlue blocks read q, k, v as slices of one [q|k|v] or [qk|v] row.
  int q_stride = 0, kv_stride = 0, k_off = 0, v_off = 0, out_stride = 0;
  int prec = 0;        // 1: split-fp16 operands on v_mfma_f32_32x32x16_f16 (head dim <= 16), 0: exact fp32 MFMA
  const int32_t* tcount = nullptr;   // [B] keys that exist in batch item b's key / value sequence (the rest of its T rows is padding), null: all T
  int kv_bshift = 0;   // keys / values of batch item b come from item (b + kv_bshift) % B (LightGlue cross attention
                       // of both directions in one launch: items [0,B/2) are image 0, [B/2,B) image 1)
};
int launch_attention(const AttnArgs& a, hipStream_t s);

// ---- LightGlue matcher (lightglue/lightglue.py; kernels in lightglue.hip) -----------------------
struct LgPosArgs {
  const float* k0; const float* k1;         // keypoints [B][M][2] / [B][N][2], pixels (x, y)
  const float* size0; const float* size1;   // image size [B][2] (w, h) or null: 1 + max - min of the keypoints
  const float* wr;                          // posenc.Wr.weight [hd/2][2]
  float* cs;                                // [B*M + B*N][hd]: cos(hd/2) | sin(hd/2) per token
  int B, M, N, hd;
};
int launch_lg_posenc(const LgPosArgs& a, hipStream_t s);

enum LgEpi { LG_EPI_NONE = 0, LG_EPI_ROTARY = 1, LG_EPI_LNGELU = 2, LG_EPI_RESID = 3 };
struct LgLinArgs {
  const float* x0; const float* x1;         // input = [x0 row (k0 wide) | x1 row (k1 wide)]; x1 unused when k1 == 0
  int k0, k1, xs0, xs1;                     // widths and row strides (floats)
  const float* w;                           // W^T packed [K][nout] (nout padded to a multiple of 32)
  const float* bias;                        // [nout] or null
  float* out; int os, oo;                   // output row stride / column offset
  int rows, nout, nvalid;                   // nvalid <= nout columns are stored
  int epi;
  const float* cs; int hd, rot_cols;        // ROTARY: per-row cos|sin, head dim, leading columns that rotate
  const float* ln_g; const float* ln_b;     // LNGELU: LayerNorm affine over the nout columns
  const float* res; int rs;                 // RESID: out = res + y
};
int launch_lg_linear(const LgLinArgs& a, hipStream_t s);

// fused tail of a Self/CrossBlock for D = 32: x += ffn(cat[x, out_proj(ctx)])  (lightglue.py:260-261 / :322-326)
struct LgTailArgs {
  float* x; const float* ctx;           // [rows][D] in place / attention context (null: projection only)
  // split-fp16 matrix-core images of W (lightglue_desc.cpp mfma_image()) and fp32 biases
  const void* io; const float* bo;       // out_proj / to_out  [D -> D]
  const void* i1; const float* b1;       // ffn.0              [2D -> 2D]
  const float* ln_g; const float* ln_b;  // ffn.1
  const void* i2; const float* b2;       // ffn.3              [2D -> D]
  int rows, D;
  // optional: the NEXT token-wise projection of the updated x in the same launch (the cross block's [to_qk | to_v], the
  // next layer's Wqkv with its rotary epilogue, or the final projection): out[row][0..nvalid) = x W^T + b
  const void* in = nullptr; const float* bn = nullptr;    // image [D -> nn] (nn = 64 or 96, padded), bias [nn]
  float* on = nullptr; int nn = 0, nos = 0, nvalid = 0;   // output, its row stride, columns stored
  const float* cs = nullptr; int hd = 0, rot_cols = 0;    // rotary: per-row cos | sin, head dim, leading columns that rotate
  // optional: fp32 W^T [D][nn] of the next projection.  Its LAST stored column (nvalid - 1) is then an fp32 dot product
  // instead of the split-fp16 one: the matchability logit, a sum that cancels and goes straight into log-sigmoid, where
  // the split product's 2^-22 |w| |x| is an ABSOLUTE error of the log assignment (6e-5 at descriptors of norm 4096)
  const float* wz = nullptr;
};
int launch_lg_tail(const LgTailArgs& a, hipStream_t s);

struct LgAssignArgs {
  const float* fz;                          // [B*M + B*N][fs]: final_proj(x) / D^0.25 in [0,D), matchability logit at D
  int fs, D, B, M, N;
  float* scores;                            // [B][M+1][N+1] log assignment (out)
  // scratch, per 64 x 64 tile of the inner block: [B][ceil(N/64)][M] for rows, [B][ceil(M/64)][N] for columns
  float* rp_m; float* rp_s; float* cp_m; float* cp_s;      // log-sum-exp partials of sim (maximum, sum of exp)
  float* rmax; int* rarg; float* cmax; int* carg;          // max / argmax partials of the final scores
  float th;                                 // filter_threshold
  const int32_t* cnt0 = nullptr; const int32_t* cnt1 = nullptr;   // [B] keypoints that exist in each set (rows past them are padding), null: M / N
  int64_t* matches0; int64_t* matches1; float* mscores0; float* mscores1;
  // point pruning: rows are survivors; row e of set 0 is original keypoint ind0[b][e] (ind1 alike).  Matches and scores
  // are scattered to the original positions (the caller has filled the outputs with -1 / 0).  null: identity
  const int32_t* ind0 = nullptr; const int32_t* ind1 = nullptr;
};
int launch_lg_assign(const LgAssignArgs& a, hipStream_t s);

// point pruning between layers (lightglue.py:564-579): the rows of every sequence whose matchability score
// sigmoid(w . x + bias) exceeds thr move to the front of the sequence, in order; cnt becomes the survivors' number
struct LgPruneArgs {
  float* x; float* cs;                      // [B*M + B*N][D] descriptors / [..][hd] cos | sin, compacted in place
  const float* w;                           // log_assignment[i].matchability: weight [D], bias at w[D]
  int32_t* cnt;                             // [2B] rows that exist in each sequence ([set 0 | set 1]), updated
  int32_t* ind0; int32_t* ind1;             // [B][M] / [B][N] original index of row j (-1 past the count), compacted
  int64_t* prune0; int64_t* prune1;         // [B][M] / [B][N] by ORIGINAL index: += 1 for every survivor
  int B, M, N, D, hd;
  float thr;                                // 1 - width_confidence
};
// cnt <- n0 | n1 clamped to [0, M] / [0, N] (null: M / N), ind <- 0..cnt-1 then -1, prune <- 1 (padding rows 0)
int launch_lg_prune_init(const LgPruneArgs& a, const int32_t* n0, const int32_t* n1, hipStream_t s);
int launch_lg_prune(const LgPruneArgs& a, hipStream_t s);

// ---- vpr.hip: flat squared-L2 top-k over global descriptors (kp2d_vpr_*) ----------------------
struct VprSearchArgs {
  const unsigned char* dbp;        // packed database rows (kp2d_vpr_pack: 4 dim + 16 bytes each)
  const float* db;                 // the same rows in fp32 [ndb, dim]
  const unsigned char* qp;         // packed queries (scratch; set by launch_vpr_search)
  const float* q;                  // [nq, dim]
  const int64_t* limit;            // [nq] or null
  int64_t ndb;
  int dim, nq, k, fp32;
  unsigned long long* codes;       // per-slice lists (scratch; set by launch_vpr_search)
  const uint32_t* mask;            // [nq, ceil(ndb / 32)] row mask or null (kp2d_vpr_search_masked); not with limit
};
// (kmeans.hip and mining.hip search with these two; the scratch is kp2d_vpr_scratch_bytes' for the same arguments)
int launch_vpr_pack(const float* x, int64_t n, int dim, void* packed, hipStream_t s);
int launch_vpr_search(VprSearchArgs a, void* scratch, float* dist, int64_t* idx, hipStream_t s);

// ---- small layout / elementwise kernels -----------------------------------------------------
int launch_preprocess(const unsigned char* src, float* dst, int B, int Hs, int Ws, int H, int W, hipStream_t s);
int launch_l2norm_channels(float* x, long npix, int C, hipStream_t s);
int launch_nhwc_to_nchw(const float* in, float* out, int B, int C, int HW, int istride, int ioff, hipStream_t s);

}  // namespace kp2d
