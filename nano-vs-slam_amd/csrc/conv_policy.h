// Host-side policy of the split-fp16 3x3 convolutions (prec = 1, taps = 9): which tile form runs a layer, on how many
// workgroups, and what the plan (plan.cpp build()) may assume before it picks the activation layouts.  Every decision is
// made here once; the launchers in conv3x3_f16.hip, conv3x3_wsm.hip and conv3x3_s16.hip only launch what it chose.
// Plain C++: it takes the CU count and the stream-lane count as arguments and never asks the device
// (tests/test_conv_policy.py compiles it with g++).
#pragma once
#include "conv_args.h"

namespace kp2d {

// the persistent forms' tile, 16 rows x 32 columns (conv3x3_f16.hip <ws>, conv3x3_wsm.hip, conv3x3_s16.hip)
constexpr int PT_TH = 16, PT_TW = 32;
constexpr int M_MAXN = 320;           // most channels of a conv3x3_wsm.hip layer (scale / shift in LDS; 320 = the five heads' first layers as one)
// A "small grid": a launch of 16 x 16 tiles with fewer workgroups than this (a frame or two at a time).  Such layers take
// 32-channel groups and 8-row tiles (twice the workgroups, half as long), and the plan runs the level-by-level schedule and
// the heads' merged first layer.
constexpr long SMALL_GRID = 256;
constexpr long BUF_LIMIT = 0x7ffffff0L;   // byte offsets the kernels address through one buffer resource stay below this

inline long persistent_tiles(int B, int H, int W) { return (long)((W + PT_TW - 1) / PT_TW) * ((H + PT_TH - 1) / PT_TH) * B; }
inline bool small_grid(int B, int H, int W, int groups) { return (long)((W + 15) / 16) * ((H + 15) / 16) * B * groups < SMALL_GRID; }

// Most workgroups of a persistent launch.  A workgroup of these forms fills its CU's LDS, so launches of L stream lanes run
// side by side only on DISJOINT CUs: cap = CUs / L (a profiling forward runs one lane and takes the whole chip), or
// grid_opt (kp2d_set_option "wsm_grid"); a multiple of 8, contiguous runs per XCD.
inline int persistent_cap(int cus, int lanes, int grid_opt) {
  int cap = grid_opt > 0 ? grid_opt : cus / (lanes > 1 ? lanes : 1);
  if (cap > cus) cap = cus;
  return cap & ~7;
}

// Workgroups of a launch of `nitems` work items on the <wsm> / <s16> forms, 0: the form does not apply.  It needs min_items
// items (<= 0: automatic, more than `full_rounds` rounds of cap: profiles/r4_layers_wsm_vs_general.txt).  Whole rounds:
// grid = ceil(items / ceil(items / cap)) rounded up to a multiple of 8 — 192 items on a cap of 128 run as 2 rounds on 96
// workgroups, not 1.5 rounds on 128 (profiles/r4_sweep_first_policy.jsonl).
inline int persistent_grid(long nitems, int cus, int lanes, int grid_opt, long min_items, int full_rounds = 2) {
  const int cap = persistent_cap(cus, lanes, grid_opt);
  if (cap < 8) return 0;
  const long need = min_items > 0 ? min_items : (long)full_rounds * cap + 1;
  if (nitems < need || nitems >= (1L << 30)) return 0;
  const long rounds = (nitems + cap - 1) / cap;
  long grid = ((nitems + rounds - 1) / rounds + 7) & ~7L;
  if (grid > cap) grid = cap;
  if (grid > nitems) grid = nitems & ~7L;
  return grid < 8 ? 0 : (int)grid;
}

// ---- eligibility --------------------------------------------------------------------------------------------------------
// conv3x3_wsm.hip with N-channel work items (64: 64-channel groups, 32: the 32-channel layers)
inline bool wsm_eligible(const ConvArgs& a, int N) {
  if (a.taps != 9 || a.prec != 1 || a.ng32 || a.npad % N != 0 || a.npad > M_MAXN) return false;
  const bool s16out = a.store == ST_S16P || a.store == ST_S16P_SHUFFLE || a.store == ST_MIX16;
  if (a.store != ST_NHWC && a.store != ST_SHUFFLE && a.store != ST_NHWC_BOTH && a.store != ST_NHWC_POOL && !s16out) return false;
  if (a.act > ACT_RELU) return false;
  if (((a.in0.c | a.cin) & 15) != 0 || a.cin < 32) return false;      // whole 16-channel chunks, never straddling the sources
  if (a.cout & 3) return false;
  if (a.store == ST_SHUFFLE && ((a.cout >> 2) & 15)) return false;      // a 16-channel N-tile is one sub-pixel
  if (a.W < 32) return false;
  const long ps = a.in0.ps > a.in1.ps ? a.in0.ps : a.in1.ps;
  if ((long)a.H * a.W * ps * 4 >= BUF_LIMIT) return false;
  if (a.in0.fmt == 1) {
    // S16P sources: whole chunks of dense tensors (a view is a run of chunks: ps = the tensor's channels)
    if (N != 64 || (a.in1.c > 0 && a.in1.fmt != 1) || ((a.in0.o | a.in1.o) & 15)) return false;
    if (a.in0.bs != (long)a.H * a.W * a.in0.ps || (a.in1.c > 0 && a.in1.bs != (long)a.H * a.W * a.in1.ps)) return false;
  } else {
    if (a.in1.c > 0 && a.in1.fmt == 1) return false;
    if (a.in0.rs != (long)a.W * a.in0.ps || (a.in1.c > 0 && a.in1.rs != (long)a.W * a.in1.ps)) return false;
  }
  if (s16out) {
    // whole chunks out, 64-channel items, a pair of N-tiles = 32 channels of one sub-pixel
    if (N != 64 || (a.cout & 15)) return false;
    if (a.store == ST_S16P_SHUFFLE && (((a.cout >> 2) & 31) || (a.os0 & 15) || (a.oo0 & 15))) return false;
    if (a.store == ST_S16P && ((a.os0 & 15) || (a.oo0 & 15))) return false;
    if (a.store == ST_MIX16 && ((a.nsplit & 63) || a.nsplit <= 0 || a.nsplit >= a.cout || (a.os1 & 15) || (a.oo1 & 15) || (a.os0 & 3))) return false;
  }
  const long up = (a.store == ST_SHUFFLE || a.store == ST_S16P_SHUFFLE) ? 4 : 1;
  if ((long)a.H * a.W * up * a.os0 * 4 >= BUF_LIMIT) return false;
  if (a.store == ST_MIX16 && (long)a.H * a.W * a.os1 * 4 >= BUF_LIMIT) return false;
  return true;
}

// conv3x3_s16.hip: 32-input-channel layers whose input is an S16P tensor, and the planar logits (or only their argmax)
// behind a 64-channel one
inline bool s16_eligible(const ConvArgs& a) {
  if (a.taps != 9 || a.prec != 1 || a.in0.fmt != 1 || a.in1.c != 0 || a.in0.c != a.cin || a.in0.o != 0) return false;
  if (a.store == ST_IDS) {
    // class ids only (convs.8 under KP2D_FWD_NO_SEG_LOGITS): one 32-channel group of plain logits, a lane stores one pixel's id
    if (a.cin != 64 || a.npad != 32 || a.cout < 1 || a.act != ACT_NONE || a.nsplit != a.cout || a.W < 32 || !a.ids_out) return false;
    if (a.in0.bs != (long)a.H * a.W * a.cin || (long)a.H * a.W * a.cin * 4 >= BUF_LIMIT) return false;
    return true;
  }
  if (a.store == ST_NCHW) {
    // planar logits behind a 64-channel S16P tensor (confBb, convs.8): one 32-channel group, every channel into out0
    if (a.cin != 64 || a.npad != 32 || a.act != ACT_NONE || a.nsplit != a.cout || a.W < 32 || (a.W & 3) || a.ids_out) return false;
    if (a.in0.bs != (long)a.H * a.W * a.cin || (long)a.H * a.W * a.cin * 4 >= BUF_LIMIT) return false;
    return true;
  }
  if (a.cin != 32) return false;
  if (a.act > ACT_RELU || a.W < 32 || (a.cout & 15)) return false;
  if (a.store == ST_S16P) { if (a.npad != 32) return false; }
  else if (a.store == ST_NHWC || a.store == ST_NHWC_POOL || a.store == ST_NHWC_BOTH || a.store == ST_S16P_BOTH) { if (a.npad != 64) return false; }
  else return false;
  if ((a.store == ST_NHWC_POOL || a.store == ST_NHWC_BOTH || a.store == ST_S16P_BOTH) && ((a.H | a.W) & 1)) return false;
  if (a.in0.bs != (long)a.H * a.W * a.cin) return false;                      // dense S16P frames
  if ((long)a.H * a.W * a.cin * 4 >= BUF_LIMIT) return false;
  const long os = (a.store == ST_S16P || a.store == ST_S16P_BOTH) ? a.cout : (a.os0 > a.os1 ? a.os0 : a.os1);
  if ((long)a.H * a.W * os * 4 >= BUF_LIMIT) return false;
  return true;
}

// the map side of conv1b's warp-specialised form <ws> (conv3x3_f16.hip), ws_min: least tiles (0: 1024).  The plan asks it
// before it keeps conv1b's output split or computes conv1a inside conv1b's launch
inline bool ws_map_ok(int B, int H, int W, int ws_min) {
  return !(H & 1) && !(W & 1) && W >= 32 && persistent_tiles(B, H, W) >= (ws_min > 0 ? ws_min : 1024) && (long)B * H * W * 16 * 4 < BUF_LIMIT;
}
// ... and the layer side: 16 -> at most 32 channels (one 32-channel group), max-pooled (the store is the caller's).  The fp32
// output masks channels past cout (the N configurations' 16 -> 24 conv1b); the S16P output takes whole chunks of a dense
// 16-channel source
inline bool ws_eligible(const ConvArgs& a, bool s16out) {
  if (!(a.cin == 16 && a.in0.c == 16 && a.in1.c == 0 && a.npad == 32 && a.act <= ACT_RELU && ws_map_ok(a.B, a.H, a.W, a.ws_min))) return false;
  if (!s16out) return (long)a.B * a.in0.bs * 4 < BUF_LIMIT;
  return a.cout == 32 && a.in0.rs == (long)a.W * a.in0.ps && a.in0.ps == 16 && a.in0.o == 0;
}

// Matrix time of one map walked as Ht x Wt in tile space, in units of one wave's four M-tiles: a multiplying wave (wr, ph)
// works when its 4 rows x 16 columns touch the map, SIMD s holds waves s and s + 4 = (wr s, ph 0) and (wr (s + 2) & 3, ph 1),
// and a step lasts as long as its busiest SIMD.  (What the model leaves out — staging, the barrier — is the same per step, and
// the cheaper walk never has more steps.)
inline int wsm_walk_cost(int Ht, int Wt) {
  int cost = 0;
  for (int y0 = 0; y0 < Ht; y0 += PT_TH)
    for (int x0 = 0; x0 < Wt; x0 += PT_TW) {
      int worst = 0;
      for (int sd = 0; sd < 4; ++sd) {
        const int b0 = (y0 + 4 * sd < Ht) ? 1 : 0;                                         // ph 0: its 16 columns start at x0
        const int b1 = (y0 + 4 * ((sd + 2) & 3) < Ht && x0 + 16 < Wt) ? 1 : 0;
        worst = b0 + b1 > worst ? b0 + b1 : worst;
      }
      cost += worst;
    }
  return cost;
}

// ---- what the plan asks before it fixes layouts -------------------------------------------------------------------------
// would the automatic <wsm> policy take a layer of `groups` 64-channel groups on a B x H x W map (full_rounds: 2 for the
// register-staging form; 1 for the S16P-input form, whose start-up is one LDS-DMA round trip, profiles/r5_ab_s16_all.txt)
inline bool wsm_would_run(int B, int H, int W, int groups, int cus, int lanes, int wsm_min, int grid_opt, int full_rounds) {
  return wsm_min >= 0 && W >= 32 && persistent_grid(persistent_tiles(B, H, W) * groups, cus, lanes, grid_opt, wsm_min, full_rounds) > 0;
}
// would <s16> run conv2a .. conv3b on a B x H x W map
inline bool s16_would_run(int B, int H, int W, int cus, int lanes, int s16_min, int grid_opt) {
  return s16_min >= 0 && W >= 32 && !((H | W) & 1) && persistent_grid(persistent_tiles(B, H, W), cus, lanes, grid_opt, s16_min) > 0;
}
// Small grids: a 64-channel-group launch would leave most CUs idle and each of its few workgroups is a long serial chain;
// 32-channel groups (ConvArgs::ng32) double the workgroups and halve their length.  Not where wsm_min_items forces <wsm>
// (the parity tests), which keeps its 64-channel groups; S16P layers (the caller's test) keep them too.
inline bool use_ng32(int B, int H, int W, int npad, int wsm_min) {
  return npad >= 64 && !(wsm_min > 0 && persistent_tiles(B, H, W) * (npad / 64) >= wsm_min) && small_grid(B, H, W, npad / 64);
}

// ---- the choice of tile form --------------------------------------------------------------------------------------------
// the persistent forms <s16>, <wsm> (64- / 32-channel items), <ws> (conv1b), then the general conv3x3_f16x3_kernel<NH, NP, TH(, FLAT32)>
enum ConvForm : int { FORM_S16, FORM_WSM, FORM_WSM32, FORM_WS, FORM_F_2_1_8, FORM_F_2_1_16, FORM_F_1_2_16, FORM_F_1_1_8_FLAT32, FORM_F_1_1_8, FORM_F_1_1_16 };
struct ConvChoice {
  int form = FORM_F_1_1_16;
  const char* variant = "";   // conv3x3_last_variant(): what the engine's profile records
  int grid = 0;               // persistent forms: workgroups (0: the general forms, one per tile)
  int walk = 0;               // <wsm>: 1 = tiles walk the map transposed (tile rows = map columns; the transposed-tap pack)
  int tiles_x = 0, tiles_y = 0;
  long ntiles = 0, nitems = 0;
  void tile(int B, int H, int W) {      // the persistent forms' 16 x 32 tiles over a B x H x W map
    tiles_x = (W + PT_TW - 1) / PT_TW; tiles_y = (H + PT_TH - 1) / PT_TH; ntiles = nitems = (long)tiles_x * tiles_y * B;
  }
};

// <wsm>.  The transposed walk (ConvArgs::wsm_tr: 0 never, 1 always, 2 where the model above says it is cheaper) is opt-in:
// it sums the nine taps in another order than every other form.  Automatic use (wsm_min 0) needs 64-channel items and at
// least four input chunks (conv3b: 0.165 against 0.157 ms); 32-channel items are not faster (profiles/r4_ab_wsm32.txt).  A
// forced layer (wsm_force: the plan fixed S16P layouts on this form) skips the item-count policy; -1006 if it cannot run.
inline int choose_wsm(const ConvArgs& a, int cus, int n_item, ConvChoice& out) {
  const bool forced = a.wsm_force != 0;
  const int no = forced ? -1006 : -1000;
  if (!forced && (a.wsm_min < 0 || (a.wsm_min == 0 && (n_item == 32 || a.cin < 64)))) return -1000;
  if (!wsm_eligible(a, n_item)) return no;
  ConvChoice c;
  const bool s16_any = a.in0.fmt == 1 || a.store == ST_S16P || a.store == ST_S16P_SHUFFLE || a.store == ST_MIX16;      // S16P rows are map rows
  c.walk = n_item == 64 && a.w_tr && a.wsm_tr > 0 && !s16_any && a.H >= 16 &&
           (a.wsm_tr == 1 || wsm_walk_cost(a.W, a.H) < wsm_walk_cost(a.H, a.W));
  c.tile(a.B, c.walk ? a.W : a.H, c.walk ? a.H : a.W);
  c.nitems = c.ntiles * (a.npad / n_item);
  c.grid = persistent_grid(c.nitems, cus, a.wsm_lanes, a.wsm_grid, forced ? 1 : a.wsm_min);
  if (c.grid == 0) return no;
  c.form = n_item == 64 ? FORM_WSM : FORM_WSM32;
  c.variant = n_item == 32 ? "<wsm32>" : c.walk ? "<wsm>t" :
              a.in0.fmt == 1 ? (a.store != ST_NHWC && a.store != ST_NHWC_POOL ? "<wsm>s16io" : "<wsm>s16in") : (s16_any ? "<wsm>s16out" : "<wsm>");
  out = c;
  return 0;
}

inline int choose_s16(const ConvArgs& a, int cus, ConvChoice& c) {
  if (!s16_eligible(a)) return -1006;
  c.tile(a.B, a.H, a.W);
  c.grid = persistent_grid(c.nitems, cus, a.wsm_lanes, a.wsm_grid, a.s16_min);
  if (c.grid == 0) return -1006;
  c.form = FORM_S16;
  // (ST_IDS: the launcher reports its variant itself, conv3x3_s16.hip.  The literals of this file are the forms
  // tests/test_gpu_layer_fp64.py must reach with a plain forward; that one runs only under KP2D_FWD_NO_SEG_LOGITS and is
  // checked bit for bit against the logits-writing forms by tests/test_gpu_seg_ids_only.py)
  c.variant = a.store == ST_NCHW ? "<s16>planar" : "<s16>";
  return 0;
}

// <ws>: one workgroup per tile up to the whole chip (its launches of two lanes share the CUs, unlike <wsm> / <s16>'s)
inline int choose_ws(const ConvArgs& a, int cus, bool s16out, ConvChoice& c) {
  c.tile(a.B, a.H, a.W);
  const int cap = persistent_cap(cus, 1, a.wsm_grid);
  c.grid = (int)(c.ntiles < cap ? c.ntiles : (cap > 8 ? cap : 8));
  c.form = FORM_WS;
  c.variant = s16out ? (a.stem_x ? "<ws>stem+s16" : "<ws>s16") : (a.stem_x ? "<ws>stem" : "<ws>");
  return 0;
}

// The tile form of launch_conv3x3_f16x3: 0 and `c` filled, or -1000 (not a layer of these kernels), -1002 (too large),
// -1004 (a source that is not dense rows), -1006 (a plan bug: an S16P tensor no form can take).
// S16P tensors (conv_args.h) are read by conv3x3_s16.hip (32 input channels) and by conv3x3_wsm.hip's IN16 form, and written
// by both and by <ws>; no other kernel takes the layout.
inline int choose_conv3x3_f16x3(const ConvArgs& a, int cus, ConvChoice& c) {
  c = ConvChoice{};
  auto general = [&c](int form, const char* variant) { c.form = form; c.variant = variant; return 0; };
  if (a.taps != 9 || a.prec != 1) return -1000;
  if (a.in0.fmt == 1 && a.in1.c == 0 && (a.cin == 32 || a.store == ST_NCHW || a.store == ST_IDS)) return choose_s16(a, cus, c);
  if (a.store == ST_IDS) return -1006;      // (the plan picks it only behind an S16P tensor)
  if (a.wsm_force) return choose_wsm(a, cus, 64, c);
  if (a.in0.fmt == 1 || a.in1.fmt == 1 || a.store == ST_S16P || a.store == ST_S16P_BOTH || a.store == ST_S16P_SHUFFLE || a.store == ST_MIX16) return -1006;
  if (a.store == ST_S16P_POOL) return ws_eligible(a, true) ? choose_ws(a, cus, true, c) : -1006;
  // the staging addresses a source pixel as (y * W + x) * pixel stride
  if (a.in0.rs != (long)a.W * a.in0.ps || (a.in1.c > 0 && a.in1.rs != (long)a.W * a.in1.ps)) return -1004;
  if ((long)a.H * a.W * (a.in0.ps > a.in1.ps ? a.in0.ps : a.in1.ps) * 4 >= BUF_LIMIT) return -1002;
  if (a.npad != 32 && a.npad % 64 != 0) return -1000;
  const int rag = a.H & 15;
  if (!(a.npad == 32 || a.ng32)) {
    // multi-chunk layers with 64-channel groups on grids that fill the chip: the warp-specialised persistent form
    if (choose_wsm(a, cus, 64, c) == 0) return 0;
    // map heights that leave the last 16-row tile row at most half full (120 = 7.5 x 16): 8 x 32 tiles, no ragged row
    if (rag >= 1 && rag <= 8 && a.W >= 32 && (long)a.H * a.W < (1L << 20)) return general(FORM_F_2_1_8, "<2,1,8>");
    return general(FORM_F_2_1_16, "<2,1,16>");
  }
  // single-chunk, max-pooled, 32 channels (conv1b) on grids that fill the chip several times: warp-specialised persistent form
  if (a.store == ST_NHWC_POOL && ws_eligible(a, false)) return choose_ws(a, cus, false, c);
  // 32-channel layers on grids that fill the chip several times: the warp-specialised persistent form with 32-channel items
  if (a.npad == 32 && !a.ng32 && choose_wsm(a, cus, 32, c) == 0) return 0;
  // 32-channel layers on grids that fill the chip anyway: 16 x 32 pixel tiles (one weight slab per 512 pixels, 16 waves per
  // CU).  (Planar API outputs keep the 16-pixel tiles: measured 0.148 -> 0.151 ms on desc_head.confBb with the wide ones.)
  const long wide_tiles = (long)((a.W + 31) / 32) * ((a.H + 15) / 16) * a.B * (a.npad / 32);
  if (a.store != ST_NCHW && a.W >= 32 && wide_tiles >= 1024 && (long)a.H * a.W < (1L << 20)) return general(FORM_F_1_2_16, "<1,2,16>");
  // planar outputs on maps with a half-empty last 16-row tile row (confBb / the class map at 120 rows): 8 x 32 tiles
  if (a.store == ST_NCHW && rag >= 1 && rag <= 8 && a.W >= 32 && !(a.W & 3) && (long)a.H * a.W < (1L << 20) &&
      (long)((a.W + 31) / 32) * ((a.H + 7) / 8) * a.B * (a.npad / 32) >= 512)
    return general(FORM_F_1_1_8_FLAT32, "<1,1,8,flat32>");
  // single frames (the grid of 16 x 16 tiles would leave most CUs idle): 8-row tiles, twice the workgroups, half as long
  if (small_grid(a.B, a.H, a.W, a.npad / 32)) return general(FORM_F_1_1_8, "<1,1,8>");
  return general(FORM_F_1_1_16, "<1,1,16>");
}

}  // namespace kp2d
