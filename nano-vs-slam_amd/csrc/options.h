// Every tuning knob of the library in one place: the per-model options behind kp2d_set_option / kp2d_get_option with the
// KP2D_* variables that give them their initial values (kOptions), and the process-wide knobs of the kernel launchers
// (Tuning).  No knob is needed for correct results; they force kernel forms for A/B runs and parity tests.  README.md's
// table of knobs describes each variable for users; tests/test_options.py keeps its names in step with this file.
// No HIP here: options.cpp compiles with g++ (tests/test_options.py).
#pragma once
#include <climits>

namespace kp2d {

struct Options {
  int ws_min, wsm_grid, wsm_tr, wsm_min, mff_fused, stem_fusion, multi_launch, s16_all, s16_min, dbg, lane_prio, lanes,
      side_overlap;
  int lanes_default;   // what option "lanes" = 0 restores: KP2D_LANES, else the row's default
  Options();           // every field at its row's default
};

// How a variable's text becomes the option's initial value.  "Set" = present in the environment, "non-empty" = set to at
// least one character; v = atol(text), so text that is no number reads as 0.  Whatever a rule does not name is ignored.
enum class Env {
  none,        // the option has no variable
  off,         // first character '0': 0
  clamp,       // set, even empty: atoi(text) clamped to min .. max
  lanes,       // set, even empty: atoi(text) clamped to 1 .. max, into lanes and lanes_default
  zero_min,    // non-empty, v == 0: min
  count_min,   // non-empty, v == 0: min; v > 0: the smaller of v and max
  count,       // non-empty, v > 0: the smaller of v and max
  exact,       // non-empty, min <= v <= max: v
};

struct OptionRow {
  const char* key;   // kp2d_set_option / kp2d_get_option name; null: only the variable sets it
  const char* var;   // environment variable read by options_from_env; null: none
  int Options::*field;
  long def, min, max;
  Env env;
  const char* what;
};

// One row per option.  0 is "automatic" for the tile-form options (the policy is conv_policy.h).
constexpr OptionRow kOptions[] = {
    {"wsm_min_items", "KP2D_WSM", &Options::wsm_min, 0, -1, INT_MAX, Env::count_min,
     "least (16 x 32 pixel tile, 64-channel group) work items of a launch for the warp-specialised persistent form of the "
     "multi-chunk 3x3 layers (conv3x3_wsm.hip); 0 automatic: more than two rounds of the launch's workgroups; -1 never"},
    {"ws_min_tiles", nullptr, &Options::ws_min, 0, 0, INT_MAX, Env::none,
     "least 16 x 32 pixel tiles of a launch for the warp-specialised form of backbone.conv1b (conv3x3_f16x3_ws_kernel); "
     "0 automatic: 1024"},
    {"wsm_grid", "KP2D_WSM_GRID", &Options::wsm_grid, 0, 0, 65536, Env::count,
     "most workgroups per launch of the persistent forms (conv3x3_wsm.hip, conv3x3_s16.hip, conv1b's); 0 automatic: CUs / "
     "stream lanes, conv1b's form the whole chip"},
    {"wsm_transposed", "KP2D_WSM_TR", &Options::wsm_tr, 0, 0, 2, Env::exact,
     "conv3x3_wsm.hip's tiles walk the map transposed (tile rows = map columns, the weight pack's taps transposed to match; "
     "\"conv3x3_f16x3<wsm>t\" in the profile): 0 never, 1 always, 2 where the matrix-time model says it is cheaper (30 x 40 "
     "maps: 3 x 1 tiles instead of 2 x 2).  It sums the nine taps in another order, so results differ from every other tile "
     "form in the last bits, which is why it is opt-in: with it off, outputs are bit-identical whatever the batch size, lane "
     "count or tile form"},
    {"s16_min_items", "KP2D_S16", &Options::s16_min, 0, -1, INT_MAX, Env::zero_min,
     "conv3x3_s16.hip, split activations through the backbone's 32-channel stage: 0 automatic (three rounds of tiles per "
     "workgroup), N from N tiles, -1 never"},
    {"s16_all", "KP2D_S16ALL", &Options::s16_all, 1, 0, 1, Env::zero_min,
     "1: big grids keep every tensor the warp-specialised 3x3 layers read as the fp16 halves of the split (LDS-DMA staging, "
     "conv3x3_wsm.hip; bit-identical); 0: only inside the backbone's 32-channel stage"},
    {"multi_launch", "KP2D_MULTI", &Options::multi_launch, 1, 0, 1, Env::zero_min,
     "1: layers of different heads that wait for the same predecessor run as one launch on small grids; 0: one launch per layer"},
    {"mff_fused", "KP2D_MFF", &Options::mff_fused, 1, 0, 1, Env::off,
     "1: depthwise 3x3 -> 1x1 -> GELU -> 1x1 of the attention modules' MixFeedForward as one launch (mff_tail.hip); 0: three"},
    {"stem_fusion", "KP2D_STEM", &Options::stem_fusion, 1, 0, 2, Env::clamp,
     "the first layer.  1: split-fp16 products, computed inside conv1b's launch on big grids (conv3x3_f16.hip STEM) and by "
     "conv1a_mfma_kernel otherwise (the same bits); 2: the same arithmetic, never fused; 0: the exact-fp32 FMA kernels "
     "(conv1a_kernel / conv1a_u8_kernel)"},
    {"side_overlap", "KP2D_SIDE", &Options::side_overlap, 1, 0, 1, Env::off,
     "1: a plain single-frame forward runs NetVLAD on a model-owned side stream beside the segmentation head (never under "
     "stream capture; the stream is created on first use); 0: in line, and kp2d_set_option destroys the stream (a process "
     "that keeps several streams busy wants the hardware queue back)"},
    {"lanes", "KP2D_LANES", &Options::lanes, 2, 0, 8, Env::lanes,
     "stream lanes one forward splits its batch over: sub-batches run side by side on internal streams (a workspace sized "
     "before a change stays valid only for lane counts <= the one it was sized for).  Setting 0 restores the initial value.  "
     "A caller that keeps several batches in flight on streams of its own (pipeline.BatchStream, each with its own workspace) "
     "sets 1: the forwards then fill each other's launch tails, which two lanes of ONE forward (the same layer at the same "
     "time) cannot: 22.9k -> 23.4k frames/s at 64 x 240 x 320"},
    {nullptr, "KP2D_DBG", &Options::dbg, 0, INT_MIN, INT_MAX, Env::clamp,
     "ConvArgs::dbg: the phase switches of the timing-ablation build (-DKP2D_ABLATE)"},
    {nullptr, "KP2D_LANE_PRIORITY", &Options::lane_prio, 0, INT_MIN, INT_MAX, Env::clamp,
     "priority of the lane streams; -1: from the high-priority pool of hardware queues (an A/B knob, profiles/r5_hw_queues.txt)"},
};

// initial values: the variables `get` knows (kp2d_create passes getenv) over what `o` holds
void options_from_env(Options& o, const char* (*get)(const char*));
// KP2D_OK, or KP2D_ERR_ARG (unknown key, value outside the row's min .. max: `o` is unchanged; kp2d_last_error() says which)
int set_option(Options& o, const char* key, long value);
int get_option(const Options& o, const char* key, long* value);
const char* option_name(int index);   // the index-th key of kOptions; null past the last

// Process-wide knobs of the kernel launchers (no model handle there), read from the environment on first use.
constexpr int TOPK_SMALL_MAX = 256;   // post.hip: 256-thread workgroups up to here; beyond, 1024 threads hold one key each in the sort
struct Tuning {
  bool match_mfma;    // KP2D_MATCH_MFMA=0: the matcher always in its VALU form
  int topk_small;     // KP2D_TOPK_SMALL=n: top-k on 256-thread workgroups up to k = n
  bool gather_lds;    // KP2D_GATHER_LDS=0: keypoint gather always by direct reads
  int vlad_px;        // KP2D_VLAD_PX=n: pixels per NetVLAD partial-sum workgroup
  bool vlad_split;    // KP2D_VLAD_SPLIT=0: NetVLAD soft-assignment logits in exact fp32 also in the f16x3 mode
  long att_ksplit;    // KP2D_ATT_KSPLIT=n: key-split attention below n workgroups of the query-tiled grid
  int att_q;          // KP2D_ATT_Q=128: split attention with 128 queries per workgroup for every shape
  bool att_affine;    // KP2D_ATT_AFFINE=0: split attention on the plain (tiles, heads, frames) grid
  bool lg_fuse;       // KP2D_LG_FUSE=0: LightGlue block tails as separate linear launches
  bool lg_fuse_next;  // KP2D_LG_FUSE_NEXT=0: LightGlue projections as their own launches
  int lg_tail_nw;     // KP2D_LG_TAIL_NW=n: waves per workgroup of the LightGlue block tail (0: four)
  bool seg_ids_only;  // KP2D_SEG_IDS_ONLY=0: KP2D_FWD_NO_SEG_LOGITS is ignored, the class logits are always stored (plan.cpp)
};
Tuning tuning_from_env(const char* (*get)(const char*));
const Tuning& tuning();

}  // namespace kp2d
