"""CPU unit test of nano-vs-slam_amd/csrc/conv_policy.h: which tile form runs each split-fp16 3x3 layer, on how many
workgroups, and what the plan may assume before it fixes the activation layouts.  The header is plain C++ and is compiled
here with g++.  The expected table was derived from the launchers and build() as they were before the policy moved into
the header (one decision per place), so it pins the engine's forms: a change here is a change of the schedule."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The plan of KP2DTiny-S (backbone conv1b .. conv4b and the heads' merged first layer) as plan.cpp build() / Plan::conv_args()
# lay it out for one sub-batch of B frames on `lanes` stream lanes, each layer's choice printed as "layer variant grid".
# The plan side is a copy, not build() itself: main() mirrors build()'s `stem`, `s16`, `small_heads` / `big_wsm` / `merged` and
# `s16_all` conditions (default options, KP2DTiny-S, float frames) and layer() mirrors Plan::conv_args()'s `wsm_force` and ng32
# rules.  A change to those in plan.cpp must be made here too.
SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "conv_policy.h"
using namespace kp2d;
static const int CUS = 256;
static ConvSrc src(int c, int H, int W, int fmt) {
  ConvSrc s{};
  s.p = nullptr; s.c = c; s.o = 0; s.ps = c; s.rs = (long)W * c; s.bs = (long)H * W * c; s.fmt = fmt;
  return s;
}
static const float dummy = 0.f;
static void layer(const char* name, int B, int H, int W, int lanes, int cin, int cout, int npad, int in_fmt, int store, bool stem,
                  int os0 = 0, int os1 = 0, int nsplit = 0) {
  ConvArgs a{};
  a.in0 = src(cin, H, W, in_fmt); a.in1 = src(0, H, W, 0); a.in1.c = 0;
  a.taps = 9; a.prec = 1; a.w = &dummy;
  a.B = B; a.H = H; a.W = W; a.cin = cin; a.cout = cout; a.npad = npad;
  a.act = ACT_LEAKY; a.store = store; a.nsplit = nsplit;
  a.os0 = os0 ? os0 : cout; a.os1 = os1 ? os1 : cout;
  a.wsm_lanes = lanes;
  if (stem) a.stem_x = &dummy;
  a.wsm_force = ((in_fmt == 1 && cin != 32) || store == ST_S16P_SHUFFLE || store == ST_MIX16 || (store == ST_S16P && npad >= 64)) ? 1 : 0;
  if (in_fmt == 0 && !a.wsm_force && use_ng32(B, H, W, npad, 0)) a.ng32 = 1;
  ConvChoice c;
  const int e = choose_conv3x3_f16x3(a, CUS, c);
  if (e) std::printf("%s ERR%d 0\n", name, e);
  else std::printf("%s %s %d\n", name, c.variant, c.grid);
}
int main(int argc, char** argv) {
  const int B = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]), lanes = atoi(argv[4]);
  const bool stem = ws_map_ok(B, H, W, 0);
  const bool s16 = stem && s16_would_run(B, H / 2, W / 2, CUS, lanes, 0, 0);
  const int Hc = H >> 2, Wc = W >> 2, Hq = H / 4, Wq = W / 4;
  const bool merged = small_grid(B, Hc, Wc, 1) || (long)Hc * Wc >= 60 * 80 ||
                      ((long)Hc * Wc >= 30 * 40 && wsm_would_run(B, Hc, Wc, 5, CUS, lanes, 0, 0, 2));
  const bool all = s16 && merged && Wq / 2 >= 32 && persistent_tiles(B, Hq / 2, Wq / 2) * 2 >= 8 &&
                   wsm_would_run(B, Hq, Wq, 1, CUS, lanes, 0, 0, 1);
  const int s = s16 ? 1 : 0, f = all ? 1 : 0;
  layer("conv1b", B, H, W, lanes, 16, 32, 32, 0, s16 ? ST_S16P_POOL : ST_NHWC_POOL, stem);
  layer("conv2a", B, H / 2, W / 2, lanes, 32, 32, 32, s, s16 ? ST_S16P : ST_NHWC, false);
  layer("conv2b", B, H / 2, W / 2, lanes, 32, 32, 32, s, s16 ? ST_S16P : ST_NHWC, false);
  layer("conv3a", B, H / 2, W / 2, lanes, 32, 32, 32, s, s16 ? ST_S16P : ST_NHWC, false);
  layer("conv3b", B, H / 2, W / 2, lanes, 32, 64, 64, s, all ? ST_S16P_BOTH : ST_NHWC_BOTH, false);
  layer("conv4a", B, Hq, Wq, lanes, 64, 64, 64, f, all ? ST_S16P : ST_NHWC, false);
  layer("conv4b", B, Hq, Wq, lanes, 64, 64, 64, f, all ? ST_S16P : ST_NHWC, false);
  if (merged) layer("heads.first", B, Hc, Wc, lanes, 64, 320, 320, f, all ? ST_MIX16 : ST_NHWC, false, all ? 64 : 0, all ? 256 : 0, all ? 64 : 0);
  return 0;
}
"""

# Boundaries and overrides, one CHECK each.
SRC_EDGES = r"""
#include <cstdio>
#include "conv_policy.h"
using namespace kp2d;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
static const float dummy = 0.f;
static ConvArgs conv(int B, int H, int W, int cin, int cout, int npad, int store) {     // dense fp32 NHWC in and out
  ConvArgs a{};
  a.in0.c = cin; a.in0.ps = cin; a.in0.rs = (long)W * cin; a.in0.bs = (long)H * W * cin;
  a.taps = 9; a.prec = 1; a.w = &dummy; a.B = B; a.H = H; a.W = W; a.cin = cin; a.cout = cout; a.npad = npad;
  a.act = ACT_LEAKY; a.store = store; a.os0 = cout; a.os1 = cout; a.wsm_lanes = 1;
  return a;
}
int main() {
  ConvChoice c;
  // <ws> (conv1b): 1024 tiles of 16 x 32 pixels and more; 1023 is the general wide form
  ConvArgs a = conv(1, 16 * 31, 32 * 33, 16, 32, 32, ST_NHWC_POOL);      // 31 x 33 = 1023 tiles
  CHECK(persistent_tiles(1, a.H, a.W) == 1023);
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form != FORM_WS);
  a = conv(1, 16 * 32, 32 * 32, 16, 32, 32, ST_NHWC_POOL);               // 1024
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form == FORM_WS && c.grid == 256 && c.ntiles == 1024);
  a.ws_min = 1 << 30;                                                     // ws_min_tiles: never
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form != FORM_WS);
  a.ws_min = 0; a.wsm_grid = 100;                                         // wsm_grid caps <ws> too (a multiple of 8)
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form == FORM_WS && c.grid == 96);
  // the N configurations' conv1b, 16 -> 24 channels (npad 32): <ws> with fp32 NHWC output; its S16P output needs 32 channels
  a = conv(8, 240, 320, 16, 24, 32, ST_NHWC_POOL);                       // 8 x 150 = 1200 tiles
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form == FORM_WS && c.grid == 256 && std::string(c.variant) == "<ws>");
  a.stem_x = &dummy;
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form == FORM_WS && std::string(c.variant) == "<ws>stem");
  a.stem_x = nullptr; a.store = ST_S16P_POOL;
  CHECK(choose_conv3x3_f16x3(a, 256, c) == -1006);
  // whole rounds: 192 items on a cap of 128 run as 2 rounds on 96 workgroups
  CHECK(persistent_grid(192, 256, 2, 0, 1) == 96);
  CHECK(persistent_grid(192, 128, 1, 0, 1) == 96);
  CHECK(persistent_grid(192, 256, 1, 128, 1) == 96);
  CHECK(persistent_cap(256, 3, 0) == 80 && persistent_cap(256, 1, 1000) == 256 && persistent_cap(256, 1, 7) == 0);
  // <wsm> automatic: more than two rounds, i.e. 2 * cap + 1 items (cap 128 on two lanes): 64-channel items of a 64-input layer
  a = conv(1, 16, 32, 64, 64, 64, ST_NHWC);                               // one tile per frame, one group: items = frames
  a.wsm_lanes = 2;
  a.B = 256; CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form != FORM_WSM);
  a.B = 257; CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form == FORM_WSM && c.grid == 88 && c.nitems == 257);
  CHECK(std::string(c.variant) == "<wsm>");
  a.wsm_lanes = 1;
  a.B = 512; CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form != FORM_WSM);
  a.B = 513; CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form == FORM_WSM && c.grid == 176);
  CHECK(wsm_would_run(513, 16, 32, 1, 256, 1, 0, 0, 2) && !wsm_would_run(512, 16, 32, 1, 256, 1, 0, 0, 2));
  CHECK(wsm_would_run(257, 16, 32, 1, 256, 1, 0, 0, 1) && !wsm_would_run(256, 16, 32, 1, 256, 1, 0, 0, 1));
  // wsm_grid: the cap
  a.B = 513; a.wsm_grid = 64;
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form == FORM_WSM && c.grid == 64);
  a.wsm_grid = 0;
  // wsm_min_items: -1 never, n from n items (and the 32-input-channel layers too)
  a.B = 600; a.wsm_min = -1;
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form != FORM_WSM);
  CHECK(!wsm_would_run(600, 16, 32, 1, 256, 1, -1, 0, 2));
  a.B = 8; a.wsm_min = 8;
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form == FORM_WSM && c.grid == 8);
  a.B = 7;
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form != FORM_WSM);
  ConvArgs b = conv(64, 128, 128, 32, 32, 32, ST_NHWC);
  b.wsm_min = 8;
  CHECK(choose_conv3x3_f16x3(b, 256, c) == 0 && c.form == FORM_WSM32 && std::string(c.variant) == "<wsm32>");
  b.wsm_min = 0;
  CHECK(choose_conv3x3_f16x3(b, 256, c) == 0 && c.form == FORM_F_1_2_16);
  // the transposed walk: asked for (1 always, 2 where cheaper), with the transposed pack, never on S16P tensors
  a = conv(64, 64, 96, 64, 64, 64, ST_NHWC);
  a.w_tr = &dummy; a.wsm_tr = 1;
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.walk == 1 && std::string(c.variant) == "<wsm>t" && c.tiles_x == 2 && c.tiles_y == 6);
  a.wsm_tr = 0;
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.walk == 0 && std::string(c.variant) == "<wsm>");
  CHECK(wsm_walk_cost(30, 40) > 0);
  // s16_min_items: -1 never; automatic: more than two rounds of 16 x 32 tiles
  CHECK(!s16_would_run(64, 120, 160, 256, 1, -1, 0));
  CHECK(s16_would_run(13, 120, 160, 256, 1, 0, 0) && !s16_would_run(12, 120, 160, 256, 1, 0, 0));      // 40 tiles per frame: 520 / 480
  CHECK(s16_would_run(1, 120, 160, 256, 1, 1, 0));
  // a forced <wsm> layer (S16P in) that the form cannot take: the plan bug code
  a = conv(4, 60, 20, 64, 64, 64, ST_S16P);                               // W < 32
  a.in0.fmt = 1; a.wsm_force = 1;
  CHECK(choose_conv3x3_f16x3(a, 256, c) == -1006);
  a.W = 80; a.in0.rs = 80 * 64; a.in0.bs = 60L * 80 * 64;
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form == FORM_WSM && std::string(c.variant) == "<wsm>s16io");
  a.wsm_min = -1;                                                          // (a forced layer has no item-count policy)
  CHECK(choose_conv3x3_f16x3(a, 256, c) == 0 && c.form == FORM_WSM);
  // the other codes: S16P nobody reads, a strided source, a 96-channel pack
  a = conv(1, 64, 64, 64, 64, 64, ST_S16P_BOTH);
  CHECK(choose_conv3x3_f16x3(a, 256, c) == -1006);
  a = conv(1, 64, 64, 64, 64, 64, ST_NHWC); a.in0.rs += 4;
  CHECK(choose_conv3x3_f16x3(a, 256, c) == -1004);
  a = conv(1, 64, 64, 64, 96, 96, ST_NHWC);
  CHECK(choose_conv3x3_f16x3(a, 256, c) == -1000);
  // the small-grid threshold, shared by ng32, the <1,1,8> form, the multi launch and the plan
  CHECK(small_grid(1, 240, 256, 1) && !small_grid(1, 256, 256, 1));      // 15 x 16 = 240 / 16 x 16 = 256 workgroups
  CHECK(use_ng32(1, 60, 80, 64, 0) && !use_ng32(16, 60, 80, 64, 0) && !use_ng32(1, 60, 80, 32, 0) && !use_ng32(1, 60, 80, 64, 8));
  std::printf(fails ? "FAILED\n" : "OK\n");
  return fails;
}
"""

# (frames, H, W, lanes) -> "layer variant grid" per layer; the forward splits the frames into ceil(frames / lanes) per lane
EXPECTED = {
    (1, 120, 160, 1): ['conv1b <1,1,8> 0', 'conv2a <1,1,8> 0', 'conv2b <1,1,8> 0', 'conv3a <1,1,8> 0', 'conv3b <1,1,8> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <1,1,8> 0'],
    (1, 120, 160, 2): ['conv1b <1,1,8> 0', 'conv2a <1,1,8> 0', 'conv2b <1,1,8> 0', 'conv3a <1,1,8> 0', 'conv3b <1,1,8> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <1,1,8> 0'],
    (2, 120, 160, 1): ['conv1b <1,1,8> 0', 'conv2a <1,1,8> 0', 'conv2b <1,1,8> 0', 'conv3a <1,1,8> 0', 'conv3b <1,1,8> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <1,1,8> 0'],
    (2, 120, 160, 2): ['conv1b <1,1,8> 0', 'conv2a <1,1,8> 0', 'conv2b <1,1,8> 0', 'conv3a <1,1,8> 0', 'conv3b <1,1,8> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <1,1,8> 0'],
    (16, 120, 160, 1): ['conv1b <1,1,16> 0', 'conv2a <1,1,16> 0', 'conv2b <1,1,16> 0', 'conv3a <1,1,16> 0', 'conv3b <2,1,16> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <2,1,16> 0'],
    (16, 120, 160, 2): ['conv1b <1,1,16> 0', 'conv2a <1,1,8> 0', 'conv2b <1,1,8> 0', 'conv3a <1,1,8> 0', 'conv3b <1,1,16> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <1,1,16> 0'],
    (32, 120, 160, 1): ['conv1b <ws>stem 256', 'conv2a <1,1,16> 0', 'conv2b <1,1,16> 0', 'conv3a <1,1,16> 0', 'conv3b <2,1,16> 0', 'conv4a <1,1,16> 0', 'conv4b <1,1,16> 0', 'heads.first <wsm> 216'],
    (32, 120, 160, 2): ['conv1b <1,1,16> 0', 'conv2a <1,1,16> 0', 'conv2b <1,1,16> 0', 'conv3a <1,1,16> 0', 'conv3b <2,1,16> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <wsm> 112'],
    (64, 120, 160, 1): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 256', 'conv2b <s16> 256', 'conv3a <s16> 256', 'conv3b <s16> 256', 'conv4a <2,1,16> 0', 'conv4b <2,1,16> 0', 'heads.first <wsm> 256'],
    (64, 120, 160, 2): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 128', 'conv2b <s16> 128', 'conv3a <s16> 128', 'conv3b <s16> 128', 'conv4a <1,1,16> 0', 'conv4b <1,1,16> 0', 'heads.first <wsm> 128'],
    (1, 240, 320, 1): ['conv1b <1,1,16> 0', 'conv2a <1,1,8> 0', 'conv2b <1,1,8> 0', 'conv3a <1,1,8> 0', 'conv3b <1,1,8> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <1,1,8> 0'],
    (1, 240, 320, 2): ['conv1b <1,1,16> 0', 'conv2a <1,1,8> 0', 'conv2b <1,1,8> 0', 'conv3a <1,1,8> 0', 'conv3b <1,1,8> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <1,1,8> 0'],
    (2, 240, 320, 1): ['conv1b <1,1,16> 0', 'conv2a <1,1,8> 0', 'conv2b <1,1,8> 0', 'conv3a <1,1,8> 0', 'conv3b <1,1,16> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <1,1,16> 0'],
    (2, 240, 320, 2): ['conv1b <1,1,16> 0', 'conv2a <1,1,8> 0', 'conv2b <1,1,8> 0', 'conv3a <1,1,8> 0', 'conv3b <1,1,8> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <1,1,8> 0'],
    (16, 240, 320, 1): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 216', 'conv2b <s16> 216', 'conv3a <s16> 216', 'conv3b <s16> 216', 'conv4a <2,1,16> 0', 'conv4b <2,1,16> 0', 'heads.first <wsm> 240'],
    (16, 240, 320, 2): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 112', 'conv2b <s16> 112', 'conv3a <s16> 112', 'conv3b <s16> 112', 'conv4a <1,1,16> 0', 'conv4b <1,1,16> 0', 'heads.first <wsm> 120'],
    (32, 240, 320, 1): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 256', 'conv2b <s16> 256', 'conv3a <s16> 256', 'conv3b <s16> 256', 'conv4a <wsm>s16io 192', 'conv4b <wsm>s16io 192', 'heads.first <wsm>s16io 240'],
    (32, 240, 320, 2): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 128', 'conv2b <s16> 128', 'conv3a <s16> 128', 'conv3b <s16> 128', 'conv4a <wsm>s16io 96', 'conv4b <wsm>s16io 96', 'heads.first <wsm>s16io 120'],
    (64, 240, 320, 1): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 256', 'conv2b <s16> 256', 'conv3a <s16> 256', 'conv3b <s16> 256', 'conv4a <wsm>s16io 256', 'conv4b <wsm>s16io 256', 'heads.first <wsm>s16io 256'],
    (64, 240, 320, 2): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 128', 'conv2b <s16> 128', 'conv3a <s16> 128', 'conv3b <s16> 128', 'conv4a <wsm>s16io 128', 'conv4b <wsm>s16io 128', 'heads.first <wsm>s16io 128'],
    (1, 480, 640, 1): ['conv1b <1,1,16> 0', 'conv2a <1,1,16> 0', 'conv2b <1,1,16> 0', 'conv3a <1,1,16> 0', 'conv3b <2,1,16> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <2,1,8> 0'],
    (1, 480, 640, 2): ['conv1b <1,1,16> 0', 'conv2a <1,1,16> 0', 'conv2b <1,1,16> 0', 'conv3a <1,1,16> 0', 'conv3b <2,1,16> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <2,1,8> 0'],
    (2, 480, 640, 1): ['conv1b <ws>stem 256', 'conv2a <1,1,16> 0', 'conv2b <1,1,16> 0', 'conv3a <1,1,16> 0', 'conv3b <2,1,16> 0', 'conv4a <1,1,16> 0', 'conv4b <1,1,16> 0', 'heads.first <2,1,8> 0'],
    (2, 480, 640, 2): ['conv1b <1,1,16> 0', 'conv2a <1,1,16> 0', 'conv2b <1,1,16> 0', 'conv3a <1,1,16> 0', 'conv3b <2,1,16> 0', 'conv4a <1,1,8> 0', 'conv4b <1,1,8> 0', 'heads.first <2,1,8> 0'],
    (16, 480, 640, 1): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 240', 'conv2b <s16> 240', 'conv3a <s16> 240', 'conv3b <s16> 240', 'conv4a <wsm>s16io 216', 'conv4b <wsm>s16io 216', 'heads.first <wsm>s16io 248'],
    (16, 480, 640, 2): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 120', 'conv2b <s16> 120', 'conv3a <s16> 120', 'conv3b <s16> 120', 'conv4a <wsm>s16io 112', 'conv4b <wsm>s16io 112', 'heads.first <wsm>s16io 128'],
    (32, 480, 640, 1): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 256', 'conv2b <s16> 256', 'conv3a <s16> 256', 'conv3b <s16> 256', 'conv4a <wsm>s16io 256', 'conv4b <wsm>s16io 256', 'heads.first <wsm>s16io 256'],
    (32, 480, 640, 2): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 128', 'conv2b <s16> 128', 'conv3a <s16> 128', 'conv3b <s16> 128', 'conv4a <wsm>s16io 128', 'conv4b <wsm>s16io 128', 'heads.first <wsm>s16io 128'],
    (64, 480, 640, 1): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 256', 'conv2b <s16> 256', 'conv3a <s16> 256', 'conv3b <s16> 256', 'conv4a <wsm>s16io 256', 'conv4b <wsm>s16io 256', 'heads.first <wsm>s16io 256'],
    (64, 480, 640, 2): ['conv1b <ws>stem+s16 256', 'conv2a <s16> 128', 'conv2b <s16> 128', 'conv3a <s16> 128', 'conv3b <s16> 128', 'conv4a <wsm>s16io 128', 'conv4b <wsm>s16io 128', 'heads.first <wsm>s16io 128'],
}


def _compile(tmp_path, name, code):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is required for the conv policy test")
    (tmp_path / (name + ".cpp")).write_text(code)
    exe = tmp_path / name
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-include", "string", "-I", os.path.join(ROOT, "nano-vs-slam_amd", "csrc"),
                    str(tmp_path / (name + ".cpp")), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("conv_policy"), "plan", SRC)


@pytest.mark.parametrize("frames,H,W,lanes", sorted(EXPECTED))
def test_conv_policy_forms_of_kp2dtiny_s(plan_exe, frames, H, W, lanes):
    nl = min(lanes, frames)
    per_lane = -(-frames // nl)
    out = subprocess.run([plan_exe, str(per_lane), str(H), str(W), str(nl)], check=True, capture_output=True, text=True).stdout
    assert out.splitlines() == EXPECTED[(frames, H, W, lanes)]


def test_conv_policy_boundaries_and_overrides(tmp_path):
    exe = _compile(tmp_path, "edges", SRC_EDGES)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
