// Host-side choice of the launch forms of one LightGlue forward (lightglue_plan.cpp run_forward, lightglue.hip
// launch_lg_tail): fused block tails or the lg_linear chain, projections inside the tails' launches or on their own, waves
// per tail workgroup, and the sequences each attention launch walks.  Plain C++: the tuning values (options.h Tuning:
// lg_fuse, lg_fuse_next, lg_tail_nw) are arguments (tests/test_lightglue_forms.py compiles it with g++).
#pragma once

namespace kp2d {

struct LgForm {
  bool fuse_tail;   // out_proj / to_out + ffn + residual as ONE row-local launch (lg_tail_mfma_kernel); else four lg_linear launches
  bool fused;       // the projection that follows a block runs in the tail's launch (and layer 0's Wqkv as a projection-only tail)
};

// D = 32 (configs S, A) has the fused tail; every other width runs the lg_linear chain whatever the knobs say
inline LgForm choose_lg_form(int D, bool lg_fuse, bool lg_fuse_next) {
  LgForm f;
  f.fuse_tail = lg_fuse && D == 32;
  f.fused = f.fuse_tail && lg_fuse_next;
  return f;
}

// waves per workgroup of the tail (16 rows each): the lg_tail_mfma_kernel<NW> instance; 0: not built
inline int lg_tail_waves(int lg_tail_nw) {
  const int nw = lg_tail_nw ? lg_tail_nw : 4;
  return nw == 4 || nw == 1 ? nw : 0;
}

// One attention launch of a block.  Sets: 0 = image 0's rows, 1 = image 1's (they follow image 0's in every buffer).
struct LgAttLaunch {
  int B, S, T;          // sequences, queries and keys per sequence
  int q_set, k_set;     // the set the first query / key sequence belongs to
  int kv_bshift;        // AttnArgs::kv_bshift
};

// The launches of a block's attention (self: every set attends to itself; cross: to the other set): returns their number.
// M == N: both images as one batch of 2B sequences, cross attention reading sequence (b + B) mod 2B.
inline int lg_attention_launches(int B, int M, int N, bool cross, LgAttLaunch out[2]) {
  if (M == N) {
    out[0] = LgAttLaunch{2 * B, M, M, 0, 0, cross ? B : 0};
    return 1;
  }
  for (int set = 0; set < 2; ++set) {
    const int other = cross ? 1 - set : set;
    out[set] = LgAttLaunch{B, set ? N : M, other ? N : M, set, other, 0};
  }
  return 2;
}

}  // namespace kp2d
