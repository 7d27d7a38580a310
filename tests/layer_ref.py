"""One convolution layer of the engine in float64, with a per-element error bound derived from the arithmetic.

The reference takes the DEVICE's own input(s) to a layer (kp2d_set_tap on the producing layer(s)) and the state dict,
and computes the layer's output in float64 with the oracle's numpy functions.  Because its input is what the device
actually fed the layer, one comparison isolates one kernel launch: errors of earlier layers do not accumulate into it.

What a layer folds into its store is folded here too: the max-pool of the pooled stores, the pixel shuffle of convB and
convs.4 / .6, the two-source layers (confAa, convs.5, convs.7 read ``cat(upsampled, skip)``), conv4a's input as the exact
``maxpool2`` of conv3b's full-resolution tap, the parts of the merged ``heads.first`` (tapped under the heads' own
names), and the planar API outputs ``score``, ``coord``, ``feat``, ``seg`` behind the heads' last layers.

The epilogue scale / shift are the fp32 values the weight upload folds BatchNorm into (model_desc.cpp bn_fold:
``s = gamma / sqrt(var + 1e-5f)``, ``sh = beta - mean * s``, both fp32): they are part of the weights the kernel is
given, not of its arithmetic, and are applied here in float64.

Error bound (per output element)
--------------------------------
Let z = sum_k x_k w_k over K = taps x Cin products, M = conv64(|x|, |w|), W1 = conv64(1[inside image], |w|) and s the
output channel's epilogue scale.  u = 2^-24 is the fp32 unit roundoff.

* fp32 accumulation.  Products and sums in fp32 (or exact fp16 x fp16 products summed in fp32) carry a rounding error
  that a worst-case analysis bounds by ~K u M.  Real sums of random-signed terms in blocked orders stay far below that,
  and a worst-case bound would be too loose to see a dropped split term at K = 576 (K u = 2^-14.8 against the
  2^-12 x 2^-11 of one lost cross term).  So the accumulation term is ``ALPHA * u * |s| * M`` with ALPHA fixed once:
  tests/test_layer_ref_cpu.py shows that a faithful fp32 emulation stays 4x below the bound and that every modelled
  kernel fault exceeds it 4x (the epilogue's own multiply-add, one more rounding of |acc s| <= |s| M, is inside ALPHA).
* The split (f16x3 only).  x = xh + xl + dx with xh = rn16(x), xl = rn16(x - xh): |dx| <= max(2^-22 |x|, 2^-25) (a normal
  xl keeps 11 bits, a subnormal one is off by at most half its spacing 2^-24).  Weights are split as w 2^e (e <= 11,
  the epilogue scale carries 2^-e), |dw| <= 2^-22 |w|.  The kernel sums xh wh + xh wl + xl wh: against x w it misses
  dx w + x dw + xl wl (|xl wl| <= 2^-22 |x w|, to first order), so the split adds ``|s| (3 * 2^-22 * M + 2^-25 * W1)``.
  The subnormal floor W1 term is what makes the bound hold for activations down to 2^-24; it is exponent-invariant
  because the weight scale cancels in the epilogue.  Left out in fp32 mode and for the exact-fp32 head kernel.
* Output rounding: ``2^-23 |y64|`` (the fp32 store after the activation; LeakyReLU's 0.01f is 0.01 to 2^-25).  The
  transcendental epilogues (sigmoid, tanh: libm-class expf / tanhf) take ``2^-21 |y64|`` (4 ulp).
* Propagation.  LeakyReLU, ReLU, sigmoid, tanh, max-pool and the shuffle are 1-Lipschitz (element-wise / max over a
  window / a permutation), so the pre-activation bound passes through them unchanged.  The channel softmax of V3's
  class map: |d ln p_i| <= b_i + max_j b_j, so |dp_i| <= p_i expm1(b_i + max_j b_j), plus p_i (C + 8) u for its own
  exponentials and the C-term sum.
"""
from __future__ import annotations

import os
import re

import numpy as np

from oracle import kp2d_oracle as orc

U = 2.0 ** -24
ALPHA = 32.0                 # fp32 accumulation, in units of u |s| M (tests/test_layer_ref_cpu.py pins it from both sides)
SPLIT_REL = 3 * 2.0 ** -22   # dx w + x dw + xl wl
SPLIT_FLOOR = 2.0 ** -25     # subnormal xl: half the fp16 subnormal spacing
OUT_LINEAR = 2.0 ** -23
OUT_TRANSCENDENTAL = 2.0 ** -21
GELU_SLOPE = 1.13            # max |d gelu / dx| = 1.1290 (at x = sqrt 2)
# conv_common.h gelu_fast (erf by Abramowitz & Stegun 7.1.26 with v_rcp_f32 and v_exp_f32) against the exact-erf GELU, relative
# to |x|: tests/test_attention_head_ref_cpu.py measures 3.00e-07 (at x = 0.055) for a numpy float32 emulation over a dense grid of
# [-12, 12]; twice that for the two hardware approximations (1 ulp each), which numpy computes correctly rounded
GELU_ERR = 6.0e-7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICY_H = os.path.join(ROOT, "nano-vs-slam_amd", "csrc", "conv_policy.h")

# profile kernel families that are convolutions (kp2d_profile_get); everything a case's profile lists under one of these
# must be compared or excluded below
CONV_FAMILIES = ("conv3x3_f16x3", "conv1x1_f16x3", "conv3x3_f32<", "conv1x1_f32", "conv3x3_head", "conv1a")
# the other launches of the attention segmentation head (tests/attention_head_ref.py)
HEAD_FAMILIES = ("channel_layernorm", "attention", "dwconv3x3", "mff_tail")
SPLIT_FAMILIES = ("conv3x3_f16x3", "conv1x1_f16x3", "conv1a_mfma", "attention_f16x3", "mff_tail")

# conv launches this module does not model, with the tests that cover them
EXCLUDED = {
    r"^vlad_head\.netvlad": "NetVLAD / ConvAP pooling: test_against_reference_golden (vlad), test_against_oracle_other_shapes",
}


def excluded(layer):
    return next((why for pat, why in EXCLUDED.items() if re.search(pat, layer)), None)


def policy_variants(path=POLICY_H):
    """Every tile-form variant literal conv_policy.h can report ("<ws>stem+s16", "<1,1,8,flat32>", ...)."""
    src = open(path).read()
    return sorted(set(re.findall(r'"(<[^"<>]*>[a-z0-9+]*)"', src)))


# ---------------------------------------------------------------------------------------------------------------------
# the layer graph
# ---------------------------------------------------------------------------------------------------------------------
class Spec:
    """One conv layer: sources [(tap | "@x", transform)], weights, epilogue, post-op of its store, and where its output is read.

    transform: None, "pool" (maxpool2 of the tap) or (c0, c1) (a channel slice).  out: ("tap", name) or
    ("api", [(key, c0, c1), ...]) — the API tensors the layer writes and which of its channels go there."""

    def __init__(self, name, srcs, bn=True, act="leaky", post=None, out=None, launch=None):
        self.name, self.srcs, self.bn, self.act, self.post = name, srcs, bn, act, post
        self.out = out or ("tap", name)
        self.launch = launch or name      # the layer name the profile lists the launch under

    def weight_key(self):
        return f"{self.name}.conv.weight" if self.bn else f"{self.name}.weight"


def layer_graph(cfg):
    """{layer name: Spec} for the V2 / V3 configurations with PixelShuffle upsampling.  The attention configurations add the
    stages of tests/attention_head_ref.py (LayerNorm, attention, depthwise 3x3, the fused MixFFN tail) between the conv layers
    of their segmentation head; both MixFFN paths are in the graph, the profile says which one ran."""
    if cfg["upscale_method"] != "pixelshuffle" or cfg.get("depth") or cfg["in_channels"] != 3:
        raise NotImplementedError("layer_ref models the V2 / V3 configurations with PixelShuffle upsampling")
    lk = "leaky" if cfg["leaky_relu"] else "relu"
    ds = cfg["downsample"]
    g = {}

    def add(name, srcs, **kw):
        kw.setdefault("act", lk)
        g[name] = Spec(name, srcs, **kw)

    B = "backbone."
    add(B + "conv1a", [("@x", None)])
    add(B + "conv1b", [(B + "conv1a", None)], post="pool" if ds >= 2 else None)
    add(B + "conv2a", [(B + "conv1b", None)])
    add(B + "conv2b", [(B + "conv2a", None)], post="pool" if ds >= 3 else None)
    add(B + "conv3a", [(B + "conv2b", None)])
    add(B + "conv3b", [(B + "conv3a", None)])
    add(B + "conv4a", [(B + "conv3b", "pool")])
    add(B + "conv4b", [(B + "conv4a", None)])
    xb, skip = [(B + "conv4b", None)], (B + "conv3b", None)
    if cfg["v3"]:
        add("score_loc_head.convDa", xb)
        add("score_loc_head.convDb", [("score_loc_head.convDa", None)], bn=False, act="sig0tanh",
            out=("api", [("score", 0, 1), ("coord", 0, 2)]))
    else:
        add("score_head.convDa", xb)
        add("score_head.convDb", [("score_head.convDa", None)], bn=False, act="sigmoid", out=("api", [("score", 0, 1)]))
        add("loc_head.convDa", xb)
        add("loc_head.convDb", [("loc_head.convDa", None)], bn=False, act="tanh", out=("api", [("coord", 0, 2)]))
        add("desc_head.convA", xb)
        add("desc_head.convB", [("desc_head.convA", None)], bn=False, act="none", post="shuffle")
        add("desc_head.confAa", [("desc_head.convB", None), skip])
        add("desc_head.confBb", [("desc_head.confAa", None)], bn=False, act="none", out=("api", [("feat", 0, cfg["nfeatures"])]))
    L = "seg_head.convs."
    add(L + "0", xb)
    if cfg["use_attention"]:      # oracle seg_trunk, attention branch: CBR, module (+ pool), module, CBR + shuffle, ...
        import attention_head_ref as A
        A.add_module(g, L + "1", L + "0", pool=True)
        A.add_module(g, L + "2", L + "1.mff", pool=False)
        add(L + "3", [(L + "2.mff", None)], post="shuffle")
        i = 4
    else:
        add(L + "1", [(L + "0", None)], post="pool")
        add(L + "2", [(L + "1", None)])
        add(L + "3", [(L + "2", None)])
        add(L + "4", [(L + "3", None)], post="shuffle")
        i = 5
    add(L + str(i), [(L + str(i - 1), None)] + xb)
    add(L + str(i + 1), [(L + str(i), None)], post="shuffle")
    add(L + str(i + 2), [(L + str(i + 1), None), skip])
    trunk, last = L + str(i + 2), L + str(i + 3)
    if cfg["v3"]:
        half = cfg["channel_dims"][4] // 2
        add("seg_head.featB", [(trunk, (0, half))], bn=False, act="none", out=("api", [("feat", 0, cfg["nfeatures"])]))
        add(last, [(trunk, (-half, None))], bn=False, act="softmax", out=("api", [("seg", 0, None)]))
    else:
        add(last, [(trunk, None)], bn=False, act="none", out=("api", [("seg", 0, None)]))
    add("vlad_head.convlad1", xb)
    add("vlad_head.convlad2", [("vlad_head.convlad1", None)])
    add("vlad_head.convlad3", [("vlad_head.convlad2", None)])
    return g


def merged_parts(cfg):
    """The layers the merged first launch of the heads ("heads.first", model_desc.cpp describe()) computes."""
    parts = ["score_loc_head.convDa"] if cfg["v3"] else ["score_head.convDa", "loc_head.convDa", "desc_head.convA"]
    return parts + ([] if cfg["use_attention"] else ["seg_head.convs.0"]) + ["vlad_head.convlad1"]


def tap_shapes(cfg, sd, H, W):
    """(C, H, W) of every tap the graph reads or writes, for forward_with_tap."""
    g = layer_graph(cfg)
    shp = {"@x": (cfg["in_channels"], H, W)}

    def src_shape(s, tr):
        c, h, w = shp[s]
        if tr == "pool":
            return c, h // 2, w // 2
        if isinstance(tr, tuple):
            return len(range(c)[tr[0]:tr[1]]), h, w
        return c, h, w

    for name, sp in g.items():          # (insertion order is a topological order)
        if hasattr(sp, "shape"):        # a stage of attention_head_ref
            shp[name] = sp.shape([src_shape(*s) for s in sp.srcs])
            continue
        _, h, w = src_shape(*sp.srcs[0])
        co = sd[sp.weight_key()].shape[0]
        if sd[sp.weight_key()].shape[-1] == 2:      # the 2 x 2 stride-2 to_kv
            h, w = h // 2, w // 2
        if sp.post == "pool":
            h, w = h // 2, w // 2
        elif sp.post == "shuffle":
            co, h, w = co // 4, 2 * h, 2 * w
        shp[name] = (co, h, w)
    return shp


# ---------------------------------------------------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------------------------------------------------
def fold(sd, sp):
    """The fp32 epilogue scale and shift the weight upload gives the kernel (model_desc.cpp bn_fold / the bias layers)."""
    co = sd[sp.weight_key()].shape[0]
    if not sp.bn:
        b = sd.get(f"{sp.name}.bias")
        return np.ones(co, np.float32), (np.asarray(b, np.float32) if b is not None else np.zeros(co, np.float32))
    p = f"{sp.name}.bn"
    gmm, beta = np.asarray(sd[p + ".weight"], np.float32), np.asarray(sd[p + ".bias"], np.float32)
    mu, var = np.asarray(sd[p + ".running_mean"], np.float32), np.asarray(sd[p + ".running_var"], np.float32)
    s = (gmm / np.sqrt(var + np.float32(1e-5))).astype(np.float32)
    return s, (beta - mu * s).astype(np.float32)


def pre_activation(x, w, s, sh, split, b_in=None):
    """z64 * s + sh and its bound for planar inputs x [C, H, W] (float64) and weights w [Co, C, 3, 3] ([Co, C, 1, 1], or the
    [Co, C, 2, 2] of a stride-2 conv).  b_in: a bound on the error the input itself carries (a stage computed inside the same
    launch): a linear layer passes it on as |s| conv(b_in, |w|)."""
    x = np.asarray(x, np.float64)[None]
    w = np.asarray(w, np.float64)
    conv = {3: orc.conv2d_3x3, 2: orc.conv2d_2x2_s2, 1: orc.conv2d_1x1}[w.shape[-1]]
    z = conv(x, w)[0]
    M = conv(np.abs(x), np.abs(w))[0]
    s64, sh64 = s.astype(np.float64)[:, None, None], sh.astype(np.float64)[:, None, None]
    b = ALPHA * U * M
    if split:
        ones = np.ones((1, 1) + x.shape[2:])
        W1 = conv(ones, np.abs(w).sum(axis=1, keepdims=True))[0]
        b = b + SPLIT_REL * M + SPLIT_FLOOR * W1
    if b_in is not None:
        b = b + conv(np.asarray(b_in, np.float64)[None], np.abs(w))[0]
    return z * s64 + sh64, np.abs(s64) * b


def activate(pre, b, act):
    """y64 and its bound behind the layer's activation (1-Lipschitz ones pass the bound through)."""
    if act == "leaky":
        y = np.where(pre >= 0, pre, 0.01 * pre)
    elif act == "relu":
        y = np.maximum(pre, 0.0)
    elif act == "none":
        y = pre
    elif act == "sigmoid":
        y = 1.0 / (1.0 + np.exp(-pre))
    elif act == "tanh":
        y = np.tanh(pre)
    elif act == "sig0tanh":
        y = np.concatenate([1.0 / (1.0 + np.exp(-pre[:1])), np.tanh(pre[1:])])
    elif act == "gelu":
        # exact-erf GELU; |d gelu / dx| <= 1.13, and the device's gelu_fast is GELU_ERR |x| away from it
        y = orc.gelu_erf(pre)
        return y, GELU_SLOPE * b + GELU_ERR * np.abs(pre) + OUT_LINEAR * np.abs(y)
    elif act == "softmax":
        e = np.exp(pre - pre.max(axis=0, keepdims=True))
        y = e / e.sum(axis=0, keepdims=True)
        return y, y * np.expm1(b + b.max(axis=0, keepdims=True)) + y * (pre.shape[0] + 8) * U
    else:
        raise ValueError(act)
    out = OUT_TRANSCENDENTAL if act in ("sigmoid", "tanh", "sig0tanh") else OUT_LINEAR
    return y, b + out * np.abs(y)


def post_op(y, b, post):
    if post == "pool":
        return orc.maxpool2(y[None])[0], orc.maxpool2(b[None])[0]
    if post == "shuffle":
        return orc.pixel_shuffle2(y[None])[0], orc.pixel_shuffle2(b[None])[0]
    return y, b


def source(tap, tr):
    t = np.asarray(tap, np.float64)
    if tr == "pool":
        return orc.maxpool2(t[None])[0]
    if isinstance(tr, tuple):
        return t[tr[0]:tr[1]]
    return t


def reference(sp, inputs, sd, split):
    """Float64 output of layer `sp` for ONE frame and its per-element bound.  inputs: the planar [C, H, W] taps named by
    sp.srcs, in order; split: the launch ran the split-fp16 arithmetic."""
    if hasattr(sp, "ref"):          # a stage of attention_head_ref
        return sp.ref([source(t, tr) for t, (_, tr) in zip(inputs, sp.srcs)], sd, split)
    x = np.concatenate([source(t, tr) for t, (_, tr) in zip(inputs, sp.srcs)], axis=0)
    s, sh = fold(sd, sp)
    pre, b = pre_activation(x, sd[sp.weight_key()], s, sh, split)
    y, b = activate(pre, b, sp.act)
    return post_op(y, b, sp.post)


def check(got, y, b):
    """(worst err / bound, its index, all finite) of a device result against the reference."""
    got = np.asarray(got, np.float64)
    assert got.shape == y.shape, (got.shape, y.shape)
    finite = bool(np.isfinite(got).all())
    r = np.abs(got - y) / b
    r = np.where(np.isfinite(r), r, np.inf)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), i, finite


def is_conv_family(kernel):
    return kernel.startswith(CONV_FAMILIES)


def is_split_family(kernel):
    return kernel.startswith(SPLIT_FAMILIES)


def variant_of(kernel):
    """"<wsm>s16io" of "conv3x3_f16x3<wsm>s16io"; "" for the families without tile forms."""
    return kernel[len("conv3x3_f16x3"):] if kernel.startswith("conv3x3_f16x3") else ""


# ---------------------------------------------------------------------------------------------------------------------
# the GPU cases (tests/test_gpu_layer_fp64.py); kept here so that the CPU suite can check their coverage of the policy
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, cid, config, v3, ncls, B, H, W, frames, options, variants, sweep=()):
        self.id, self.config, self.v3, self.ncls = cid, config, v3, ncls
        self.B, self.H, self.W, self.frames = B, H, W, frames
        self.options = options      # kp2d_set_option key -> value, applied after kp2d_create
        self.variants = variants    # the exact set of conv3x3_f16x3 tile forms its f16x3 profiled forward runs
        self.sweep = sweep          # (producer, consumer) pairs of the activation-magnitude sweep (f16x3)


CASES = [
    Case("S_v2_headline_lanes1", "S", False, 28, 64, 240, 320, [0, 63], {"lanes": 1},
         {"<ws>stem+s16", "<s16>", "<wsm>s16io", "<wsm>s16in", "<wsm>s16out", "<s16>planar", "<2,1,16>", "<1,1,8,flat32>"},
         sweep=(("backbone.conv1b", "backbone.conv2a"), ("backbone.conv3b", "backbone.conv4a"),
                ("desc_head.convA", "desc_head.convB"), ("seg_head.convs.4", "seg_head.convs.5"))),
    Case("S_v2_headline_lanes2", "S", False, 28, 64, 240, 320, [0, 31, 32, 63], {},
         {"<ws>stem+s16", "<s16>", "<wsm>s16io", "<wsm>s16in", "<wsm>s16out", "<s16>planar", "<2,1,16>", "<1,1,8,flat32>"}),
    Case("S_v2_headline_general", "S", False, 28, 64, 240, 320, [0, 63],
         {"lanes": 1, "wsm_min_items": -1, "s16_min_items": -1},
         {"<ws>stem", "<1,2,16>", "<2,1,16>", "<2,1,8>", "<1,1,8,flat32>"}),
    Case("S_v2_ragged_wsm", "S", False, 28, 5, 104, 176, [0, 4], {"lanes": 1, "wsm_min_items": 8},
         {"<1,1,16>", "<2,1,16>", "<wsm32>", "<wsm>", "<1,1,8>"}),
    Case("S_v2_ragged_wsm_transposed", "S", False, 28, 5, 104, 176, [0, 4],
         {"lanes": 1, "wsm_min_items": 8, "wsm_transposed": 1},
         {"<1,1,16>", "<2,1,16>", "<wsm32>", "<wsm>t", "<1,1,8>"}),
    Case("S_v2_s16_all_ragged_unfused_stem", "S", False, 28, 12, 272, 320, [0, 11],
         {"lanes": 1, "s16_min_items": 1, "ws_min_tiles": 1, "wsm_min_items": 1, "stem_fusion": 2},
         {"<ws>s16", "<s16>", "<wsm>", "<wsm>s16io", "<wsm>s16in", "<wsm>s16out", "<s16>planar", "<1,1,8,flat32>"}),
    Case("S_v2_480x640", "S", False, 28, 2, 480, 640, [0, 1], {"lanes": 1},
         {"<ws>stem", "<1,1,16>", "<1,1,8>", "<2,1,16>", "<2,1,8>"}),
    Case("S_v2_one_frame", "S", False, 28, 1, 120, 160, [0], {"lanes": 1}, {"<1,1,8>"},
         sweep=(("backbone.conv1b", "backbone.conv2a"),)),
    Case("S_v2_16x120x160", "S", False, 28, 16, 120, 160, [0, 15], {"lanes": 1},
         {"<1,1,16>", "<2,1,16>", "<1,1,8>"}),
    Case("N_v2_240x320", "N", False, 28, 8, 240, 320, [0, 7], {"lanes": 1}, {"<ws>", "<1,1,16>", "<1,1,8>", "<1,1,8,flat32>", "<2,1,16>", "<2,1,8>"}),
    Case("N_v2_small", "N", False, 28, 2, 40, 56, [0, 1], {"lanes": 1}, {"<1,1,8>"}),
    Case("S_v3_heads", "S", True, 19, 3, 104, 176, [0, 2], {"lanes": 1}, {"<1,1,8>"}),
    Case("F_v2_three_pools", "F", False, 28, 2, 48, 80, [0, 1], {"lanes": 1}, {"<1,1,8>"}),
]
