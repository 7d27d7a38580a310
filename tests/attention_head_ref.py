"""The launches of a SegFormerAttentionModule (Plan::attention_module) in float64, one stage per launch, with per-element error
bounds derived from the kernels' arithmetic.  Extends tests/layer_ref.py: layer_graph() calls add_module() for the attention
configurations, and every stage reads the DEVICE's own tapped input(s), so one comparison isolates one launch.

The 1x1 layers (to_q, to_out, mff.fn.net.0, net.1.net.1 + GELU, net.3 with or without the pooled store) and the 2x2 stride-2
to_kv are plain layer_ref Specs: layer_ref.pre_activation / activate / post_op with the bias as the epilogue shift.  The stages
below are the launches that are no convolution.  u = 2^-24.

LayerNorm (channel_layernorm_q_kernel / channel_layernorm_kernel: y = (x - mean) / (std + 1e-5) g + b, biased variance)
    Two passes in fp32.  The channel sum is a tree of depth <= 7 (two adds inside a float4 and log2 of the lane group, or six
    butterfly steps), times 1 / C (one rounding of the constant, one of the product): |mean^ - mean| <= dm = u (LN_SUM mean|x|
    + 2 |mean|) with LN_SUM = 7 (mean|x| <= max|x|).  The deviations v = x - mean^ inherit dm absolutely, plus u |v| of their
    own.  Because sum(x - mean) = 0 the common shift enters the variance only as its square: std^ = sqrt(var + dm^2) up to
    LN_STD u std for the squares, their tree sum, 1 / C and the square root, so |std^ - std| <= sqrt(std^2 + dm^2) - std +
    LN_STD u std.  The divisor D = std + eps adds 2 u D (the fp32 constant 1e-5f, the addition).  With r = |g| / (std + eps):
        bound = r dm  +  |x - mean| r (dstd + 2 u D) / D  +  4 u |x - mean| r  +  2^-23 |y|
    (the 4 u: v's own rounding, the division, the multiply by g, the add of b; division and square root are correctly
    rounded).  Every term is a function of the pixel's float64 mean, std, mean|x| and of g, b, so the bound follows the input
    down to any scale: for std << eps the divisor is eps and the r dm term, relative to the output's spread, stays dm / std.

Attention (attention_ksplit_kernel / attention_split_kernel in f16x3, attention_kernel in fp32; q [S, C], kv [T, 2C])
    Logits.  f16x3: q' = q * (scale * log2 e) in fp32 (three roundings: the two constants' product, the multiply), q' and k split
    into fp16 hi + lo, kh q'h + kh q'l + kl q'h summed in fp32 into an accumulator that starts at minus the running maximum.
    Neither operand carries a power-of-two scale, so the subnormal floor of the split applies to both.  With M = sum_c |q_c k_c|:
        E(j) = scale ((ALPHA u + SPLIT_REL) M_j + SPLIT_FLOOR (sum_c |q_c| + sum_c |k_jc| / (scale log2 e)))
               + ATT_LOGIT u (|s_j| + max_j |s_j|)
    (the last term: the roundings of q', and of sums whose partial values are as large as the reference the accumulator starts
    from).  fp32: exact products in fp32 sums, E(j) = scale ALPHA u M_j + ATT_LOGIT u (|s_j| + max|s|).  E_s = max_j E(j).
    Softmax: logits off by at most E_s move every probability by a factor within exp(+-2 E_s): expm1(2 E_s) sum_j p_j |v_jc|.
    P V and the denominator (row 16 of the same matrix product in f16x3): each ATT_PV u + SPLIT_REL relative to sum_j p_j |v_jc|
    (>= |o_c|), where ATT_PV u also holds the 1-ulp exp2 and the rescaling of the accumulator at a new maximum; the floors
    of the split of p (every key: a lo half below 2^-14 is a multiple of 2^-24) and of v:
        SPLIT_FLOOR (sum_j |v_jc| + T |o_c| + 1)
    Output: 2^-23 |o|.

Depthwise 3x3 (dwconv3x3_kernel): nine fp32 FMAs on top of the bias, in tap order: DW_ACC u (conv(|x|, |w|) + |b|) + 2^-23 |y|.

mff_tail (one launch: depthwise -> split 1x1 + bias -> GELU -> split 1x1 + bias [-> max-pool]): the composition of the stages
    above, each with its own term, a stage's input bound carried through GELU times 1.13 and through the next linear layer.
    The worst case conv(b_in, |w|) of that step assumes that the errors of all 128 hidden channels, each already at its
    bound, line up with the signs of the weights; it comes out so wide (1e-3 of the output) that a dropped cross term of the
    second product or a tanh-form GELU pass.  The accumulation and split errors of different hidden channels are independent
    roundings of zero mean, so they are carried as the root sum of squares sqrt(conv(b_in^2, w^2)): every b_in is a bound
    that faithful arithmetic uses at most a quarter of (the CPU test's 4x margin on the 1x1 and depthwise stages; on the device
    those launches of their own use up to 0.07 and 0.32), so this is three to four standard deviations of the propagated error
    at the least, and more than ten for the 1x1 part that dominates it.  This departs from the plain conv(b_in, |w|) on purpose,
    towards the tighter side; the CPU test holds it from both sides like every other constant.  gelu_fast's own error, a fixed function of x and not a
    rounding, keeps the worst case conv(GELU_ERR |pre|, |w|) (layer_ref.pre_activation b_in).

tests/test_attention_head_ref_cpu.py pins every constant from both sides (faithful float32 emulations 4x inside, modelled
kernel faults 4x outside) and evaluates attention_form.h for the GPU cases below."""
from __future__ import annotations

import numpy as np

import layer_ref as L
from oracle import kp2d_oracle as orc

U = L.U
LN_SUM = 7.0         # the channel sum's tree depth: its error in units of u sum|x| (so, of u mean|x| for the mean)
LN_STD = 8.0         # relative error of std^ beyond the shift of the mean, in u
LN_EPS = 1e-5
ATT_LOGIT = 4.0      # roundings of a logit at the magnitude of the logit and of the running maximum, in u
ATT_PV = 32.0        # = layer_ref.ALPHA: fp32 accumulation of P V over the keys, exp2, the online rescaling
DW_ACC = 10.0        # nine FMAs and the bias
HEADS = 4            # SegFormerAttentionModule(c): heads 4, reduction 2, expansion 2
PEAK_LIMIT = 2.0 ** 15      # lightglue_fp64_ref.PEAK_LIMIT: the device is compared while the operands of its split stay below


class Stage:
    """A launch that is no convolution.  srcs as in layer_ref.Spec; ref(inputs, sd, split) -> (y64, bound) for one frame;
    shape(source shapes) -> (C, H, W) of the output tap."""

    post = None

    def __init__(self, name, srcs, launch=None):
        self.name, self.srcs, self.out, self.launch = name, srcs, ("tap", name), launch or name


def _vec(sd, key):
    return np.asarray(sd[key], np.float64).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def layernorm_ref(x, g, b):
    x = np.asarray(x, np.float64)
    g, b = g[:, None, None], b[:, None, None]
    mean = x.mean(axis=0, keepdims=True)
    d = x - mean
    std = np.sqrt((d * d).mean(axis=0, keepdims=True))
    y = orc.channel_layernorm(x[None], g[None], b[None], eps=LN_EPS)[0]
    dm = U * (LN_SUM * np.abs(x).mean(axis=0, keepdims=True) + 2 * np.abs(mean))
    D = std + LN_EPS
    dstd = np.sqrt(std * std + dm * dm) - std + LN_STD * U * std
    r = np.abs(g) / D
    bound = r * dm + np.abs(d) * r * (dstd + 2 * U * D) / D + 4 * U * np.abs(d) * r + L.OUT_LINEAR * np.abs(y)
    return y, bound


class LayerNorm(Stage):
    def ref(self, inputs, sd, split):
        return layernorm_ref(inputs[0], _vec(sd, self.name + ".g"), _vec(sd, self.name + ".b"))

    def shape(self, shapes):
        return shapes[0]


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def attention_ref(q, kv, split, heads=HEADS):
    """softmax(q k^T d^-0.5) v per head from the planar q [C, h, w] and kv [2C, h/2, w/2] (orc.efficient_self_attention
    between its convolutions)."""
    q, kv = np.asarray(q, np.float64), np.asarray(kv, np.float64)
    C, h, w = q.shape
    d = C // heads
    scale = d ** -0.5
    qh = q.reshape(heads, d, h * w).transpose(0, 2, 1)           # heads, S, d
    kh = kv[:C].reshape(heads, d, -1)                            # heads, d, T
    vh = kv[C:].reshape(heads, d, -1).transpose(0, 2, 1)         # heads, T, d
    T = kh.shape[2]
    s = np.matmul(qh, kh) * scale
    M = np.matmul(np.abs(qh), np.abs(kh))
    smax = np.abs(s).max(axis=2, keepdims=True)
    E = scale * L.ALPHA * U * M + ATT_LOGIT * U * (np.abs(s) + smax)
    if split:
        f = scale * np.log2(np.e)
        E = E + scale * (L.SPLIT_REL * M + L.SPLIT_FLOOR * (np.abs(qh).sum(axis=2, keepdims=True) + np.abs(kh).sum(axis=1, keepdims=True) / f))
    Es = E.max(axis=2, keepdims=True)                            # heads, S, 1
    p = orc.softmax(s, axis=2)
    o = np.matmul(p, vh)                                         # heads, S, d
    pv = np.matmul(p, np.abs(vh))
    bound = np.expm1(2 * Es) * pv + 2 * ATT_PV * U * pv + L.OUT_LINEAR * np.abs(o)
    if split:
        bound = bound + 2 * L.SPLIT_REL * pv + L.SPLIT_FLOOR * (np.abs(vh).sum(axis=1, keepdims=True) + T * np.abs(o) + 1.0)
    back = lambda t: t.transpose(0, 2, 1).reshape(C, h, w)
    return back(o), back(bound)


class Attention(Stage):
    def ref(self, inputs, sd, split):
        return attention_ref(inputs[0], inputs[1], split)

    def shape(self, shapes):
        return shapes[0]


# ---------------------------------------------------------------------------------------------------------------------
# depthwise 3x3 and the fused tail
# ---------------------------------------------------------------------------------------------------------------------
def depthwise_ref(x, w, b):
    x, w, b = np.asarray(x, np.float64)[None], np.asarray(w, np.float64), np.asarray(b, np.float64)
    y = orc.dwconv2d_3x3(x, w, b)[0]
    m = orc.dwconv2d_3x3(np.abs(x), np.abs(w), np.abs(b))[0]
    return y, DW_ACC * U * m + L.OUT_LINEAR * np.abs(y)


class Depthwise(Stage):
    def ref(self, inputs, sd, split):
        return depthwise_ref(inputs[0], sd[self.name + ".weight"], sd[self.name + ".bias"])

    def shape(self, shapes):
        return shapes[0]


def _bias_layer(sd, name):
    w = sd[name + ".weight"]
    return w, np.ones(w.shape[0], np.float32), np.asarray(sd[name + ".bias"], np.float32)


def _rss(b, w):
    """independent rounding errors, each within b, through a linear layer: the root sum of squares (see mff_tail above)"""
    w = np.asarray(w, np.float64)
    return np.sqrt(orc.conv2d_1x1(np.square(b)[None], np.square(w))[0])


def tail_ref(x, sd, p, pool):
    """mff.fn.net.1.net.0 -> net.1.net.1 -> GELU -> net.3 [-> maxpool2] from the net.0 tap, the bounds composed.  Two kinds
    of error are carried apart: rounding and split errors (independent from one hidden channel to the next: _rss through a
    linear layer) and the systematic error of gelu_fast (the same function of x in every channel: conv(b, |w|))."""
    y, rnd = depthwise_ref(x, sd[p + ".net.1.net.0.weight"], sd[p + ".net.1.net.0.bias"])
    w1, s1, sh1 = _bias_layer(sd, p + ".net.1.net.1")
    pre, own = L.pre_activation(y, w1, s1, sh1, True)
    rnd = own + _rss(rnd, w1)
    y = orc.gelu_erf(pre)
    rnd, sys = L.GELU_SLOPE * rnd, L.GELU_ERR * np.abs(pre)
    w3, s3, sh3 = _bias_layer(sd, p + ".net.3")
    pre, own = L.pre_activation(y, w3, s3, sh3, True, b_in=sys)
    y, b = L.activate(pre, own + _rss(rnd, w3), "none")
    return L.post_op(y, b, "pool" if pool else None)


def tail_peak(x, sd, p):
    """the largest |depthwise output|, |pre-GELU| and |GELU output| of the float64 tail: what reaches the fp16 hi halves"""
    x = np.asarray(x, np.float64)[None]
    y = orc.dwconv2d_3x3(x, sd[p + ".net.1.net.0.weight"].astype(np.float64), sd[p + ".net.1.net.0.bias"].astype(np.float64))
    pre = orc.conv2d_1x1(y, sd[p + ".net.1.net.1.weight"].astype(np.float64), sd[p + ".net.1.net.1.bias"].astype(np.float64))
    return float(max(np.abs(y).max(), np.abs(pre).max(), np.abs(orc.gelu_erf(pre)).max()))


class Tail(Stage):
    def __init__(self, name, srcs, launch, prefix, pool):
        super().__init__(name, srcs, launch)
        self.prefix, self.pool = prefix, pool

    def ref(self, inputs, sd, split):
        return tail_ref(inputs[0], sd, self.prefix, self.pool)

    def shape(self, shapes):
        c, h, w = shapes[0]
        return (c // 2, h // 2, w // 2) if self.pool else (c // 2, h, w)


# ---------------------------------------------------------------------------------------------------------------------
# the graph of one module (Plan::attention_module, in launch order)
# ---------------------------------------------------------------------------------------------------------------------
FUSED_ONLY = (".mff",)                                            # stages of the one-launch MixFFN tail
UNFUSED_ONLY = (".mff.fn.net.1.net.0", ".mff.fn.net.1.net.1", ".mff.fn.net.3")


def add_module(g, p, src, pool):
    """p = "seg_head.convs.1"; src = the tap the module reads.  Both MixFFN paths: the three launches (net.1.net.0,
    net.1.net.1, net.3) and the fused tail, whose output is the module's ".mff" tap (which the next layer reads on both)."""
    pw = lambda name, s, **kw: g.__setitem__(name, L.Spec(name, [(s, None)], bn=False, **kw))
    g[p + ".att.norm"] = LayerNorm(p + ".att.norm", [(src, None)])
    pw(p + ".att.fn.to_q", p + ".att.norm", act="none")
    pw(p + ".att.fn.to_kv", p + ".att.norm", act="none")
    g[p + ".att.fn"] = Attention(p + ".att.fn", [(p + ".att.fn.to_q", None), (p + ".att.fn.to_kv", None)])
    pw(p + ".att.fn.to_out", p + ".att.fn", act="none")
    g[p + ".mff.norm"] = LayerNorm(p + ".mff.norm", [(p + ".att.fn.to_out", None)])
    pw(p + ".mff.fn.net.0", p + ".mff.norm", act="none")
    g[p + ".mff.fn.net.1.net.0"] = Depthwise(p + ".mff.fn.net.1.net.0", [(p + ".mff.fn.net.0", None)])
    pw(p + ".mff.fn.net.1.net.1", p + ".mff.fn.net.1.net.0", act="gelu")
    pw(p + ".mff.fn.net.3", p + ".mff.fn.net.1.net.1", act="none", post="pool" if pool else None)
    g[p + ".mff"] = Tail(p + ".mff", [(p + ".mff.fn.net.0", None)], p + ".mff.fn.net.1-3", p + ".mff.fn", pool)


def is_head_family(kernel):
    return kernel.startswith(L.HEAD_FAMILIES)


# ---------------------------------------------------------------------------------------------------------------------
# the GPU cases (tests/test_gpu_attention_head_fp64.py).  forms: the attention launch of (module 1, module 2) in f16x3, as
# (attention_form.h kernel, template instance, XCD-affine grid) — tests/test_attention_head_ref_cpu.py evaluates
# choose_attention for every row and checks that the table reaches each of the four.
# ---------------------------------------------------------------------------------------------------------------------
KSPLIT, SPLIT256, SPLIT256_AFFINE, SPLIT512_AFFINE = ("ksplit", 0, False), ("split", 256, False), ("split", 256, True), ("split", 512, True)


class HeadCase(L.Case):
    def __init__(self, cid, config, v3, ncls, B, H, W, frames, options, forms, why):
        super().__init__(cid, config, v3, ncls, B, H, W, frames, options, variants=None)
        self.forms, self.why = forms, why

    def maps(self, downsample):
        """[(h, w)] of the two modules"""
        h, w = self.H >> downsample, self.W >> downsample
        return [(h, w), (h // 2, w // 2)]


CASES = [
    HeadCase("A_S_A_v3_80x112", "S_A", True, 19, 1, 80, 112, [0], {"lanes": 1}, (KSPLIT, SPLIT256),
             "module 1 on 20 x 28: S = 560, T = 140: key-split attention, a ragged last 32-query group (560 = 17 * 32 + 16), "
             "140 keys at 64 per wave (the third wave has 12 of them in a ragged 32-key tile, the fourth none); mff_tail on 2 x 2 "
             "ragged tiles with the pool.  "
             "Module 2 on 10 x 14: S = 140, T = 35: split<256> on the plain grid (heads * B = 4); one ragged tile, no pool"),
    HeadCase("B_S_A_v2_72x88", "S_A", False, 28, 2, 72, 88, [0, 1], {"lanes": 1}, (SPLIT256_AFFINE, SPLIT256_AFFINE),
             "module 1 on 18 x 22: split<256> on the XCD-affine grid (heads * B = 8).  Module 2 on the odd 9 x 11 map: to_kv drops "
             "the last row and column (T = 4 * 5 = 20)"),
    HeadCase("B_unfused", "S_A", False, 28, 2, 72, 88, [0, 1], {"lanes": 1, "mff_fused": 0}, (SPLIT256_AFFINE, SPLIT256_AFFINE),
             "f16x3 three-launch MixFFN at C = 64: dwconv3x3 with both frames inside one 256-thread block's descriptor "
             "(module 2: 99 pixels a frame), 1x1 + gelu_fast, 1x1 with the pooled store"),
    HeadCase("C_S_A_v3_30x136x136", "S_A", True, 19, 30, 136, 136, [0, 29], {"lanes": 1}, (SPLIT512_AFFINE, SPLIT256_AFFINE),
             "module 1 on 34 x 34: 9 tiles x 30 frames = 270 mff_tail tiles, more than the chip has CUs: workgroups walk a second "
             "tile.  Attention split<512> (5 x 4 x 30 = 600 >= 512 workgroups), affine.  Module 2 on the odd 17 x 17 map"),
    HeadCase("D_N_A_v3_72x88", "N_A", True, 19, 2, 72, 88, [0, 1], {"lanes": 1}, (SPLIT256_AFFINE, SPLIT256_AFFINE),
             "C = 48: the wave-per-pixel LayerNorm, head dim 12, 48 / 96-channel 1x1 layers, MixFFN never fused"),
]
TAIL_TILES_C = 9 * 30      # case C, module 1: must exceed the device's multi_processor_count
