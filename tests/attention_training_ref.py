"""float64 numpy oracle of the attention head's training step (nano_vs_slam_amd.attention_training, train_ops' stage calls,
csrc/attention_train.hip): the reference's SegFormerAttentionModule stage by stage (channel LayerNorm, to_q 1 x 1, to_kv 2 x 2
stride 2, four-head softmax attention, to_out, LayerNorm, 1 x 1, depthwise 3 x 3, 1 x 1, exact GELU, 1 x 1; no residuals)
forward and backward by the formulas of include/kp2d.h, the V2 SegmentationHeadATT around two of them (the Conv + BatchNorm
layers, pooling, pixel shuffle and losses come from seg_training_ref / depth_training_ref), and Adam.  Also the seeded inputs of
the cases: fixtures under tests/golden/attention_training/ hold outputs, settings and seeds only (written by
tools/make_attention_training_golden.py from the reference's own modules under torch autograd); the inputs are regenerated
here from seeds.json.
"""
import json
import math
import os

import numpy as np

import augment_ref as aug
import depth_training_ref as dr
import seg_training_ref as sr

hr, vr = sr.hr, sr.vr
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_training")
HEADS, LN_EPS, SLOPE, LR = 4, 1e-5, sr.SLOPE, 1e-4
FLOOR = sr.FLOOR
stored = sr.stored


def rel_err(g, g64):
    """E(G) = max|G - G64| / max|G64|; of a tensor that is zero everywhere (one key: dQ, dK and to_q's gradient): 0 when G is
    zero everywhere too, else infinity."""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    top, diff = float(np.abs(g64).max()), float(np.abs(g - g64).max())
    return diff / top if top > 0 else (0.0 if diff == 0 else float("inf"))

# name -> (frames, channels, H, W): the smallest shapes at which the kernels can go wrong (tiles of 16 queries and 16 keys,
# 64 pixels per pointwise block, slabs of at least 64 pixels)
MODULE_CASES = {
    "A": (1, 64, 4, 6),         # under every tile
    "B": (2, 64, 15, 20),       # odd height: the last row feeds no key
    "C": (3, 48, 18, 26),       # head dimension 12; hidden 96
    "D": (1, 64, 2, 2),         # one key
    "E": (2, 64, 34, 50),       # several query and key tiles, ragged last tiles on both axes
}
# name -> (N, c_in, c_hidden, d1, c_skip, classes, h, w, loss)
HEAD_CASES = {
    "seg": (2, 64, 64, 128, 64, 28, 8, 12, "seg"),
    "odd": (2, 64, 64, 128, 64, 28, 10, 14, "seg"),        # pooled 5 x 7, odd both ways
    "depth": (2, 64, 64, 128, 64, 1, 8, 12, "depth"),
}
BASE_SEED = {"A": 601, "B": 602, "C": 603, "D": 604, "E": 605, "seg": 611, "odd": 612, "depth": 613, "pair": 621}
TRAJECTORY_STEPS = 5
PAIR_STEPS, PAIR_FRAMES, PAIR_IMAGE, CROSS_WEIGHT = 3, 1, (32, 48), 0.5     # the depth trainer's pair step: one frame per view
NEAREST_SAFE = 1e-3          # pixels: every nearest decision of a kept pair seed is further than this from a tie
TRAJ_STORED = sr.TRAJ_STORED
MODULE_PARAMS = ("att.fn.to_q.weight", "att.fn.to_kv.weight", "att.fn.to_out.weight", "att.norm.g", "att.norm.b", "mff.fn.net.0.weight",
                 "mff.fn.net.0.bias", "mff.fn.net.1.net.0.weight", "mff.fn.net.1.net.0.bias", "mff.fn.net.1.net.1.weight",
                 "mff.fn.net.1.net.1.bias", "mff.fn.net.3.weight", "mff.fn.net.3.bias", "mff.norm.g", "mff.norm.b")
HEAD_PARAMS = tuple(f"convs.0.{p}" for p in ("conv.weight", "bn.weight", "bn.bias")) + tuple(f"convs.{i}.{p}" for i in (1, 2) for p in MODULE_PARAMS) + \
    tuple(f"convs.{i}.{p}" for i in (3, 4, 5, 6) for p in ("conv.weight", "bn.weight", "bn.bias")) + ("convs.7.weight", "convs.7.bias")
MODULE_MAPS = ("n1", "q", "kv", "o", "lse", "a", "n2", "h0", "h1", "pre", "h2", "y")
MODULE_DMAPS = ("d_h2", "d_pre", "d_h1", "d_h0", "d_n2", "d_a", "d_o", "d_q", "d_kv", "d_n1", "dx")
HEAD_MAPS = ("y0", "m1", "pooled", "m2", "y3", "y4", "y5", "y6", "logits")
MIN_S = 0.05        # LayerNorm's sqrt(var) stays above this in every pinned case


def seed_of(name):
    with open(os.path.join(GOLDEN, "seeds.json")) as f:
        return int(json.load(f)[name])


def module_params(rng, C):
    """The 15 float32 arrays of a SegFormerAttentionModule(C) in MODULE_PARAMS order."""
    f = lambda *s, scale=1.0: (rng.standard_normal(s) * scale).astype(np.float32)
    g = lambda: rng.uniform(0.5, 1.5, (1, C, 1, 1)).astype(np.float32)
    b = lambda: f(1, C, 1, 1, scale=0.2)
    h = 2 * C
    return [f(C, C, 1, 1, scale=1.5 / math.sqrt(C)), f(2 * C, C, 2, 2, scale=1.5 / math.sqrt(4 * C)), f(C, C, 1, 1, scale=1.0 / math.sqrt(C)),
            g(), b(), f(h, C, 1, 1, scale=1.0 / math.sqrt(C)), f(h, scale=0.2), f(h, 1, 3, 3, scale=1.0 / 3.0), f(h, scale=0.2),
            f(h, h, 1, 1, scale=1.0 / math.sqrt(h)), f(h, scale=0.2), f(C, h, 1, 1, scale=1.0 / math.sqrt(h)), f(C, scale=0.2), g(), b()]


def make_module_inputs(name, seed=None):
    N, C, H, W = MODULE_CASES[name]
    rng = np.random.default_rng(seed_of(name) if seed is None else seed)
    x = (rng.standard_normal((N, C, H, W)) + 0.3 * rng.standard_normal((N, C, 1, 1))).astype(np.float32)
    dy = rng.standard_normal((N, C, H, W)).astype(np.float32)
    return {"x": x, "dy": dy, "params": module_params(rng, C), "N": N, "C": C, "H": H, "W": W}


def layer_channels(c_in, c_hidden, d1, c_skip, classes):
    """(Cin, Cout) of the six convolution layers: convs 0, 3, 4, 5, 6 and 7."""
    return ((c_in, c_hidden), (c_hidden, d1), (c_hidden + d1 // 4, c_hidden), (c_hidden, d1), (d1 // 4 + c_skip, c_hidden), (c_hidden, classes))


def make_head_inputs(name, seed=None, frames=None):
    """-> dict: x, skip (float32), target (labels uint8 [N, 2h, 2w] or depth float32), params (47 arrays in HEAD_PARAMS order),
    stats {layer: (running_mean, running_var)}, and the sizes."""
    N, c_in, c_hidden, d1, c_skip, classes, h, w, loss = HEAD_CASES[name]
    N = N if frames is None else frames
    rng = np.random.default_rng(seed_of(name) if seed is None else seed)
    x = (np.abs(rng.standard_normal((N, c_in, h, w))) * 0.8 + 0.3 * rng.standard_normal((N, c_in, 1, 1))).astype(np.float32)
    skip = (np.abs(rng.standard_normal((N, c_skip, 2 * h, 2 * w))) * 0.8 + 0.3 * rng.standard_normal((N, c_skip, 1, 1))).astype(np.float32)
    if loss == "seg":
        target = rng.integers(0, classes, (N, 2 * h, 2 * w)).astype(np.uint8)
        target[rng.random(target.shape) < 0.1] = sr.IGNORE
    else:
        target = rng.uniform(0.05, 1.0, (N, 2 * h, 2 * w)).astype(np.float32)
        target[rng.random(target.shape) < 0.1] = 0.0
    convs, stats = [], {}
    for i, (ci, co) in zip((0, 3, 4, 5, 6, 7), layer_channels(c_in, c_hidden, d1, c_skip, classes)):
        wgt = (rng.standard_normal((co, ci, 3, 3)) * math.sqrt(2.0 / (9 * ci))).astype(np.float32)
        if i < 7:
            stats[i] = ((0.3 * rng.standard_normal(co)).astype(np.float32), rng.uniform(0.5, 1.5, co).astype(np.float32))
            convs.append([wgt, rng.uniform(0.5, 1.5, co).astype(np.float32), (0.2 * rng.standard_normal(co)).astype(np.float32)])
        else:
            convs.append([wgt, (0.2 * rng.standard_normal(co)).astype(np.float32)])
    params = convs[0] + module_params(rng, c_hidden) + module_params(rng, c_hidden) + convs[1] + convs[2] + convs[3] + convs[4] + convs[5]
    return {"x": x, "skip": skip, "target": target, "params": params, "stats": stats, "loss": loss, "N": N, "c_in": c_in, "c_hidden": c_hidden,
            "d1": d1, "c_skip": c_skip, "classes": classes, "h": h, "w": w}


def make_pair_inputs(seed=None):
    """The depth case's head on a view pair of PAIR_FRAMES frames -> make_head_inputs' dict (x, skip, target of the plain view)
    plus x_aug, skip_aug, gt (= target), gt_aug (gt under the homography, what view_pair hands the trainer), homography
    float32 [N, 3, 3] in normalised coordinates, and weights."""
    seed = seed_of("pair") if seed is None else seed
    inp = make_head_inputs("depth", seed, frames=PAIR_FRAMES)
    rng = np.random.default_rng(seed + 1)
    N = PAIR_FRAMES
    inp["x_aug"] = (np.abs(rng.standard_normal(inp["x"].shape)) * 0.8 + 0.3 * rng.standard_normal((N, inp["c_in"], 1, 1))).astype(np.float32)
    inp["skip_aug"] = (np.abs(rng.standard_normal(inp["skip"].shape)) * 0.8 + 0.3 * rng.standard_normal((N, inp["c_skip"], 1, 1))).astype(np.float32)
    draws = np.empty((N, aug.SLOTS))
    draws[:, list(aug.NORMAL_SLOTS)] = rng.standard_normal((N, len(aug.NORMAL_SLOTS)))
    draws[:, [4, 6, 7, 8]] = rng.random((N, 4))
    inp["homography"] = aug.sample_homographies(draws, PAIR_IMAGE).astype(np.float32)
    inp["gt"] = inp["target"]
    inp["gt_aug"] = aug.warp(inp["gt"][:, None], inp["homography"].astype(np.float64), fill=0.0)[:, 0].astype(np.float32)
    inp["weights"] = dr.WEIGHTS
    return inp


# ---- the stages ----------------------------------------------------------------------------------------------------------------
def _f(*ts):
    return [np.asarray(t, np.float64) for t in ts]


def layernorm(x, g, b, eps=LN_EPS):
    """-> (y, mean [N, H, W], rinv = 1 / (sqrt(var) + eps) [N, H, W])"""
    x, g, b = _f(x, g, b)
    mean = x.mean(axis=1)
    s = np.sqrt(((x - mean[:, None]) ** 2).mean(axis=1))
    rinv = 1.0 / (s + eps)
    return (x - mean[:, None]) * rinv[:, None] * g.reshape(1, -1, 1, 1) + b.reshape(1, -1, 1, 1), mean, rinv


def layernorm_backward(x, g, dy, eps=LN_EPS):
    """-> (dx, dg, db); a pixel with sqrt(var) = 0 takes the term through the deviation as 0"""
    x, g, dy = _f(x, g, dy)
    C = x.shape[1]
    d = x - x.mean(axis=1, keepdims=True)
    s = np.sqrt((d ** 2).mean(axis=1, keepdims=True))
    D = s + eps
    a = g.reshape(1, -1, 1, 1) * dy
    k = np.divide((a * d).sum(axis=1, keepdims=True), C * s * D * D, out=np.zeros_like(s), where=s > 0)
    dx = (a - a.mean(axis=1, keepdims=True)) / D - d * k
    return dx, (dy * d / D).sum(axis=(0, 2, 3)).reshape(g.shape), dy.sum(axis=(0, 2, 3)).reshape(g.shape)


def pointwise(x, w, bias=None):
    x, w = _f(x, w)
    y = np.einsum("oc,nchw->nohw", w[:, :, 0, 0], x)
    return y if bias is None else y + np.asarray(bias, np.float64).reshape(1, -1, 1, 1)


def pointwise_backward(x, w, dy):
    """-> (dx, dw, dbias)"""
    x, w, dy = _f(x, w, dy)
    return np.einsum("oc,nohw->nchw", w[:, :, 0, 0], dy), np.einsum("nohw,nchw->oc", dy, x)[:, :, None, None], dy.sum(axis=(0, 2, 3))


def _patches(x):
    N, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    return x[:, :, :2 * Ho, :2 * Wo].reshape(N, C, Ho, 2, Wo, 2)


def patch2(x, w):
    x, w = _f(x, w)
    return np.einsum("ocab,nciajb->noij", w, _patches(x))


def patch2_backward(x, w, dy):
    """-> (dx with zeros where no patch reaches, dw)"""
    x, w, dy = _f(x, w, dy)
    N, C, H, W = x.shape
    dx = np.zeros_like(x)
    dx[:, :, :2 * (H // 2), :2 * (W // 2)] = np.einsum("ocab,noij->nciajb", w, dy).reshape(N, C, 2 * (H // 2), 2 * (W // 2))
    return dx, np.einsum("noij,nciajb->ocab", dy, _patches(x))


def _shifted(x):
    """The nine 3 x 3 taps' views of x with padding 1, row-major."""
    H, W = x.shape[2:]
    p = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    return [p[:, :, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)]


def dwconv3(x, w, bias):
    x, w, bias = _f(x, w, bias)
    return sum(w[:, 0, t // 3, t % 3].reshape(1, -1, 1, 1) * v for t, v in enumerate(_shifted(x))) + bias.reshape(1, -1, 1, 1)


def dwconv3_backward(x, w, dy):
    """-> (dx, dw [C, 1, 3, 3], dbias)"""
    x, w, dy = _f(x, w, dy)
    dw = np.stack([(dy * v).sum(axis=(0, 2, 3)) for v in _shifted(x)], axis=1).reshape(-1, 1, 3, 3)
    dx = sum(w[:, 0, 2 - t // 3, 2 - t % 3].reshape(1, -1, 1, 1) * v for t, v in enumerate(_shifted(dy)))
    return dx, dw, dy.sum(axis=(0, 2, 3))


_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(v):
    v = np.asarray(v, np.float64)
    return 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))


def gelu_backward(v, dy):
    v, dy = _f(v, dy)
    return dy * (0.5 * (1.0 + _erf(v / math.sqrt(2.0))) + v * np.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi))


def _heads(t):
    """[N, C, H, W] -> [N, HEADS, H W, C / HEADS]"""
    N, C, H, W = t.shape
    return t.reshape(N, HEADS, C // HEADS, H * W).transpose(0, 1, 3, 2)


def _unheads(t, H, W):
    N, _, S, hd = t.shape
    return t.transpose(0, 1, 3, 2).reshape(N, HEADS * hd, H, W)


def _probabilities(q, kv):
    C = q.shape[1]
    qh, kh, vh = _heads(q), _heads(kv[:, :C]), _heads(kv[:, C:])
    sim = np.einsum("nhic,nhjc->nhij", qh, kh) * (C // HEADS) ** -0.5
    m = sim.max(axis=3, keepdims=True)
    e = np.exp(sim - m)
    l = e.sum(axis=3, keepdims=True)
    return qh, kh, vh, e / l, (m + np.log(l))[..., 0]


def attention(q, kv):
    """-> (o [N, C, H, W], lse [N, HEADS, H W])"""
    q, kv = _f(q, kv)
    qh, kh, vh, p, lse = _probabilities(q, kv)
    return _unheads(np.einsum("nhij,nhjc->nhic", p, vh), *q.shape[2:]), lse


def attention_backward(q, kv, do):
    """-> (dq, dkv)"""
    q, kv, do = _f(q, kv, do)
    C = q.shape[1]
    qh, kh, vh, p, _ = _probabilities(q, kv)
    doh = _heads(do)
    dv = np.einsum("nhij,nhic->nhjc", p, doh)
    dp = np.einsum("nhic,nhjc->nhij", doh, vh)
    ds = p * (dp - (p * dp).sum(axis=3, keepdims=True))
    scale = (C // HEADS) ** -0.5
    dq = np.einsum("nhij,nhjc->nhic", ds, kh) * scale
    dk = np.einsum("nhij,nhic->nhjc", ds, qh) * scale
    return _unheads(dq, *q.shape[2:]), np.concatenate([_unheads(dk, *kv.shape[2:]), _unheads(dv, *kv.shape[2:])], axis=1)


# ---- one module ------------------------------------------------------------------------------------------------------------------
def module_forward(x, p):
    """-> dict of MODULE_MAPS (and x)"""
    s = {"x": np.asarray(x, np.float64)}
    s["n1"], s["mean1"], s["rinv1"] = layernorm(s["x"], p[3], p[4])
    s["q"] = pointwise(s["n1"], p[0])
    s["kv"] = patch2(s["n1"], p[1])
    s["o"], s["lse"] = attention(s["q"], s["kv"])
    s["a"] = pointwise(s["o"], p[2])
    s["n2"], s["mean2"], s["rinv2"] = layernorm(s["a"], p[13], p[14])
    s["h0"] = pointwise(s["n2"], p[5], p[6])
    s["h1"] = dwconv3(s["h0"], p[7], p[8])
    s["pre"] = pointwise(s["h1"], p[9], p[10])
    s["h2"] = gelu(s["pre"])
    s["y"] = pointwise(s["h2"], p[11], p[12])
    return s


def module_backward(s, p, dy):
    """``module_forward``'s dict and the gradient of y -> (dict of MODULE_DMAPS, the 15 gradients in MODULE_PARAMS order)"""
    g, d = [None] * 15, {}
    d["d_h2"], g[11], g[12] = pointwise_backward(s["h2"], p[11], dy)
    d["d_pre"] = gelu_backward(s["pre"], d["d_h2"])
    d["d_h1"], g[9], g[10] = pointwise_backward(s["h1"], p[9], d["d_pre"])
    d["d_h0"], g[7], g[8] = dwconv3_backward(s["h0"], p[7], d["d_h1"])
    d["d_n2"], g[5], g[6] = pointwise_backward(s["n2"], p[5], d["d_h0"])
    d["d_a"], g[13], g[14] = layernorm_backward(s["a"], p[13], d["d_n2"])
    d["d_o"], g[2], _ = pointwise_backward(s["o"], p[2], d["d_a"])
    d["d_q"], d["d_kv"] = attention_backward(s["q"], s["kv"], d["d_o"])
    dn_q, g[0], _ = pointwise_backward(s["n1"], p[0], d["d_q"])
    dn_kv, g[1] = patch2_backward(s["n1"], p[1], d["d_kv"])
    d["d_n1"] = dn_q + dn_kv
    d["dx"], g[3], g[4] = layernorm_backward(s["x"], p[3], d["d_n1"])
    return d, g


def module_step(inp, params=None):
    p = inp["params"] if params is None else params
    s = module_forward(inp["x"], p)
    d, g = module_backward(s, p, inp["dy"])
    s.update(d)
    s["grads"] = g
    return s


# ---- the head ----------------------------------------------------------------------------------------------------------------------
SLOT = {0: 0, 3: 33, 4: 36, 5: 39, 6: 42}       # a Conv + BatchNorm layer's first parameter in HEAD_PARAMS order


def head_loss(inp, logits):
    """-> (loss, dlogits)"""
    if inp["loss"] == "seg":
        ls = sr.seg_loss(logits, inp["target"])
        return ls["loss"], ls["dz"]
    ls = dr.depth_loss(logits[:, 0], inp["target"])
    return ls["loss"], ls["dz"][:, None]


def head_step(inp, params=None, x=None, skip=None, loss_fn=None):
    """One forward, loss and backward of the SegmentationHeadATT in .eval() -> dict: HEAD_MAPS, loss, dlogits, grads (47).
    ``x``, ``skip``: other maps than the case's; ``loss_fn(logits) -> (loss, dlogits)``: another loss (the pair step's)."""
    p = inp["params"] if params is None else params
    x, skip = _f(inp["x"] if x is None else x, inp["skip"] if skip is None else skip)
    f, acts = {}, {}

    def cbr(i, v):
        w, gamma, beta = p[SLOT[i]:SLOT[i] + 3]
        y, c, scale, invstd = hr.cbr_forward(v, w, gamma, beta, inp["stats"][i][0], inp["stats"][i][1], SLOPE)
        acts[i] = (np.asarray(v, np.float64), y, c, scale, invstd)
        return y

    f["y0"] = cbr(0, x)
    s1 = module_forward(f["y0"], p[3:18])
    f["m1"] = s1["y"]
    f["pooled"], _ = sr.maxpool2(f["m1"])
    s2 = module_forward(f["pooled"], p[18:33])
    f["m2"] = s2["y"]
    f["y3"] = cbr(3, f["m2"])
    f["y4"] = cbr(4, sr.shuffle_cat(f["y3"], x))
    f["y5"] = cbr(5, f["y4"])
    f["y6"] = cbr(6, sr.shuffle_cat(f["y5"], skip))
    f["logits"] = sr.conv_bias(f["y6"], p[45], p[46])
    f["loss"], f["dlogits"] = head_loss(inp, f["logits"]) if loss_fn is None else loss_fn(f["logits"])
    g = [None] * 47
    g[45], g[46], dy = sr.conv_bias_backward(f["y6"], p[45], f["dlogits"])

    def back(i, dy, need_dx=True):
        lx, y, c, scale, invstd = acts[i]
        dw, dgamma, dbeta, dx = hr.cbr_backward(lx, p[SLOT[i]], scale, inp["stats"][i][0], invstd, SLOPE, y, c, dy, need_dx)
        g[SLOT[i]:SLOT[i] + 3] = [dw, dgamma, dbeta]
        return dx

    dy = back(6, dy)
    dy = back(5, sr.shuffle_cat_backward(dy, inp["d1"] // 4))
    dy = back(4, dy)
    dy = back(3, sr.shuffle_cat_backward(dy, inp["d1"] // 4))
    d2, g[18:33] = module_backward(s2, p[18:33], dy)
    d1, g[3:18] = module_backward(s1, p[3:18], sr.maxpool2_backward(f["m1"], d2["dx"]))
    back(0, d1["dx"], need_dx=False)
    f["grads"] = g
    f["min_s"] = min(float((1.0 / s[k] - LN_EPS).min()) for s in (s1, s2) for k in ("rinv1", "rinv2"))
    return f


def pair_step(inp, params=None, cross_weight=CROSS_WEIGHT):
    """DepthHeadTrainer.pair_gradients: both views through the head as one batch under
    L(z, gt) + L(z_aug, gt_aug) + cross_weight MSE(sigmoid(z_aug), warp(sigmoid(z)))."""
    N = inp["x"].shape[0]
    hom = inp["homography"].astype(np.float64)

    def loss_fn(logits):
        z, za = logits[:N, 0], logits[N:, 0]
        l0, l1 = dr.depth_loss(z, inp["gt"], inp["weights"]), dr.depth_loss(za, inp["gt_aug"], inp["weights"])
        pr, pa = 1.0 / (1.0 + np.exp(-z)), 1.0 / (1.0 + np.exp(-za))
        cv = aug.cross_view_mse(pr, pa, hom, 1.0)
        dz = np.concatenate([l0["dz"] + cross_weight * cv["d_depth"] * pr * (1.0 - pr), l1["dz"] + cross_weight * cv["d_depth_aug"] * pa * (1.0 - pa)])
        return (l0["loss"] + l1["loss"]) + cross_weight * cv["loss"], dz[:, None]

    return head_step(inp, params, np.concatenate([inp["x"], inp["x_aug"]]), np.concatenate([inp["skip"], inp["skip_aug"]]), loss_fn)


def trajectory(inp, steps=TRAJECTORY_STEPS, lr=LR, step_fn=None, keep_grads=False):
    """Adam on one batch over all 47 parameters -> (losses [steps], the parameters after every step[, the gradients of every
    step]); ``step_fn``: head_step or pair_step."""
    params = [a.astype(np.float64) for a in inp["params"]]
    opt = vr.Adam(params, lr=lr)
    losses, after, grads = [], [], []
    for _ in range(steps):
        s = (step_fn or head_step)(inp, params)
        losses.append(s["loss"])
        grads.append([np.asarray(g).reshape(a.shape).copy() for g, a in zip(s["grads"], params)])
        opt.step(grads[-1])
        after.append([a.copy() for a in params])
    return (np.asarray(losses), after, grads) if keep_grads else (np.asarray(losses), after)


def sign_driven(grads, i, gradient_bound):
    """The elements of parameter i whose oracle gradient at one of the given steps lies below the bound of that gradient
    (|g| < gradient_bound max|g|): a device gradient within its bound may differ there by its own size or have the other
    sign, and Adam's first steps move by lr g / (|g| + eps) - by the sign of g, not by its size (vlad_training_ref's rule)."""
    mask = np.zeros(grads[0][i].shape, bool)
    for step in grads:
        mask |= np.abs(step[i]) < gradient_bound * np.abs(step[i]).max()
    return mask


def load_fixture(name):
    return np.load(os.path.join(GOLDEN, f"case_{name}.npz"))


def load_trajectory(name):
    return np.load(os.path.join(GOLDEN, f"trajectory_{name}.npz"))


def bound(fixture, key):
    """The bound on E = max|G - G64| / max|G64| of one quantity of one fixture: max(8 x the reference modules' own float32
    error of it, 16 x 2^-24)."""
    return max(8.0 * float(fixture["err32_" + key]), FLOOR)
