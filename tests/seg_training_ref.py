"""float64 numpy oracle of the segmentation head's training step (nano_vs_slam_amd.seg_training, csrc/seg_train.hip and
csrc/vpr_head_train.hip): the V2 SegmentationHead in .eval() (eight Conv + BatchNorm + (Leaky)ReLU layers from
vpr_head_training_ref, 2 x 2 max pooling, pixel shuffle + concatenation, the last 3 x 3 convolution with bias), the loss
ce_weight CE + dice_weight Dice by the formulas of include/kp2d.h, their gradients, and Adam.  Also the seeded inputs of
the test cases: fixtures under tests/golden/seg_training/ hold outputs and settings only (written by
tools/make_seg_training_golden.py from the reference's SegmentationHead under torch autograd); the inputs are regenerated
here from the seeds that generator kept (seeds.json).
"""
import json
import os

import numpy as np

import vpr_head_training_ref as hr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_training")
vr = hr.vr

# name -> (N, c_in, c_hidden, d1, c_skip, classes, h, w, (ce_weight, dice_weight), inputs of): the smallest shapes at which
# the kernels can go wrong; the conv tile is 8 rows x 16 columns
CASES = {
    "A": (2, 16, 16, 64, 16, 5, 6, 10, (0.5, 1.5), "A"),      # fewer than 16 classes; ragged tiles; about 10 % ignored labels
    "B": (3, 16, 16, 64, 16, 19, 10, 18, (0.5, 1.5), "B"),    # classes across a 16 boundary; odd pooled map 5 x 9; frame 2 wholly
                                                               # ignored; class 18 absent from every label
    "Bce": (3, 16, 16, 64, 16, 19, 10, 18, (1.0, 0.0), "B"),  # the same inputs under CE alone, which torch alone pins
    "C": (2, 64, 64, 128, 64, 28, 4, 6, (0.5, 1.5), "C"),     # config S's channel counts: 96-channel concatenations, Cout 128
    "D": (1, 16, 16, 64, 16, 2, 2, 2, (0.5, 1.5), "D"),       # the smallest map: pooled 1 x 1
}
BASE_SEED = {"A": 301, "B": 302, "C": 303, "D": 304}
IGNORE = 255
SLOPE = 0.01
BN_EPS = hr.BN_EPS
LR = 1e-4
TRAJECTORY_CASE, HEAD_STEPS, LAST_STEPS = "A", 10, 3
MAX_STORED = 256        # a fixture keeps at most this many entries of an array (every stride_of(size)-th of the flattened array)
TRAJ_STORED = 64        # and of a parameter along the trajectory
PARAMS = tuple(f"convs.{i}.{p}" for i in range(8) for p in ("conv.weight", "bn.weight", "bn.bias")) + ("convs.8.weight", "convs.8.bias")
MAPS = tuple(f"y{i}" for i in range(8)) + ("pooled", "cat1", "cat2", "logits")
DMAPS = ("dlogits", "d_y7", "d_cat2", "d_y6", "d_y5", "d_cat1", "d_y4", "d_y3", "d_y2", "d_pooled", "d_y1", "d_y0")


def stride_of(size, cap=MAX_STORED):
    st = -(-size // cap)
    return st if st == 1 or st % 2 else st + 1


def stored(a, cap=MAX_STORED):
    a = np.asarray(a)
    return a.ravel()[::stride_of(a.size, cap)]


def layer_channels(c_in, c_hidden, d1, c_skip, classes):
    """(Cin, Cout) of the nine layers."""
    return ((c_in, c_hidden), (c_hidden, c_hidden), (c_hidden, c_hidden), (c_hidden, c_hidden), (c_hidden, d1),
            (c_hidden + d1 // 4, c_hidden), (c_hidden, d1), (d1 // 4 + c_skip, c_hidden), (c_hidden, classes))


def seed_of(name):
    with open(os.path.join(GOLDEN, "seeds.json")) as f:
        return int(json.load(f)[CASES[name][9]])


def make_inputs(name, seed=None):
    """-> dict: x [N, c_in, h, w], skip [N, c_skip, 2h, 2w] (float32), labels [N, 2h, 2w] uint8, params (the 26 float32 arrays
    in PARAMS order), stats [(running_mean, running_var) per BatchNorm layer], weights, and the case's sizes.  About one
    label in ten is IGNORE; case B's last frame is ignored altogether and its last class is drawn nowhere."""
    N, c_in, c_hidden, d1, c_skip, classes, h, w, weights, src = CASES[name]
    rng = np.random.default_rng(seed_of(name) if seed is None else seed)
    x = (np.abs(rng.standard_normal((N, c_in, h, w))) * 0.8 + 0.3 * rng.standard_normal((N, c_in, 1, 1))).astype(np.float32)
    skip = (np.abs(rng.standard_normal((N, c_skip, 2 * h, 2 * w))) * 0.8 + 0.3 * rng.standard_normal((N, c_skip, 1, 1))).astype(np.float32)
    drawn = classes - 1 if src == "B" else classes
    labels = rng.integers(0, drawn, (N, 2 * h, 2 * w)).astype(np.uint8)
    labels[rng.random(labels.shape) < 0.1] = IGNORE
    if src == "B":
        labels[-1] = IGNORE
    params, stats = [], []
    for i, (ci, co) in enumerate(layer_channels(c_in, c_hidden, d1, c_skip, classes)):
        wgt = (rng.standard_normal((co, ci, 3, 3)) * np.sqrt(2.0 / (9 * ci))).astype(np.float32)
        if i < 8:
            gamma, beta = rng.uniform(0.5, 1.5, co), 0.2 * rng.standard_normal(co)
            stats.append(((0.3 * rng.standard_normal(co)).astype(np.float32), rng.uniform(0.5, 1.5, co).astype(np.float32)))
            params += [wgt, gamma.astype(np.float32), beta.astype(np.float32)]
        else:
            params += [wgt, (0.2 * rng.standard_normal(co)).astype(np.float32)]
    return {"x": x, "skip": skip, "labels": labels, "params": params, "stats": stats, "weights": weights, "N": N, "c_in": c_in,
            "c_hidden": c_hidden, "d1": d1, "c_skip": c_skip, "classes": classes, "h": h, "w": w}


# ---- the scale changes ---------------------------------------------------------------------------------------------------
def _windows(x):
    N, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    return x[:, :, :2 * Ho, :2 * Wo].reshape(N, C, Ho, 2, Wo, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, Ho, Wo, 4)


def maxpool2(x):
    """-> (y, argmax in the window's row-major order; np.argmax takes the first maximum, torch's rule)"""
    win = _windows(np.asarray(x))
    return win.max(axis=4), win.argmax(axis=4)


def maxpool2_backward(x, dy):
    x = np.asarray(x)
    N, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    _, at = maxpool2(x)
    d = np.zeros((N, C, Ho, Wo, 4), np.asarray(dy).dtype)
    np.put_along_axis(d, at[..., None], np.asarray(dy)[..., None], axis=4)
    dx = np.zeros(x.shape, d.dtype)
    dx[:, :, :2 * Ho, :2 * Wo] = d.reshape(N, C, Ho, Wo, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * Ho, 2 * Wo)
    return dx


def pool_gap(x):
    """The smallest distance between a window's largest and second largest value."""
    s = np.sort(_windows(np.asarray(x, np.float64)), axis=4)
    return float((s[..., 3] - s[..., 2]).min())


def shuffle_cat(a, b):
    a, b = np.asarray(a), np.asarray(b)
    N, C4, h, w = a.shape
    C = C4 // 4
    up = a.reshape(N, C, 2, 2, h, w).transpose(0, 1, 4, 2, 5, 3).reshape(N, C, 2 * h, 2 * w)
    return np.concatenate([up, b], axis=1)


def shuffle_cat_backward(dout, C):
    dout = np.asarray(dout)
    N, _, H, W = dout.shape
    h, w = H // 2, W // 2
    return dout[:, :C].reshape(N, C, h, 2, w, 2).transpose(0, 1, 3, 5, 2, 4).reshape(N, 4 * C, h, w)


# ---- the last layer and the loss ---------------------------------------------------------------------------------------------
def conv_bias(x, w, b):
    return hr.conv3x3(np.asarray(x, np.float64), np.asarray(w, np.float64)) + np.asarray(b, np.float64)[None, :, None, None]


def conv_bias_backward(x, w, dy, need_dx=True):
    x, w, dy = (np.asarray(t, np.float64) for t in (x, w, dy))
    return hr.conv3x3_dw(dy, x), dy.sum(axis=(0, 2, 3)), (hr.conv3x3_dx(dy, w) if need_dx else None)


def seg_loss(z, labels, weights=(0.5, 1.5), ignore=IGNORE, eps=1e-7):
    """include/kp2d.h's kp2d_seg_loss in float64 -> dict(loss, ce, dice, dz, valid, stray, S, present)."""
    z = np.asarray(z, np.float64)
    N, C, H, W = z.shape
    lab = np.asarray(labels).astype(np.int64)
    ignored = np.zeros(lab.shape, bool) if ignore is None else lab == ignore
    stray = ~ignored & ((lab < 0) | (lab >= C))
    ok = ~ignored & ~stray
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    p = e / e.sum(axis=1, keepdims=True)
    logp = (z - m) - np.log(e.sum(axis=1, keepdims=True))
    t = np.zeros(z.shape)
    np.put_along_axis(t, np.where(ok, lab, 0)[:, None], 1.0, axis=1)
    t *= ok[:, None]
    pv = p * ok[:, None]
    V = int(ok.sum())
    ce = -(logp * t).sum() / V if V else 0.0
    I, S, T = (pv * t).sum(axis=(0, 2, 3)), (pv + t).sum(axis=(0, 2, 3)), t.sum(axis=(0, 2, 3))
    present = T > 0
    D = np.maximum(S, eps)
    dice = float((present * (1.0 - 2.0 * I / D)).sum() / C)
    wce, wd = weights
    a = np.where(present, -2.0 / (C * D), 0.0)
    b = np.where(present & (S > eps), 2.0 * I / (C * D * D), 0.0)
    g = a[None, :, None, None] * t + b[None, :, None, None]
    dz = wd * pv * (g - (pv * g).sum(axis=1, keepdims=True))
    if V:
        dz += wce * (pv - t) / V
    return {"loss": wce * ce + wd * dice, "ce": float(ce), "dice": dice, "dz": dz, "valid": V, "stray": int(stray.sum()), "S": S,
            "present": present}


# ---- the step --------------------------------------------------------------------------------------------------------------
def head_forward(inp, params=None, x=None, skip=None):
    """-> dict: acts [(x, y, c, scale, invstd) per BatchNorm layer], y0..y7, pooled, cat1, cat2, logits."""
    params = inp["params"] if params is None else params
    x = np.asarray(inp["x"] if x is None else x, np.float64)
    skip = np.asarray(inp["skip"] if skip is None else skip, np.float64)
    out, acts = {}, []

    def cbr(i, v):
        w, gamma, beta = params[3 * i:3 * i + 3]
        y, c, scale, invstd = hr.cbr_forward(v, w, gamma, beta, inp["stats"][i][0], inp["stats"][i][1], SLOPE)
        acts.append((np.asarray(v, np.float64), y, c, scale, invstd))
        out[f"y{i}"] = y
        return y

    y1 = cbr(1, cbr(0, x))
    out["pooled"], _ = maxpool2(y1)
    y4 = cbr(4, cbr(3, cbr(2, out["pooled"])))
    out["cat1"] = shuffle_cat(y4, x)
    y6 = cbr(6, cbr(5, out["cat1"]))
    out["cat2"] = shuffle_cat(y6, skip)
    y7 = cbr(7, out["cat2"])
    out["logits"] = conv_bias(y7, params[24], params[25])
    out["acts"] = acts
    return out


def step_gradients(inp, params=None, weights=None, x=None, skip=None):
    """One forward / loss / backward -> the forward's dict plus loss, ce, dice, valid, stray, dlogits and the other DMAPS,
    grads (PARAMS order)."""
    params = inp["params"] if params is None else params
    f = head_forward(inp, params, x, skip)
    ls = seg_loss(f["logits"], inp["labels"], inp["weights"] if weights is None else weights)
    f.update({k: ls[k] for k in ("loss", "ce", "dice", "valid", "stray")})
    f["dlogits"] = ls["dz"]
    grads = [None] * 26
    grads[24], grads[25], dy = conv_bias_backward(f["y7"], params[24], ls["dz"])
    f["d_y7"] = dy

    def back(i, dy, need_dx=True):
        lx, y, c, scale, invstd = f["acts"][i]
        dw, dgamma, dbeta, dx = hr.cbr_backward(lx, params[3 * i], scale, inp["stats"][i][0], invstd, SLOPE, y, c, dy, need_dx)
        grads[3 * i:3 * i + 3] = [dw, dgamma, dbeta]
        return dx

    f["d_cat2"] = back(7, dy)
    f["d_y6"] = shuffle_cat_backward(f["d_cat2"], inp["d1"] // 4)
    f["d_y5"] = back(6, f["d_y6"])
    f["d_cat1"] = back(5, f["d_y5"])
    f["d_y4"] = shuffle_cat_backward(f["d_cat1"], inp["d1"] // 4)
    f["d_y3"] = back(4, f["d_y4"])
    f["d_y2"] = back(3, f["d_y3"])
    f["d_pooled"] = back(2, f["d_y2"])
    f["d_y1"] = maxpool2_backward(f["y1"], f["d_pooled"])
    f["d_y0"] = back(1, f["d_y1"])
    back(0, f["d_y0"], need_dx=False)
    f["grads"] = grads
    return f


def loss_from(inp, params, x=None, skip=None):
    f = head_forward(inp, params, x, skip)
    return seg_loss(f["logits"], inp["labels"], inp["weights"])["loss"]


def trajectory(inp, mode="head", steps=None, lr=LR):
    """Adam on one batch over all 26 parameters ("head") or the last layer's two ("last") -> (losses [steps], the trained
    parameters after every step)."""
    steps = (HEAD_STEPS if mode == "head" else LAST_STEPS) if steps is None else steps
    params = [p.astype(np.float64) for p in inp["params"]]
    trained = list(range(26)) if mode == "head" else [24, 25]
    opt = vr.Adam([params[i] for i in trained], lr=lr)
    losses, after = [], []
    for _ in range(steps):
        s = step_gradients(inp, params)
        losses.append(s["loss"])
        opt.step([np.asarray(s["grads"][i]).reshape(params[i].shape) for i in trained])
        after.append([params[i].copy() for i in trained])
    return np.asarray(losses), after


rel_err = vr.rel_err


def load_fixture(name):
    return np.load(os.path.join(GOLDEN, f"case_{name}.npz"))


def load_trajectory():
    return np.load(os.path.join(GOLDEN, "trajectory.npz"))


FLOOR = 16.0 * 2.0 ** -24      # of a tensor's largest magnitude: what fp32 storage and one other order of summation cost


def bounds():
    """-> dict: per quantity (loss, every map of MAPS and DMAPS, g0..g25) the bound on E = max|G - G64| / max|G64| (the loss:
    |loss - loss64| / |loss64|): max(8 x the reference module's own float32 error of that quantity, the maximum over the
    fixture cases, 16 x 2^-24)."""
    fx = [load_fixture(n) for n in CASES]
    keys = ("loss",) + MAPS + DMAPS + tuple(f"g{i}" for i in range(26))
    return {k: max(8.0 * max(float(f["err32_" + k]) for f in fx), FLOOR) for k in keys}


def trajectory_bounds():
    """The same for the trajectory: loss_head, loss_last, and per trained parameter p{i}_head / p{i}_last (the maximum over
    the steps)."""
    fx = load_trajectory()
    return {k[6:]: max(8.0 * float(fx[k]), FLOOR) for k in fx.files if k.startswith("err32_")}
