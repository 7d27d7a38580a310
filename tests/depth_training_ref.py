"""float64 numpy oracle of the depth head's training step (nano_vs_slam_amd.depth_training, csrc/depth_train.hip): the loss
silog_weight SILog + huber_weight Huber and its gradient by the formulas of include/kp2d.h, the whole step over the V2
SegmentationHead with one class (the layer stack is seg_training_ref's, by import), and Adam.  Also the seeded inputs of the
test cases: fixtures under tests/golden/depth_training/ hold outputs and settings only (written by
tools/make_depth_training_golden.py from the reference's SegmentationHead and SILogLoss with torch.nn.HuberLoss under torch
autograd); the inputs are regenerated here from the seeds that generator kept (seeds.json).
"""
import json
import os

import numpy as np

import seg_training_ref as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_training")
hr, vr = sr.hr, sr.vr

SILOG_SCALE, SILOG_LAMBDA, HUBER_DELTA = 10.0, 0.15, 1.0      # KP2D_SILOG_SCALE, KP2D_SILOG_LAMBDA, KP2D_HUBER_DELTA
WEIGHTS = (1.0, 1.0)                                          # the reference: SILog + huber_loss_factor (1.0) Huber

# the loss alone: name -> (N, H, W); a chunk of the kernel is 1024 pixels
LOSS_CASES = {
    "L1": (1, 3, 5),          # a single ragged chunk
    "L2": (3, 17, 23),        # 1173 pixels: ragged against any power-of-two chunk, a frame boundary inside a chunk
    "L3": (5, 41, 53),        # 10865 pixels, 11 chunks; frame 1 wholly invalid, frame 3 with a single valid pixel
    "L4": (2, 17, 23),        # "offset": logits near -20 with a spread of 1e-3, gt near 0.9: mean^2 / var about 2e9
}
# the whole step: name -> (N, c_in, c_hidden, d1, c_skip, h, w): seg_training_ref's channel counts (A, B: its cases A, B, D; C:
# its case C, config S's), so every width the stack uses is walked; the conv tile is 8 rows x 16 columns
STEP_CASES = {
    "A": (2, 16, 16, 64, 16, 4, 6),
    "B": (3, 16, 16, 64, 16, 2, 2),       # the smallest map: pooled 1 x 1
    "C": (2, 64, 64, 128, 64, 6, 10),     # the trajectory case
}
BASE_SEED = {"L1": 401, "L2": 402, "L3": 403, "L4": 404, "A": 411, "B": 412, "C": 413}
SLOPE, BN_EPS, LR = sr.SLOPE, sr.BN_EPS, sr.LR
TRAJECTORY_CASE, HEAD_STEPS, LAST_STEPS = "C", 10, 3
MAX_STORED, TRAJ_STORED = sr.MAX_STORED, sr.TRAJ_STORED
PARAMS, MAPS, DMAPS = sr.PARAMS, sr.MAPS, sr.DMAPS
stride_of, stored, rel_err, FLOOR = sr.stride_of, sr.stored, sr.rel_err, sr.FLOOR
Z_MAX = 8.0             # |logit| in every pinned case but L4: the reference's own log(sigmoid(z)) is then exact to 1e-15


def seed_of(name):
    with open(os.path.join(GOLDEN, "seeds.json")) as f:
        return int(json.load(f)[name])


def _draw_gt(rng, shape):
    """gt from (0, 3], about a quarter of the pixels without ground truth (0 or negative)."""
    gt = (3.0 * (1.0 - rng.random(shape))).astype(np.float32)
    none = rng.random(shape)
    gt[none < 0.25] = 0.0
    gt[none < 0.08] = -1.5
    return gt


def make_loss_inputs(name, seed=None):
    """-> (logits [N, H, W], gt [N, H, W]), float32."""
    N, H, W = LOSS_CASES[name]
    rng = np.random.default_rng(seed_of(name) if seed is None else seed)
    if name == "L4":
        z = (-20.0 + 1e-3 * (rng.random((N, H, W)) - 0.5)).astype(np.float32)
        gt = (0.9 * (1.0 + 1e-3 * (rng.random((N, H, W)) - 0.5))).astype(np.float32)
        gt[rng.random((N, H, W)) < 0.2] = 0.0
        return z, gt
    z = np.clip(2.5 * rng.standard_normal((N, H, W)), -7.5, 7.5).astype(np.float32)
    gt = _draw_gt(rng, (N, H, W))
    if name == "L3":
        gt[1] = np.where(rng.random((H, W)) < 0.5, 0.0, -2.0)      # no ground truth in the whole frame
        keep = gt[3, 20, 31]
        gt[3] = 0.0
        gt[3, 20, 31] = keep if keep > 0 else 1.75                    # a single valid pixel
    return z, gt


def make_inputs(name, seed=None):
    """-> dict like seg_training_ref.make_inputs': x [N, c_in, h, w], skip [N, c_skip, 2h, 2w] (float32), gt [N, 2h, 2w]
    float32, params (the 26 float32 arrays in PARAMS order, the last layer with one output channel), stats, and the sizes."""
    N, c_in, c_hidden, d1, c_skip, h, w = STEP_CASES[name]
    rng = np.random.default_rng(seed_of(name) if seed is None else seed)
    x = (np.abs(rng.standard_normal((N, c_in, h, w))) * 0.8 + 0.3 * rng.standard_normal((N, c_in, 1, 1))).astype(np.float32)
    skip = (np.abs(rng.standard_normal((N, c_skip, 2 * h, 2 * w))) * 0.8 + 0.3 * rng.standard_normal((N, c_skip, 1, 1))).astype(np.float32)
    gt = _draw_gt(rng, (N, 2 * h, 2 * w))
    params, stats = [], []
    for i, (ci, co) in enumerate(sr.layer_channels(c_in, c_hidden, d1, c_skip, 1)):
        wgt = (rng.standard_normal((co, ci, 3, 3)) * np.sqrt(2.0 / (9 * ci))).astype(np.float32)
        if i < 8:
            gamma, beta = rng.uniform(0.5, 1.5, co), 0.2 * rng.standard_normal(co)
            stats.append(((0.3 * rng.standard_normal(co)).astype(np.float32), rng.uniform(0.5, 1.5, co).astype(np.float32)))
            params += [wgt, gamma.astype(np.float32), beta.astype(np.float32)]
        else:
            params += [wgt, (0.2 * rng.standard_normal(co)).astype(np.float32)]
    return {"x": x, "skip": skip, "gt": gt, "params": params, "stats": stats, "weights": WEIGHTS, "N": N, "c_in": c_in,
            "c_hidden": c_hidden, "d1": d1, "c_skip": c_skip, "classes": 1, "h": h, "w": w}


# ---- the loss --------------------------------------------------------------------------------------------------------------
def depth_loss(z, gt, weights=WEIGHTS):
    """include/kp2d.h's kp2d_depth_loss in float64 -> dict(loss, silog, huber, dz, valid, stray, Dg, g, d); z and gt of one
    shape."""
    z, gt = np.asarray(z, np.float64), np.asarray(gt, np.float64)
    assert z.shape == gt.shape
    finite = np.isfinite(z) & np.isfinite(gt)
    ok = finite & (np.where(finite, gt, 0.0) > 0)
    zs, gs = np.where(ok, z, 0.0), np.where(ok, gt, 1.0)
    e = np.exp(-np.abs(zs))
    p = np.where(zs >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    q = np.where(zs >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    g = -(np.maximum(-zs, 0.0) + np.log1p(e)) - np.log(gs)
    d = p - gs
    M = int(ok.sum())
    ws, wh = weights
    mean = g[ok].sum() / M if M else 0.0
    Dg = ((g[ok] - mean) ** 2).sum() / (M - 1) + SILOG_LAMBDA * mean * mean if M >= 2 else 0.0
    on = M >= 2 and Dg > 0
    silog = SILOG_SCALE * np.sqrt(Dg) if on else 0.0
    ad = np.abs(d)
    huber = float(np.where(ad < HUBER_DELTA, 0.5 * d * d, HUBER_DELTA * (ad - 0.5 * HUBER_DELTA))[ok].sum() / M) if M else 0.0
    dz = np.zeros(z.shape)
    if on:
        k = ws * 0.5 * SILOG_SCALE / np.sqrt(Dg)
        dz += k * (2.0 * (g - mean) / (M - 1) + 2.0 * SILOG_LAMBDA * mean / M) * q
    if M:
        dz += wh * np.where(ad < HUBER_DELTA, d, np.sign(d) * HUBER_DELTA) / M * p * q
    dz *= ok
    return {"loss": float(ws * silog + wh * huber), "silog": float(silog), "huber": huber, "dz": dz, "valid": M,
            "stray": int((~finite).sum()), "Dg": float(Dg), "g": np.where(ok, g, 0.0), "d": np.where(ok, d, 0.0), "ok": ok}


# ---- the step --------------------------------------------------------------------------------------------------------------
def step_gradients(inp, params=None, weights=None, x=None, skip=None):
    """One forward / loss / backward -> seg_training_ref.head_forward's dict (logits [N, 1, 2h, 2w]) plus loss, silog, huber,
    valid, stray, dlogits and the other DMAPS, grads (PARAMS order)."""
    params = inp["params"] if params is None else params
    f = sr.head_forward(inp, params, x, skip)
    ls = depth_loss(f["logits"][:, 0], inp["gt"], inp["weights"] if weights is None else weights)
    f.update({k: ls[k] for k in ("loss", "silog", "huber", "valid", "stray", "Dg")})
    f["dlogits"] = ls["dz"][:, None]
    f["d"] = ls["d"]
    grads = [None] * 26
    grads[24], grads[25], dy = sr.conv_bias_backward(f["y7"], params[24], f["dlogits"])
    f["d_y7"] = dy

    def back(i, dy, need_dx=True):
        lx, y, c, scale, invstd = f["acts"][i]
        dw, dgamma, dbeta, dx = hr.cbr_backward(lx, params[3 * i], scale, inp["stats"][i][0], invstd, SLOPE, y, c, dy, need_dx)
        grads[3 * i:3 * i + 3] = [dw, dgamma, dbeta]
        return dx

    f["d_cat2"] = back(7, dy)
    f["d_y6"] = sr.shuffle_cat_backward(f["d_cat2"], inp["d1"] // 4)
    f["d_y5"] = back(6, f["d_y6"])
    f["d_cat1"] = back(5, f["d_y5"])
    f["d_y4"] = sr.shuffle_cat_backward(f["d_cat1"], inp["d1"] // 4)
    f["d_y3"] = back(4, f["d_y4"])
    f["d_y2"] = back(3, f["d_y3"])
    f["d_pooled"] = back(2, f["d_y2"])
    f["d_y1"] = sr.maxpool2_backward(f["y1"], f["d_pooled"])
    f["d_y0"] = back(1, f["d_y1"])
    back(0, f["d_y0"], need_dx=False)
    f["grads"] = grads
    return f


def loss_from(inp, params, x=None, skip=None):
    f = sr.head_forward(inp, params, x, skip)
    return depth_loss(f["logits"][:, 0], inp["gt"], inp["weights"])["loss"]


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


def load_fixture(name):
    return np.load(os.path.join(GOLDEN, f"case_{name}.npz"))


def load_trajectory():
    return np.load(os.path.join(GOLDEN, "trajectory.npz"))


LOSS_KEYS = ("loss", "silog", "huber", "dlogits")
STEP_KEYS = LOSS_KEYS[:3] + MAPS + DMAPS + tuple(f"g{i}" for i in range(26))


def bounds():
    """-> dict: per quantity (loss, silog, huber, every map of MAPS and DMAPS, g0..g25) the bound on E = max|G - G64| / max|G64|
    (a scalar: |v - v64| / |v64|): max(8 x the reference module's own float32 error of that quantity, the maximum over the
    fixture cases that have it, 16 x 2^-24)."""
    fx = [load_fixture(n) for n in list(LOSS_CASES) + list(STEP_CASES)]
    return {k: max(8.0 * max(float(f["err32_" + k]) for f in fx if "err32_" + k in f.files), FLOOR) for k in STEP_KEYS}


def floor_bounds():
    """The unpinned cases: 16 x 2^-24 of the quantity's largest magnitude alone, against this oracle."""
    return {k: FLOOR for k in LOSS_KEYS}


def trajectory_bounds():
    """The same for the trajectory: loss_head, loss_last, and per trained parameter p{i}_head / p{i}_last (the maximum over
    the steps)."""
    fx = load_trajectory()
    return {k[6:]: max(8.0 * float(fx[k]), FLOOR) for k in fx.files if k.startswith("err32_")}
