"""float64 numpy oracle of the head training step in the reference's own mode (nano_vs_slam_amd.vpr_head_training with
bn="batch" and dropout; kp2d_cbr_forward_batchnorm, kp2d_cbr_backward_batchnorm, kp2d_dropout2d_mask of include/kp2d.h):
convlad1..3 with BatchNorm on the batch's own statistics, the running statistics' update, Dropout2d behind convlad1, by the
formulas of the header.  The convolution products and the inputs come from vpr_head_training_ref, NetVLAD, the loss and Adam
from vlad_training_ref; the counter-based dropout draw is restated here in Python integers.  Fixtures under
tests/golden/vpr_head_bn/ hold outputs, settings and the reference's dropout masks only (written by
tools/make_vpr_head_bn_golden.py from the reference's VPRHead in .train() with torch autograd).
"""
import os

import numpy as np

import vpr_head_training_ref as hr

vr = hr.vr
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vpr_head_bn")
P_DROP = 0.2                      # the reference's Dropout2d(0.2) (modules/decoders/vpr.py:55)
MOMENTUM = 0.1                    # its bn_momentum default
# fixture name -> (case of hr.CASES, p, torch seed the reference's Dropout2d ran under); the seeds are recorded in the fixtures.
# (E: under seed 305 torch's mask leaves the case's one triplet inactive, every gradient zero: nothing to compare.)
FIXTURES = {"A_p20": ("A", P_DROP, 301), "B_p20": ("B", P_DROP, 302), "C_p20": ("C", P_DROP, 303), "D_p20": ("D", P_DROP, 304),
            "E_p20": ("E", P_DROP, 306), "B_p0": ("B", 0.0, 302), "C_p0": ("C", 0.0, 303)}
TRAJECTORY = "C_p20"
STATS = tuple(f"{k}{i}" for i in (1, 2, 3) for k in ("mean", "var", "rmean", "rvar"))      # per layer: batch mean, biased
                                                                                          # variance, running statistics after
QUANTITIES = ("loss",) + tuple(hr.GROUPS) + hr.MAPS + ("mean", "var", "rmean", "rvar")     # one err32_* each


# ---- the dropout draw, in Python integers ------------------------------------------------------------------------------
M64 = (1 << 64) - 1


def mix(z):
    """splitmix64's finaliser (csrc/mix64.h)"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, step, layer, n, c):
    """The 64-bit draw of kp2d_dropout2d_mask for one (frame, channel)."""
    h = mix((seed + 0x9E3779B97F4A7C15) & M64)
    h = mix(h ^ ((step << 32) | layer))
    return mix(h ^ ((n << 32) | c))


def dropout_scale(N, C, p, seed, step, layer):
    """-> float32 [N, C]: 0 where the top 53 bits of the draw, as a value in [0, 1), lie below p, else 1 / (1 - p).  The
    comparison is in integers: u >= p for u = k 2^-53 is k >= ceil(p 2^53), and p 2^53 is exact in double."""
    out = np.zeros((N, C), np.float32)
    kept = np.float32(1.0 / (1.0 - p))
    t = p * 2.0 ** 53
    thr = int(t) if t == int(t) else int(t) + 1
    for n in range(N):
        for c in range(C):
            if (draw(seed, step, layer, n, c) >> 11) >= thr:
                out[n, c] = kept
    return out


# ---- one layer -----------------------------------------------------------------------------------------------------------
def _ch(v):
    return np.asarray(v, np.float64)[None, :, None, None]


def cbr_forward_batch(x, w, gamma, beta, slope, drop=None, eps=hr.BN_EPS):
    """-> (y, c, mean, var (biased), invstd)"""
    x, w, gamma, beta = (np.asarray(t, np.float64) for t in (x, w, gamma, beta))
    c = hr.conv3x3(x, w)
    mean = c.mean(axis=(0, 2, 3))
    var = ((c - _ch(mean)) ** 2).mean(axis=(0, 2, 3))
    invstd = 1.0 / np.sqrt(var + eps)
    pre = _ch(gamma * invstd) * (c - _ch(mean)) + _ch(beta)
    y = np.where(pre > 0, pre, slope * pre)
    if drop is not None:
        y = y * np.asarray(drop, np.float64)[:, :, None, None]
    return y, c, mean, var, invstd


def running_update(running, mean, var, M, momentum=MOMENTUM):
    rm, rv = (np.asarray(t, np.float64) for t in running)
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * var * M / (M - 1)


def cbr_backward_batch(x, w, gamma, mean, invstd, slope, y, c, dy, drop=None, need_dx=True):
    """-> (dw, dgamma, dbeta, dx or None, dc)"""
    x, w, gamma = (np.asarray(t, np.float64) for t in (x, w, gamma))
    M = c.shape[0] * c.shape[2] * c.shape[3]
    d = dy if drop is None else dy * np.asarray(drop, np.float64)[:, :, None, None]
    g = np.where(y > 0, d, slope * d)
    xh = (c - _ch(mean)) * _ch(invstd)
    dbeta = g.sum(axis=(0, 2, 3))
    dgamma = (g * xh).sum(axis=(0, 2, 3))
    dc = _ch(gamma * invstd) * (g - _ch(dbeta) / M - xh * _ch(dgamma) / M)
    return hr.conv3x3_dw(dc, x), dgamma, dbeta, (hr.conv3x3_dx(dc, w) if need_dx else None), dc


# ---- the step ------------------------------------------------------------------------------------------------------------
def head_forward(feat, params, slope, drop, start=0):
    """The layers from ``start`` on (as hr.head_forward), on batch statistics; ``drop`` acts behind layer 0 ->
    dict(acts [(x, y, c, mean, var, invstd)], enc, fwd, vlad)."""
    acts, x = [], np.asarray(feat, np.float64)
    for i in range(start, 3):
        w, gamma, beta = params[3 * i:3 * i + 3]
        y, c, mean, var, invstd = cbr_forward_batch(x, w, gamma, beta, slope, drop if i == 0 else None)
        acts.append((x, y, c, mean, var, invstd))
        x = y
    N, C = x.shape[:2]
    fwd = vr.forward(x.reshape(N, C, -1), params[9], params[10])
    return {"acts": acts, "enc": x, "fwd": fwd, "vlad": fwd["vlad"]}


def step_gradients(feat, params, stats, B, counts, slope, drop, margin=hr.MARGIN):
    """One forward / loss / backward -> dict: y1..y3, vlad, loss, dvlad, n_active, hinge, grads (hr.PARAMS order),
    dx_netvlad, dx3, dx2, mean{i}, var{i}, rmean{i}, rvar{i} (the running statistics after the step), dc{i}."""
    f = head_forward(feat, params, slope, drop)
    loss, dvlad, n_active, hinge = vr.triplet_loss(f["vlad"], B, counts, margin)
    dW, dcent, dU = vr.backward(f["fwd"], params[10], dvlad)
    enc = f["enc"]
    N, C = enc.shape[:2]
    dy = hr.netvlad_dx(f["fwd"], enc.reshape(N, C, -1), params[9], params[10], dU).reshape(enc.shape)
    out = {"vlad": f["vlad"], "loss": loss, "dvlad": dvlad, "n_active": n_active, "hinge": hinge, "dx_netvlad": dy}
    grads = [None] * 9 + [dW, dcent]
    for i in (2, 1, 0):
        x, y, c, mean, var, invstd = f["acts"][i]
        M = c.shape[0] * c.shape[2] * c.shape[3]
        out[f"y{i + 1}"], out[f"mean{i + 1}"], out[f"var{i + 1}"] = y, mean, var
        out[f"rmean{i + 1}"], out[f"rvar{i + 1}"] = running_update(stats[i], mean, var, M)
        dw, dgamma, dbeta, dy, dc = cbr_backward_batch(x, params[3 * i], params[3 * i + 1], mean, invstd, slope, y, c, dy,
                                                       drop if i == 0 else None, need_dx=i > 0)
        out[f"dc{i + 1}"] = dc
        grads[3 * i:3 * i + 3] = [dw, dgamma, dbeta]
        if i > 0:
            out[f"dx{i + 1}"] = dy
    out["grads"] = grads
    return out


def loss_from(x, start, params, B, counts, slope, drop, margin=hr.MARGIN):
    """The loss as a function of the input of layer ``start`` (3: NetVLAD's) and the parameters: for finite differences."""
    return vr.triplet_loss(head_forward(x, params, slope, drop, start)["vlad"], B, counts, margin)[0]


def trajectory(inp, drops, keep=hr.PARAM_STEPS, lr=hr.LR, margin=hr.MARGIN):
    """len(drops) Adam steps on one batch, step t under the mask drops[t] -> (losses, the parameters after `keep` steps, the
    running statistics [(mean, var) per layer] after `keep` steps, the gradients of the first `keep` steps)."""
    params = [p.astype(np.float64) for p in inp["params"]]
    stats = [tuple(np.asarray(t, np.float64) for t in s) for s in inp["stats"]]
    opt = vr.Adam(params, lr=lr)
    losses, kept, kept_stats, grads = [], None, None, []
    for t, drop in enumerate(drops):
        s = step_gradients(inp["feat"], params, stats, inp["B"], inp["counts"], inp["slope"], drop, margin)
        losses.append(s["loss"])
        stats = [(s[f"rmean{i}"], s[f"rvar{i}"]) for i in (1, 2, 3)]
        g = [np.asarray(gi).reshape(p.shape) for gi, p in zip(s["grads"], params)]
        if t < keep:
            grads.append([gi.copy() for gi in g])
        opt.step(g)
        if t + 1 == keep:
            kept, kept_stats = [p.copy() for p in params], stats
    return np.asarray(losses), kept, kept_stats, grads


rel_err = hr.rel_err
stored = hr.stored
FLOOR = 16.0 * 2.0 ** -24


def load_fixture(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"))


def bounds():
    """-> dict, one entry per name of QUANTITIES: max(8 x the reference's own float32 error of that quantity, 16 x 2^-24);
    the error is that of its VPRHead in .train() run in float32 on the CPU against its float64 run under the same mask
    (E = max|G - G64| / max|G64|; for the loss the absolute difference), the maximum over the fixtures.  A group's figure is
    the maximum over its members (mean, var, rmean, rvar: over the three layers)."""
    fx = [load_fixture(n) for n in FIXTURES]
    return {k: max(8.0 * max(float(f["err32_" + k]) for f in fx), FLOOR) for k in QUANTITIES}


def loss_bound(loss64, b=None):
    b = b or bounds()
    return max(b["loss"], 16.0 * float(np.spacing(np.float32(abs(loss64)))))
