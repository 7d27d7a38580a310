"""float64 numpy oracle of the head training step (nano_vs_slam_amd.vpr_head_training, csrc/vpr_head_train.hip and
csrc/vlad_train.hip): convlad1..3 (conv3x3, BatchNorm on running statistics, (Leaky)ReLU) forward and backward by the
formulas of include/kp2d.h, NetVLAD with its input gradient, the triplet margin loss and Adam (the last three from
vlad_training_ref).  Also the seeded inputs of the test cases: fixtures under tests/golden/vpr_head_training/ hold outputs
and settings only (written by tools/make_vpr_head_training_golden.py from the reference's VPRHead with torch autograd), the
inputs are regenerated here.
"""
import os

import numpy as np

import vlad_training_ref as vr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vpr_head_training")

# name -> (Cin, C, K, H, W, B, counts, slope, gamma0, seed): the smallest shapes at which the kernels can go wrong
CASES = {
    "A": (16, 16, 4, 5, 7, 1, (3,), 0.01, False, 201),       # every pixel touches a border; one ragged 64-pixel tile
    "B": (32, 48, 32, 9, 13, 2, (2, 0), 0.01, False, 202),   # config N's width, Cin != Cout, ragged second tile, a query
                                                             # without negatives: two frames with exactly zero dy
    "C": (64, 64, 64, 8, 8, 1, (2,), 0.01, False, 203),      # config S, exactly one tile; the trajectory case
    "D": (16, 16, 4, 3, 70, 1, (1,), 0.01, False, 204),      # a row longer than a tile
    "E": (16, 16, 4, 2, 3, 1, (1,), 0.0, True, 205),         # more padding than pixels, ReLU, one channel per layer with gamma 0
}
MARGIN, LR = vr.MARGIN, vr.LR
BN_EPS = 1e-5
TRAJECTORY_CASE, TRAJECTORY_STEPS, PARAM_STEPS = "C", 10, 3
MAX_STORED = 768      # a fixture keeps at most this many entries of an array: every stride_of(size)-th of the flattened array
PARAMS = tuple(f"convlad{i}.{p}" for i in (1, 2, 3) for p in ("conv.weight", "bn.weight", "bn.bias")) + ("netvlad.conv.weight", "netvlad.centroids")
# gradient groups of the error bounds: name -> indices into PARAMS
GROUPS = {"conv": (0, 3, 6), "bn": (1, 2, 4, 5, 7, 8), "dW": (9,), "dcent": (10,)}
MAPS = ("y1", "y2", "y3", "dx_netvlad", "dx3", "dx2")


def stride_of(size):
    """The stored stride of an array of ``size`` entries: 1 up to MAX_STORED entries, else the smallest odd number that
    keeps at most MAX_STORED (odd: it does not lock onto the power-of-two channel and tile structure)."""
    st = -(-size // MAX_STORED)
    return st if st == 1 or st % 2 else st + 1


def stored(a):
    a = np.asarray(a)
    return a.ravel()[::stride_of(a.size)]


def make_inputs(name):
    """-> dict: feat [N, Cin, H, W] (rows: queries, positives, the negatives in query order), params (the eleven float32
    arrays in PARAMS order), stats [(running_mean, running_var) per layer], and the case's settings.  Frames are correlated
    the way mined triplets are: a positive is its query plus a little noise, the first negative of a query (and every second
    one after it) is a near miss, the others are unrelated frames."""
    Cin, C, K, H, W, B, counts, slope, gamma0, seed = CASES[name]
    rng = np.random.default_rng(seed)

    def frame():
        return np.abs(rng.standard_normal((Cin, H, W))) * 0.8 + 0.3 * rng.standard_normal((Cin, 1, 1))

    q = [frame() for _ in range(B)]
    p = [qi + 0.1 * rng.standard_normal((Cin, H, W)) for qi in q]
    n = []
    for i, cnt in enumerate(counts):
        for j in range(cnt):
            n.append(q[i] + 0.25 * rng.standard_normal((Cin, H, W)) if j % 2 == 0 else frame())
    feat = np.stack(q + p + n).astype(np.float32)
    params, stats = [], []
    ci = Cin
    for _ in range(3):
        w = rng.standard_normal((C, ci, 3, 3)) * np.sqrt(2.0 / (9 * ci))
        gamma = rng.uniform(0.5, 1.5, C)
        if gamma0:
            gamma[int(rng.integers(0, C))] = 0.0
        beta = 0.2 * rng.standard_normal(C)
        stats.append(((0.3 * rng.standard_normal(C)).astype(np.float32), rng.uniform(0.5, 1.5, C).astype(np.float32)))
        params += [w.astype(np.float32), gamma.astype(np.float32), beta.astype(np.float32)]
        ci = C
    cent0 = rng.standard_normal((K, C))
    unit = cent0 / np.linalg.norm(cent0, axis=1, keepdims=True)
    params.append((6.0 * unit + 0.05 * rng.standard_normal((K, C))).astype(np.float32))
    params.append((0.6 * unit + 0.02 * rng.standard_normal((K, C))).astype(np.float32))
    return {"feat": feat, "params": params, "stats": stats, "B": B, "counts": tuple(counts), "slope": slope, "Cin": Cin, "C": C,
            "K": K, "H": H, "W": W, "N": feat.shape[0]}


# ---- the three convolution-shaped products ---------------------------------------------------------------------------
def conv3x3(x, w):
    N, _, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros((N, w.shape[0], H, W))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("oc,nchw->nohw", w[:, :, ky, kx], xp[:, :, ky:ky + H, kx:kx + W])
    return out


def conv3x3_dw(dc, x):
    """dw[co,ci,ky,kx] = sum_{n,y,x} dc[n,co,y,x] x[n,ci,y+ky-1,x+kx-1]"""
    _, _, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    dw = np.zeros((dc.shape[1], x.shape[1], 3, 3))
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = np.einsum("nohw,nchw->oc", dc, xp[:, :, ky:ky + H, kx:kx + W])
    return dw


def conv3x3_dx(dc, w):
    """dx[n,ci,y,x] = sum_{co,ky,kx} dc[n,co,y-ky+1,x-kx+1] w[co,ci,ky,kx]"""
    N, _, H, W = dc.shape
    dp = np.pad(dc, ((0, 0), (0, 0), (1, 1), (1, 1)))
    dx = np.zeros((N, w.shape[1], H, W))
    for ky in range(3):
        for kx in range(3):
            dx += np.einsum("oc,nohw->nchw", w[:, :, ky, kx], dp[:, :, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W])
    return dx


# ---- one layer ---------------------------------------------------------------------------------------------------------
def cbr_forward(x, w, gamma, beta, mean, var, slope, eps=BN_EPS):
    """-> (y, c, scale, invstd)"""
    x, w, gamma, beta, mean, var = (np.asarray(t, np.float64) for t in (x, w, gamma, beta, mean, var))
    c = conv3x3(x, w)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * invstd
    pre = c * scale[None, :, None, None] + (beta - mean * scale)[None, :, None, None]
    return np.where(pre > 0, pre, slope * pre), c, scale, invstd


def cbr_backward(x, w, scale, mean, invstd, slope, y, c, dy, need_dx=True):
    """-> (dw, dgamma, dbeta, dx or None)"""
    x, w, mean = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(mean, np.float64)
    dpre = np.where(y > 0, dy, slope * dy)
    dbeta = dpre.sum(axis=(0, 2, 3))
    dgamma = (dpre * (c - mean[None, :, None, None]) * invstd[None, :, None, None]).sum(axis=(0, 2, 3))
    dc = dpre * scale[None, :, None, None]
    return conv3x3_dw(dc, x), dgamma, dbeta, (conv3x3_dx(dc, w) if need_dx else None)


def netvlad_dx(fwd, x, W, cent, dU):
    """The NetVLAD layer's gradient with respect to its input x [N, C, S], from vlad_training_ref.forward's dict and
    backward's dU."""
    x, W, cent = (np.asarray(t, np.float64) for t in (x, W, cent))
    a, xh = fwd["a"], fwd["xh"]
    da = np.einsum("nsc,nkc->nsk", xh, dU) - (cent[None] * dU).sum(axis=2)[:, None, :]
    dz = a * (da - (a * da).sum(axis=2, keepdims=True))
    dxh = np.einsum("nsk,nkc->nsc", a, dU) + dz @ W
    norm = np.maximum(np.linalg.norm(np.swapaxes(x, 1, 2), axis=2, keepdims=True), 1e-12)
    dx = (dxh - xh * (xh * dxh).sum(axis=2, keepdims=True)) / norm
    return np.swapaxes(dx, 1, 2)


# ---- the step ------------------------------------------------------------------------------------------------------------
def head_forward(feat, params, stats, slope, start=0):
    """The layers from ``start`` on (0: feat is the backbone map; 1, 2: a layer's input; 3: NetVLAD's) ->
    dict(acts [(x, y, c, scale, invstd) per layer run], enc, fwd (NetVLAD's), vlad)."""
    acts, x = [], np.asarray(feat, np.float64)
    for i in range(start, 3):
        w, gamma, beta = params[3 * i:3 * i + 3]
        y, c, scale, invstd = cbr_forward(x, w, gamma, beta, stats[i][0], stats[i][1], slope)
        acts.append((x, y, c, scale, invstd))
        x = y
    N, C = x.shape[:2]
    fwd = vr.forward(x.reshape(N, C, -1), params[9], params[10])
    return {"acts": acts, "enc": x, "fwd": fwd, "vlad": fwd["vlad"]}


def step_gradients(feat, params, stats, B, counts, slope, margin=MARGIN):
    """One forward / loss / backward -> dict: y1..y3, vlad, loss, dvlad, n_active, hinge, grads (PARAMS order),
    dx_netvlad, dx3, dx2."""
    f = head_forward(feat, params, stats, slope)
    loss, dvlad, n_active, hinge = vr.triplet_loss(f["vlad"], B, counts, margin)
    dW, dcent, dU = vr.backward(f["fwd"], params[10], dvlad)
    enc = f["enc"]
    N, C = enc.shape[:2]
    dy = netvlad_dx(f["fwd"], enc.reshape(N, C, -1), params[9], params[10], dU).reshape(enc.shape)
    out = {"vlad": f["vlad"], "loss": loss, "dvlad": dvlad, "n_active": n_active, "hinge": hinge, "dx_netvlad": dy}
    grads = [None] * 9 + [dW, dcent]
    for i in (2, 1, 0):
        x, y, c, scale, invstd = f["acts"][i]
        out[f"y{i + 1}"] = y
        dw, dgamma, dbeta, dy = cbr_backward(x, params[3 * i], scale, stats[i][0], invstd, slope, y, c, dy, need_dx=i > 0)
        grads[3 * i:3 * i + 3] = [dw, dgamma, dbeta]
        if i > 0:
            out[f"dx{i + 1}"] = dy
    out["grads"] = grads
    return out


def loss_from(x, start, params, stats, B, counts, slope, margin=MARGIN):
    """The loss as a function of the input of layer ``start`` (3: NetVLAD's) and the parameters: for finite differences."""
    return vr.triplet_loss(head_forward(x, params, stats, slope, start)["vlad"], B, counts, margin)[0]


def trajectory(inp, steps=TRAJECTORY_STEPS, keep=PARAM_STEPS, lr=LR, margin=MARGIN):
    """`steps` Adam steps on one batch over all eleven parameters -> (losses [steps], the parameters after `keep` steps,
    the gradients of the first `keep` steps: for the sign-driven exemption of the parameter comparison)."""
    params = [p.astype(np.float64) for p in inp["params"]]
    opt = vr.Adam(params, lr=lr)
    losses, kept, grads = [], None, []
    for t in range(steps):
        s = step_gradients(inp["feat"], params, inp["stats"], inp["B"], inp["counts"], inp["slope"], margin)
        losses.append(s["loss"])
        g = [np.asarray(gi).reshape(p.shape) for gi, p in zip(s["grads"], params)]
        if t < keep:
            grads.append([gi.copy() for gi in g])
        opt.step(g)
        if t + 1 == keep:
            kept = [p.copy() for p in params]
    return np.asarray(losses), kept, grads


rel_err = vr.rel_err


def load_fixture(name):
    return np.load(os.path.join(GOLDEN, f"case_{name}.npz"))


def bounds():
    """-> dict(loss, conv, bn, dW, dcent, and one entry per map of MAPS): 8 x the reference's own float32 error of that
    quantity (its VPRHead run in float32 on the CPU against its float64 run; E = max|G - G64| / max|G64|, for the loss the
    absolute difference), the maximum over the fixture cases.  A group's figure is the maximum over its members.  The loss
    bound has a floor of 16 ulp of the loss in fp32, applied by loss_bound()."""
    fx = [load_fixture(n) for n in CASES]
    return {k: 8.0 * max(float(f["err32_" + k]) for f in fx) for k in ("loss",) + tuple(GROUPS) + MAPS}


def loss_bound(loss64, b=None):
    b = b or bounds()
    return max(b["loss"], 16.0 * float(np.spacing(np.float32(abs(loss64)))))
