"""float64 numpy oracle of the NetVLAD training step (nano_vs_slam_amd.vlad_training, csrc/vlad_train.hip): forward,
backward by the formulas of include/kp2d.h, the triplet margin loss with its gradient, and Adam.  Also the seeded inputs
of the test cases: fixtures under tests/golden/vlad_training/ hold outputs only (written by
tools/make_vlad_training_golden.py from the reference's NetVLAD module with torch autograd), the inputs are regenerated here.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vlad_training")

# name -> (K, C, S, B, counts, seed): the smallest shapes at which the kernels can go wrong
CASES = {
    "A": (64, 64, 300, 2, (3, 2), 101),      # the training default map (120 x 160), ragged last tile
    "B": (32, 48, 77, 3, (1, 0, 4), 102),    # config N's sizes, a query without negatives
    "C": (8, 16, 12, 1, (1,), 103),          # less than one tile
    "D": (64, 128, 65, 1, (2,), 104),        # K C at the limit, one pixel past a tile
    "E": (64, 64, 1200, 1, (2,), 105),       # many tiles per frame
}
MARGIN = 0.1          # the reference's default (train_visloc.py --margin): the hinge uses MARGIN ** 0.5
LR = 1e-4             # the reference's default learning rate
TRAJECTORY_CASE, TRAJECTORY_STEPS, PARAM_STEPS = "A", 10, 3
COL_STRIDE = 4        # the fixtures keep every fourth column of vlad and dvlad (vlad_cols, dvlad_cols), all rows


def make_inputs(name):
    """-> dict(x [N, C, S], W [K, C], cent [K, C] float32; B, counts, K, C, S, N).  Rows of x: queries, positives, the
    negatives in query order.  Frames are correlated the way mined triplets are: a positive is its query plus a little
    noise, the first negative of a query (and every second one after it) is a near miss that violates the margin, the
    others are unrelated frames that do not, so every case with two or more negatives has active and inactive triplets."""
    K, C, S, B, counts, seed = CASES[name]
    rng = np.random.default_rng(seed)
    cent0 = rng.standard_normal((K, C))
    unit = cent0 / np.linalg.norm(cent0, axis=1, keepdims=True)
    W = 6.0 * unit + 0.05 * rng.standard_normal((K, C))
    cent = 0.6 * unit + 0.02 * rng.standard_normal((K, C))

    def frame():
        # pixels scattered around the cluster directions, as an encoder map around its k-means centroids
        which = rng.integers(0, K, size=S)
        return (unit[which] + 0.35 * rng.standard_normal((S, C))).T

    q = [frame() for _ in range(B)]
    p = [qi + 0.15 * rng.standard_normal((C, S)) for qi in q]
    n = []
    for i, cnt in enumerate(counts):
        for j in range(cnt):
            n.append(q[i] + 0.3 * rng.standard_normal((C, S)) if j % 2 == 0 else frame())
    x = np.stack(q + p + n).astype(np.float32)
    return {"x": x, "W": W.astype(np.float32), "cent": cent.astype(np.float32), "B": B, "counts": tuple(counts),
            "K": K, "C": C, "S": S, "N": x.shape[0]}


def forward(x, W, cent):
    """x [N, C, S], W, cent [K, C] -> dict: vlad [N, K C] and what the backward needs."""
    x, W, cent = (np.asarray(t, np.float64) for t in (x, W, cent))
    xh = np.swapaxes(x, 1, 2)                                             # [N, S, C]
    xh = xh / np.maximum(np.linalg.norm(xh, axis=2, keepdims=True), 1e-12)
    z = xh @ W.T                                                          # [N, S, K]
    a = np.exp(z - z.max(axis=2, keepdims=True))
    a /= a.sum(axis=2, keepdims=True)
    r = a.sum(axis=1)                                                     # [N, K]
    U = np.einsum("nsk,nsc->nkc", a, xh) - r[:, :, None] * cent[None]
    n = np.maximum(np.linalg.norm(U, axis=2), 1e-12)                      # [N, K]
    V = U / n[:, :, None]
    g = np.maximum(np.sqrt((V * V).sum(axis=(1, 2))), 1e-12)              # [N]
    v = V / g[:, None, None]
    return {"vlad": v.reshape(x.shape[0], -1), "V": V, "n": n, "r": r, "g": g, "xh": xh, "a": a}


def backward(fwd, cent, dvlad):
    """-> (dW [K, C], dcent [K, C], dU [N, K, C]) from forward()'s dict and dvlad [N, K C]."""
    cent = np.asarray(cent, np.float64)
    V, n, r, g, xh, a = (fwd[k] for k in ("V", "n", "r", "g", "xh", "a"))
    N, K, C = V.shape
    dv = np.asarray(dvlad, np.float64).reshape(N, K, C)
    v = V / g[:, None, None]
    dV = (dv - v * (v * dv).sum(axis=(1, 2), keepdims=True)) / g[:, None, None]
    dU = (dV - V * (V * dV).sum(axis=2, keepdims=True)) / n[:, :, None]
    dcent = -(r[:, :, None] * dU).sum(axis=0)
    da = np.einsum("nsc,nkc->nsk", xh, dU) - (cent[None] * dU).sum(axis=2)[:, None, :]
    dz = a * (da - (a * da).sum(axis=2, keepdims=True))
    dW = np.einsum("nsk,nsc->kc", dz, xh)
    return dW, dcent, dU


def triplet_loss(vlad, B, counts, margin=MARGIN):
    """-> (loss, dvlad, n_active, hinge arguments per triplet).  d(u, w) = ||u - w + 1e-6||, hinge margin ** 0.5."""
    v = np.asarray(vlad, np.float64)
    counts = [int(c) for c in counts]
    tot = sum(counts)
    dv = np.zeros_like(v)
    hinge = []
    loss = 0.0
    j = 0
    for i, cnt in enumerate(counts):
        dqp = v[i] - v[B + i] + 1e-6
        dp = np.sqrt((dqp * dqp).sum())
        for _ in range(cnt):
            row = 2 * B + j
            dqn = v[i] - v[row] + 1e-6
            dn = np.sqrt((dqn * dqn).sum())
            h = dp - dn + margin ** 0.5
            hinge.append(h)
            if h > 0:
                loss += h / tot
                dv[i] += (dqp / dp - dqn / dn) / tot
                dv[B + i] -= dqp / dp / tot
                dv[row] += dqn / dn / tot
            j += 1
    hinge = np.asarray(hinge, np.float64)
    return loss, dv, int((hinge > 0).sum()), hinge


class Adam:
    """torch.optim.Adam (no weight decay, no amsgrad) on float64 arrays, updated in place."""

    def __init__(self, params, lr=LR, betas=(0.9, 0.999), eps=1e-8):
        self.params, self.lr, self.betas, self.eps = params, lr, betas, eps
        self.m = [np.zeros_like(p) for p in params]
        self.v = [np.zeros_like(p) for p in params]
        self.t = 0

    def step(self, grads):
        self.t += 1
        b1, b2 = self.betas
        for p, g, m, v in zip(self.params, grads, self.m, self.v):
            m += (1 - b1) * (g - m)
            v *= b2
            v += (1 - b2) * g * g
            denom = np.sqrt(v) / np.sqrt(1 - b2 ** self.t) + self.eps
            p -= self.lr / (1 - b1 ** self.t) * m / denom


def step_gradients(x, W, cent, B, counts, margin=MARGIN):
    """One forward / loss / backward -> dict(vlad, loss, dvlad, dW, dcent, n_active, hinge)."""
    fwd = forward(x, W, cent)
    loss, dvlad, n_active, hinge = triplet_loss(fwd["vlad"], B, counts, margin)
    dW, dcent, _ = backward(fwd, cent, dvlad)
    return {"vlad": fwd["vlad"], "loss": loss, "dvlad": dvlad, "dW": dW, "dcent": dcent, "n_active": n_active, "hinge": hinge}


def trajectory(inp, steps=TRAJECTORY_STEPS, keep=PARAM_STEPS, lr=LR, margin=MARGIN):
    """`steps` Adam steps on one batch -> (losses [steps], W and cent after `keep` steps, max |grad| fraction record:
    the gradients of the first `keep` steps, for the sign-driven exemption of the parameter comparison)."""
    W, cent = inp["W"].astype(np.float64), inp["cent"].astype(np.float64)
    opt = Adam([W, cent], lr=lr)
    losses, kept, grads = [], None, []
    for t in range(steps):
        s = step_gradients(inp["x"], W, cent, inp["B"], inp["counts"], margin)
        losses.append(s["loss"])
        if t < keep:
            grads.append((s["dW"].copy(), s["dcent"].copy()))
        opt.step([s["dW"], s["dcent"]])
        if t + 1 == keep:
            kept = (W.copy(), cent.copy())
    return np.asarray(losses), kept[0], kept[1], grads


def rel_err(g, g64):
    """E(G) = max|G - G64| / max|G64|."""
    g64 = np.asarray(g64, np.float64)
    return float(np.abs(np.asarray(g, np.float64) - g64).max() / np.abs(g64).max())


def sign_driven(grads, bound):
    """Elements whose oracle gradient at some of the given steps was below the gradient bound (|g| < bound * max|g|): a
    device gradient within the bound may have the other sign there, and Adam's first steps move by lr * sign(g).
    grads: [(dW, dcent), ...] per step; bound: dict with "dW" and "dcent" -> (mask for W, mask for cent)."""
    mw = np.zeros(grads[0][0].shape, bool)
    mc = np.zeros(grads[0][1].shape, bool)
    for dW, dcent in grads:
        mw |= np.abs(dW) < bound["dW"] * np.abs(dW).max()
        mc |= np.abs(dcent) < bound["dcent"] * np.abs(dcent).max()
    return mw, mc


def load_fixture(name):
    return np.load(os.path.join(GOLDEN, f"case_{name}.npz"))


def bounds():
    """-> dict(loss, dW, dcent, grad): 8 x the reference's own float32 error (its module run in float32 on the CPU
    against its float64 run), the maximum over the fixture cases per quantity.  `grad`, used for dvlad (for which the
    fixtures store no float32 error of its own), is the smaller of the two gradient bounds.  The loss bound has a floor of
    16 ulp of the loss in fp32, applied by loss_bound()."""
    fx = [load_fixture(n) for n in CASES]
    b = {k: 8.0 * max(float(f["err32_" + k]) for f in fx) for k in ("loss", "dW", "dcent")}
    b["grad"] = min(b["dW"], b["dcent"])
    return b


def loss_bound(loss64, b=None):
    b = b or bounds()
    return max(b["loss"], 16.0 * float(np.spacing(np.float32(abs(loss64)))))
