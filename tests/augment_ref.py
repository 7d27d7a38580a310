"""float64 numpy oracle of the view-pair calls (nano_vs_slam_amd.augment, csrc/augment.hip) by the formulas of include/kp2d.h:
the coordinate map, the nearest and bilinear warp, the nearest warp's backward (in float64, and in float32 adding in ascending
row-major order, the device's order), the cross-view depth term, sample_homography driven by a ``draws`` array, and the draw
function restated in Python integers.  tests/test_augment_cpu.py holds the warp to torch's grid_sample and the sampler to the
fixtures tools/make_augment_golden.py wrote from the reference's own function (tests/golden/augment/).
"""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment")
TILE_W, TILE_H = 64, 4          # KP2D_WARP_TILE_W, KP2D_WARP_TILE_H: a workgroup's pixels
SLOTS = 9                       # KP2D_HOMOGRAPHY_DRAWS
NORMAL_SLOTS = (0, 1, 2, 3, 5)
DEFAULTS = dict(perspective=True, scaling=True, rotation=True, translation=True, n_scales=100, n_angles=100, scaling_amplitude=0.2,
                perspective_amplitude=0.2, patch_ratio=0.7, max_angle=math.pi / 2)

# a homography that leaves the image: 22 % of a 17 x 23 map falls outside
GENERAL = np.array([[0.99, 0.25, 0.2], [-0.2, 1.155, -0.15], [0.1, -0.15, 1.0]])
# the full-scan case of the backward: forward w' > 0 on the whole 6 x 8 grid, source corners with inverse w' <= 0
FULL_SCAN = np.array([[-0.414, 0.511, -0.48], [-0.834, 1.138, 0.35], [-0.222, -0.538, 1.0]])
# every coordinate of a 9 x 17 map is an exact half: ties go to even
HALVES = np.array([[1.0, 0.0, 1.0 / 16], [0.0, 1.0, 1.0 / 8], [0.0, 0.0, 1.0]])
ZOOM_IN = np.array([[0.4, 0.05, 0.1], [-0.03, 0.45, -0.05], [0.0, 0.0, 1.0]])      # fan-in >= 4


# ---- the coordinate map ---------------------------------------------------------------------------------------------------------
def grid(hom, H, W, stride=1):
    """hom [3,3] -> (u'/w', v'/w') [Ho, Wo] float64: the normalised source coordinates of every output pixel."""
    h = np.asarray(hom, np.float64)
    X = (np.arange(W // stride) * stride).astype(np.float64)[None, :]
    Y = (np.arange(H // stride) * stride).astype(np.float64)[:, None]
    gx = 2.0 * X / (W - 1) - 1.0
    gy = 2.0 * Y / (H - 1) - 1.0
    with np.errstate(all="ignore"):
        u = (h[0, 0] * gx + h[0, 1] * gy) + h[0, 2]
        v = (h[1, 0] * gx + h[1, 1] * gy) + h[1, 2]
        w = (h[2, 0] * gx + h[2, 1] * gy) + h[2, 2]
        return u / w, v / w


def src_coords(hom, H, W, stride=1):
    """-> (px, py) [Ho, Wo] float64 in source pixels."""
    un, vn = grid(hom, H, W, stride)
    with np.errstate(all="ignore"):
        return ((un + 1.0) / 2.0) * (W - 1), ((vn + 1.0) / 2.0) * (H - 1)


def nearest(hom, H, W, stride=1):
    """-> (inside [Ho, Wo] bool, flat source index [Ho, Wo] int64, 0 where outside)."""
    px, py = src_coords(hom, H, W, stride)
    with np.errstate(all="ignore"):
        rx, ry = np.rint(px), np.rint(py)
        inside = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
    xi = np.where(inside, rx, 0).astype(np.int64)
    yi = np.where(inside, ry, 0).astype(np.int64)
    return inside, yi * W + xi


def _homs(hom, N):
    hom = np.asarray(hom, np.float64)
    return np.broadcast_to(hom, (N, 3, 3)) if hom.ndim == 2 else hom


def warp(x, hom, mode="nearest", fill=0, stride=1):
    """x [N, C, H, W] -> [N, C, H / stride, W / stride].  nearest: x's dtype, exact.  bilinear: float64."""
    x = np.asarray(x)
    N, C, H, W = x.shape
    homs = _homs(hom, N)
    Ho, Wo = H // stride, W // stride
    if mode == "nearest":
        out = np.empty((N, C, Ho, Wo), x.dtype)
        for n in range(N):
            inside, at = nearest(homs[n], H, W, stride)
            got = x[n].reshape(C, H * W)[:, at.ravel()].reshape(C, Ho, Wo)
            out[n] = np.where(inside[None], got, np.asarray(fill).astype(x.dtype))
        return out
    out = np.zeros((N, C, Ho, Wo), np.float64)
    xf = x.astype(np.float64)
    for n in range(N):
        px, py = src_coords(homs[n], H, W, stride)
        x0, y0 = np.floor(px), np.floor(py)
        fx, fy = px - x0, py - y0
        for dx_, dy_, wgt in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
            xs, ys = x0 + dx_, y0 + dy_
            with np.errstate(all="ignore"):
                live = (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
            at = (np.where(live, ys, 0) * W + np.where(live, xs, 0)).astype(np.int64)
            out[n] += np.where(live[None], wgt[None] * xf[n].reshape(C, H * W)[:, at.ravel()].reshape(C, Ho, Wo), 0.0)
    return out


def warp_backward(dy, hom, size, stride=1, dtype=np.float32):
    """dy [N, C, Ho, Wo] -> dx [N, C, H, W]: the sum of dy over the outputs whose nearest source is the pixel, added in
    ascending row-major order in ``dtype`` (float32: the device's sum, bit for bit; float64: the yardstick)."""
    dy = np.asarray(dy, dtype)
    N, C = dy.shape[:2]
    H, W = size
    homs = _homs(hom, N)
    dx = np.zeros((N, C, H * W), dtype)
    for n in range(N):
        inside, at = nearest(homs[n], H, W, stride)
        sel, idx = inside.ravel(), at.ravel()
        for c in range(C):
            np.add.at(dx[n, c], idx[sel], dy[n, c].ravel()[sel])          # unbuffered: one addition after the other, in order
    return dx.reshape(N, C, H, W)


def fan_in(hom, H, W, stride=1):
    """-> [H, W] int64: how many outputs read each source pixel."""
    inside, at = nearest(hom, H, W, stride)
    return np.bincount(at.ravel()[inside.ravel()], minlength=H * W).reshape(H, W)


def inverse_corner_w(hom, H, W, guard=1.0 / 64):
    """-> [H, W, 4]: the inverse homography's w' at the four corners of every source pixel's guarded square."""
    inv = np.linalg.inv(np.asarray(hom, np.float64))
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.empty((H, W, 4))
    for k in range(4):
        cx = xs + (0.5 + guard if k & 1 else -0.5 - guard)
        cy = ys + (0.5 + guard if k & 2 else -0.5 - guard)
        u, v = 2.0 * cx / (W - 1) - 1.0, 2.0 * cy / (H - 1) - 1.0
        out[..., k] = inv[2, 0] * u + inv[2, 1] * v + inv[2, 2]
    return out


def cross_view_mse(depth, depth_aug, hom, weight=0.5, inside_only=False):
    """include/kp2d.h's kp2d_cross_view_mse in float64 -> dict(loss, d_depth, d_depth_aug, inside)."""
    depth, depth_aug = np.asarray(depth, np.float64), np.asarray(depth_aug, np.float64)
    N, H, W = depth.shape
    homs = _homs(hom, N)
    warped = warp(depth[:, None], homs, fill=0.0)[:, 0]
    inside = np.stack([nearest(homs[n], H, W)[0] for n in range(N)])
    counted = inside if inside_only else np.ones_like(inside)
    M = int(counted.sum())
    diff = (depth_aug - warped) * counted
    loss = weight * (diff ** 2).sum() / M if M else 0.0
    d_aug = weight * 2.0 * diff / M if M else np.zeros_like(diff)
    d_depth = warp_backward(-d_aug[:, None], homs, (H, W), dtype=np.float64)[:, 0]
    return {"loss": float(loss), "d_depth": d_depth, "d_depth_aug": d_aug, "inside": int(inside.sum())}


# ---- the sampler -----------------------------------------------------------------------------------------------------------------
def sample_homography(draws, shape, margins=None, **options):
    """One frame's nine draws (z0..z3, u_s, z_s, u_x, u_y, u_r) -> the reference's sample_homography(shape) [3,3] float64, by
    the steps include/kp2d.h lists.  ``margins``: a list that receives the distance of every discrete choice (the clips, the
    angle validity tests, the index floors) from its threshold."""
    o = dict(DEFAULTS, **options)
    d = [float(v) for v in draws]
    note = margins.append if margins is not None else (lambda v: None)
    hw = float(shape[0]) / float(shape[1])
    p1 = np.array([[-1.0, -1.0], [-1.0, 1.0], [1.0, -1.0], [1.0, 1.0]])
    p2 = p1 * o["patch_ratio"]
    p2[:, 1] *= hw
    if o["perspective"]:
        sx, sy = o["perspective_amplitude"] / 2, hw * o["perspective_amplitude"] / 2
        raw = [sx * d[0], sx * d[1], sy * d[2], sy * d[3]]
        for r, s in zip(raw, (sx, sx, sy, sy)):
            note(abs(abs(r) - s))
        ax0, ax1 = np.clip(raw[0], -sx, sx), np.clip(raw[1], -sx, sx)
        ay0, ay1 = np.clip(raw[2], -sy, sy), np.clip(raw[3], -sy, sy)
        p2 += np.array([[-ax1, -ay1], [-ax0, ay1], [ax1, -ay0], [ax0, ay0]])
    if o["scaling"]:
        t = d[4] * o["n_scales"]
        note(min(t - math.floor(t), math.floor(t) + 1 - t))
        idx = min(max(int(math.floor(t)), 0), o["n_scales"] - 1)
        s = 1.0
        if idx:
            half = o["scaling_amplitude"] / 2
            note(abs(abs(d[5] * half) - half))
            s = float(np.clip(1.0 + d[5] * half, 1.0 - half, 1.0 + half))
        c = p2.mean(axis=0, keepdims=True)
        p2 = (p2 - c) * s + c
    if o["translation"]:
        lim = np.array([1.0, hw])
        tmin, tmax = (p2 + lim).min(axis=0), (lim - p2).min(axis=0)
        p2 = p2 + (-tmin + (tmax + tmin) * np.array([d[6], d[7]]))[None]
    if o["rotation"]:
        n = o["n_angles"]
        angles = np.concatenate([[0.0], np.linspace(-o["max_angle"], o["max_angle"], n)])
        c = p2.mean(axis=0, keepdims=True)
        q = p2 - c
        cos, sin = np.cos(angles)[:, None], np.sin(angles)[:, None]
        rot = np.stack([q[None, :, 0] * cos + q[None, :, 1] * sin, q[None, :, 1] * cos - q[None, :, 0] * sin], axis=2) + c[None]
        lo, hi = np.array([-1.0, -hw]), np.array([1.0, hw])
        note(float(np.minimum(np.abs(rot - lo), np.abs(rot - hi)).min()))
        valid = np.nonzero(((rot >= lo) & (rot < hi)).all(axis=(1, 2)))[0]
        if len(valid):
            t = d[8] * len(valid)
            note(min(t - math.floor(t), math.floor(t) + 1 - t))
            p2 = rot[valid[min(max(int(math.floor(t)), 0), len(valid) - 1)]]
    p2 = p2.copy()
    p2[:, 1] /= hw
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        (px, py), (qx, qy) = p1[i], p2[i]
        A[2 * i] = [px, py, 1, 0, 0, 0, -px * qx, -py * qx]
        A[2 * i + 1] = [0, 0, 0, px, py, 1, -px * qy, -py * qy]
        b[2 * i], b[2 * i + 1] = qx, qy
    return np.concatenate([np.linalg.solve(A, b), [1.0]]).reshape(3, 3)


def sample_homographies(draws, shape, **options):
    return np.stack([sample_homography(d, shape, **options) for d in np.asarray(draws, np.float64)])


def view_corners(hom):
    """The four corners (+-1, +-1) of the second view in the first view's normalised coordinates [4, 2]."""
    p = np.array([[-1.0, -1.0, 1.0], [-1.0, 1.0, 1.0], [1.0, -1.0, 1.0], [1.0, 1.0, 1.0]]) @ np.asarray(hom, np.float64).T
    return p[:, :2] / p[:, 2:]


# ---- the draws: the counter layout of kp2d_homography_draws in Python integers ----------------------------------------------------
_M64 = (1 << 64) - 1


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw_hash(seed, step, frame, slot, k):
    return mix(mix(mix((seed + 0x9E3779B97F4A7C15) & _M64) ^ ((step << 32) | frame)) ^ ((slot << 32) | k))


def homography_draws(B, seed, step):
    """-> [B, 9] float64."""
    out = np.empty((B, SLOTS))
    for frame in range(B):
        for slot in range(SLOTS):
            ua = (draw_hash(seed, step, frame, slot, 0) >> 11) * 2.0 ** -53
            if slot in NORMAL_SLOTS:
                ub = (draw_hash(seed, step, frame, slot, 1) >> 11) * 2.0 ** -53
                ua = math.sqrt(-2.0 * math.log(1.0 - ua)) * math.cos(6.283185307179586 * ub)
            out[frame, slot] = ua
    return out


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
def sampler_cases():
    """-> {name: dict(shape, options)}: settings only (tests/golden/augment/cases.json)."""
    with open(os.path.join(GOLDEN, "cases.json")) as f:
        return json.load(f)


def load_sampler():
    return np.load(os.path.join(GOLDEN, "sampler.npz"))


def reference_homography(shape=(17, 23), which=0):
    """A matrix the reference's sampler returned for the fixture draws of the first case, as the oracle restates it at ``shape``."""
    fx, cases = load_sampler(), sampler_cases()
    name = sorted(cases)[0]
    return sample_homography(fx["draws_" + name][which], shape, **cases[name]["options"])
