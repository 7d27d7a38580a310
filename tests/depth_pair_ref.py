"""The seeded inputs and the bounds of the depth head's PAIR step (DepthHeadTrainer.pair_gradients / step_pair_features): config
S's head (depth_training_ref's case C channel counts) on 2 pairs of 32 x 48 frames, i.e. backbone maps x [2, 64, 8, 12] and
skip [2, 64, 16, 24] per view, ground truth at the logits' 16 x 24, and a homography of the reference's sampler per pair.
Fixtures under tests/golden/depth_pair/ hold outputs, settings and the seed only (tools/make_depth_pair_golden.py wrote them
from the reference's SegmentationHead and SILogLoss with the warper restated by grid_sample); the inputs are regenerated here.
"""
import json
import os

import numpy as np

import augment_ref as ar
import depth_training_ref as dr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_pair")
sr = dr.sr
N, C_IN, C_HIDDEN, D1, C_SKIP, H8, W8 = 2, 64, 64, 128, 64, 8, 12
FRAME = (32, 48)
CROSS_WEIGHT = 0.5
STEPS = 5
BASE_SEED = 501
NEAREST_SAFE = 1e-3          # pixels: every nearest decision of a kept seed is further than this from a tie
PARTS = ("silog", "huber", "silog_aug", "huber_aug", "cross")
stored, rel_err, FLOOR, LR, TRAJ_STORED = dr.stored, dr.rel_err, dr.FLOOR, dr.LR, dr.TRAJ_STORED


def seed_of():
    with open(os.path.join(GOLDEN, "seed.json")) as f:
        return int(json.load(f)["pair"])


def make_inputs(seed=None):
    """-> depth_training_ref.make_inputs' dict for one view plus x_aug, skip_aug, gt_aug and homography float32 [N, 3, 3]."""
    rng = np.random.default_rng(seed_of() if seed is None else seed)

    def maps():
        x = (np.abs(rng.standard_normal((N, C_IN, H8, W8))) * 0.8 + 0.3 * rng.standard_normal((N, C_IN, 1, 1))).astype(np.float32)
        skip = (np.abs(rng.standard_normal((N, C_SKIP, 2 * H8, 2 * W8))) * 0.8 + 0.3 * rng.standard_normal((N, C_SKIP, 1, 1))).astype(np.float32)
        return x, skip

    x, skip = maps()
    x_aug, skip_aug = maps()
    gt = dr._draw_gt(rng, (N, 2 * H8, 2 * W8))
    draws = np.empty((N, ar.SLOTS))
    draws[:, list(ar.NORMAL_SLOTS)] = rng.standard_normal((N, len(ar.NORMAL_SLOTS)))
    draws[:, [4, 6, 7, 8]] = rng.random((N, 4))
    hom = ar.sample_homographies(draws, FRAME).astype(np.float32)
    gt_aug = ar.warp(gt[:, None], hom.astype(np.float64), fill=0.0)[:, 0]          # what view_pair hands the trainer
    params, stats = [], []
    for i, (ci, co) in enumerate(sr.layer_channels(C_IN, C_HIDDEN, D1, C_SKIP, 1)):
        wgt = (rng.standard_normal((co, ci, 3, 3)) * np.sqrt(2.0 / (9 * ci))).astype(np.float32)
        if i < 8:
            gamma, beta = rng.uniform(0.5, 1.5, co), 0.2 * rng.standard_normal(co)
            stats.append(((0.3 * rng.standard_normal(co)).astype(np.float32), rng.uniform(0.5, 1.5, co).astype(np.float32)))
            params += [wgt, gamma.astype(np.float32), beta.astype(np.float32)]
        else:
            params += [wgt, (0.2 * rng.standard_normal(co)).astype(np.float32)]
    return {"x": x, "skip": skip, "gt": gt, "x_aug": x_aug, "skip_aug": skip_aug, "gt_aug": gt_aug, "homography": hom, "params": params,
            "stats": stats, "weights": dr.WEIGHTS, "N": N, "c_in": C_IN, "c_hidden": C_HIDDEN, "d1": D1, "c_skip": C_SKIP, "classes": 1,
            "h": H8, "w": W8}


def nearest_margin(hom, H, W):
    """The smallest distance, in pixels, of a coordinate near the map from a rounding tie, over the batch."""
    worst = np.inf
    for h in np.asarray(hom, np.float64):
        px, py = ar.src_coords(h, H, W)
        near = (px > -1) & (px < W) & (py > -1) & (py < H)
        for p in (px[near], py[near]):
            worst = min(worst, float(np.abs(p - np.floor(p) - 0.5).min())) if p.size else worst
    return worst


def load_fixture():
    return np.load(os.path.join(GOLDEN, "pair.npz"))


def bounds():
    """-> dict per quantity (loss, the five parts, g0..g25, loss_traj, p0_traj..p25_traj): max(8 x the reference modules' own
    float32 error of that quantity, 16 x 2^-24)."""
    fx = load_fixture()
    return {k[6:]: max(8.0 * float(fx[k]), FLOOR) for k in fx.files if k.startswith("err32_")}
