"""Scores of the dense heads (csrc/dense_metrics.hip, nano_vs_slam_amd.dense_metrics) on the MI355X against the numpy
oracle of tests/dense_ref.py: segmentation counts exactly, depth sums within the header's bound, the metrics, the bit
identities, the Python surface and both evaluate_* functions end to end on the model's own outputs."""
import functools
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

import dense_ref as dr
from conftest import ROOT
from nano_vs_slam_amd import dense_metrics as dm

pytestmark = pytest.mark.gpu
SEG_SHAPES = {"small": (3, 37, 53, ("mixed", "ignored", "equal")), "large": (2, 240, 320, ("mixed", "single"))}
DTYPES = (np.uint8, np.int32, np.int64)
SCORES = {"iou": dm.iou_score, "accuracy": dm.accuracy, "f1": dm.f1_score}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # a copy: the shared inputs are read-only


def host(*ts):
    return [t.cpu().numpy() for t in ts]


def classes(c):
    return dm.seg_conf_lds_max() + {"lds_max": 0, "lds_max+1": 1}[c] if isinstance(c, str) else c


def check_seg(pred, target, C, ignore, label):
    want = dr.seg_stats(pred.reshape(len(pred), -1), target.reshape(len(target), -1), C, ignore)
    got = host(*dm.seg_stats(dev(pred), dev(target), C, ignore, confusion=True))
    for name, g, w in zip(("stats", "confusion", "ignored", "stray"), got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w), (label, name)
    n = pred[0].size
    assert np.all(got[0].sum(2) == (n - got[2] - got[3])[:, None])      # tp + fp + fn + tn = counted, for every class
    without = dm.seg_stats(dev(pred), dev(target), C, ignore)           # no confusion matrix: the same counts
    assert without[1] is None and np.array_equal(without[0].cpu().numpy(), want[0]), (label, "stats alone")
    return got


@pytest.mark.parametrize("shape", sorted(SEG_SHAPES))
@pytest.mark.parametrize("C", [1, 2, 19, 28, 150, 256, "lds_max", "lds_max+1"])
def test_seg_counts_are_exact(C, shape):
    C = classes(C)
    B, H, W, kinds = SEG_SHAPES[shape]
    for dtype in DTYPES:
        pred, target = dr.seg_case(B, H, W, C, dtype, 100 * C + H, kinds)
        _, _, ignored, stray = check_seg(pred, target, C, 255, f"{shape}:C{C}:{np.dtype(dtype).name}")
        if "ignored" in kinds:
            assert ignored[kinds.index("ignored")] == H * W
        assert 0.05 * H * W < ignored[0] < 0.15 * H * W and stray[0] > 0
        if "equal" in kinds:
            i = kinds.index("equal")                  # nothing planted there; with C = 256 class 255 IS the ignore index
            assert ignored[i] == (target[i] == 255).sum() == (0 if C < 256 else ignored[i]) and stray[i] == 0


@pytest.mark.parametrize("C", [19, 256])
def test_seg_without_ignore_index(C):
    B, H, W, kinds = SEG_SHAPES["small"]
    for dtype in DTYPES:
        # planted with 255 as the ignore value, scored with none: 255 is then a stray value (C = 19) or a class (C = 256)
        pred, target = dr.seg_case(B, H, W, C, dtype, 7 + C, ("mixed", "mixed", "equal"))
        _, _, ignored, stray = check_seg(pred, target, C, None, f"none:C{C}:{np.dtype(dtype).name}")
        assert not ignored.any()
        assert stray[0] > (0.05 * H * W if C == 19 else 0)


def test_seg_wide_class_range_and_odd_ignore_index():
    rng = np.random.default_rng(5)
    target = rng.integers(0, 1024, (2, 1, 50, 41)).astype(np.int32)
    pred = np.where(rng.random(target.shape) < 0.5, target, rng.integers(0, 1024, target.shape)).astype(np.int64)
    target[0, 0, :5] = -7
    want = dr.seg_stats(pred.reshape(2, -1), target.reshape(2, -1), 1024, -7)
    stats, conf, ignored, stray = dm.seg_stats(dev(pred), dev(target), 1024, -7)
    assert conf is None and np.array_equal(stats.cpu().numpy(), want[0]) and ignored.tolist() == [5 * 41, 0] and not stray.any()
    with pytest.raises(ValueError, match="confusion"):
        dm.confusion_matrix(dev(pred), dev(target), 1024)
    # an ignore index inside the class range takes that class out of the counts
    want = dr.seg_stats(pred.reshape(2, -1), target.reshape(2, -1), 1024, 3)
    tp, fp, fn, tn = dm.get_stats(dev(pred), dev(target), num_classes=1024, ignore_index=3)
    assert np.array_equal(torch.stack([tp, fp, fn, tn], -1).cpu().numpy(), want[0]) and int(fn[:, 3].sum()) == 0


@pytest.mark.parametrize("reduction", dr.REDUCTIONS)
def test_scores_in_every_reduction(reduction):
    B, H, W, kinds = SEG_SHAPES["small"]
    pred, target = dr.seg_case(B, H, W, 19, np.uint8, 11, kinds)
    want = dr.seg_stats(pred.reshape(B, -1), target.reshape(B, -1), 19, 255)[0]
    st = dm.get_stats(dev(pred), dev(target), mode="multiclass", num_classes=19, ignore_index=255)
    assert all(t.is_cuda and t.dtype == torch.int64 and tuple(t.shape) == (B, 19) for t in st)
    for kind, fn in SCORES.items():
        for zd in (1.0, 0.0):
            got = fn(*st, reduction=reduction, zero_division=zd)
            assert got.is_cuda and got.dtype == torch.float64
            assert np.abs(got.cpu().numpy() - dr.score(kind, want, reduction, zd)).max() <= 1e-12, (kind, reduction)


def depth_call(shape, limits=dr.DEPTH_LIMITS, with_valid=True):
    gt, pred, valid = dr.depth_case(*shape)
    return dm.depth_sums(dev(gt), dev(pred), dev(valid) if with_valid else None, *limits)


@functools.lru_cache(maxsize=None)
def depth_oracle(shape):
    gt, pred, valid = dr.depth_case(*shape)
    return dr.depth_sums(gt, pred, valid, *dr.DEPTH_LIMITS)


@pytest.mark.parametrize("shape", dr.DEPTH_SHAPES)
def test_depth_sums_within_the_bound(shape):
    gt, pred, valid = dr.depth_case(*shape)
    got = depth_call(shape).cpu().numpy()
    want = depth_oracle(shape)
    assert got.dtype == np.float64 and got.shape == (shape[0], dr.NSUMS)
    n = gt[0].size
    for b in range(shape[0]):
        for s in (0, 1, 2, 3, 10):
            assert got[b, s] == want[b, s], (b, s)
        assert got[b, 0] + got[b, 10] == n and want[b, 10] > 8
        ok = dr.depth_valid(gt[b], pred[b], valid[b], *dr.DEPTH_LIMITS)
        bound = dr.depth_bounds(gt[b][ok], pred[b][ok], n)
        for s in dr.FLOAT_SLOTS:
            err = abs(got[b, s] - want[b, s])
            print(f"{shape} image {b} slot {s}: error {err:.3e} uses {err / bound[s]:.4f} of the bound {bound[s]:.3e}")
            assert err <= bound[s], (b, s)
    # no mask, no limits: only the planted zeros, negatives, NaN and inf are invalid
    bare = depth_call(shape, (None, None), False).cpu().numpy()
    assert np.array_equal(bare[:, [0, 1, 2, 3, 10]], dr.depth_sums(gt, pred)[:, [0, 1, 2, 3, 10]]) and np.all(bare[:, 10] == 8)


@pytest.mark.parametrize("shape", dr.DEPTH_SHAPES)
def test_depth_metrics(shape):
    gt, pred, valid = dr.depth_case(*shape)
    got = dm.compute_errors_torch(dev(gt), dev(pred), dev(valid), *dr.DEPTH_LIMITS)
    want = dr.compute_errors(gt, pred, valid, *dr.DEPTH_LIMITS)
    assert tuple(got) == dr.DEPTH_KEYS
    for k in dr.DEPTH_KEYS:
        print(f"{shape} {k}: {got[k]!r} against {want[k]!r}")
        assert abs(got[k] - want[k]) <= 1e-10 * abs(want[k]), k


def test_depth_bit_identities():
    shape = (3, 240, 320)
    gt, pred, valid = dr.depth_case(*shape)
    a, b = depth_call(shape), depth_call(shape)
    assert torch.equal(a, b)
    alone = dm.depth_sums(dev(gt[1:2]), dev(pred[1:2]), dev(valid[1:2]), *dr.DEPTH_LIMITS)
    assert torch.equal(alone[0], a[1])
    small = depth_call(dr.DEPTH_SHAPES[0])
    g0, p0, v0 = dr.depth_case(*dr.DEPTH_SHAPES[0])
    assert torch.equal(dm.depth_sums(dev(g0[1:2]), dev(p0[1:2]), dev(v0[1:2]), *dr.DEPTH_LIMITS)[0], small[1])


def test_depth_image_without_a_valid_pixel():
    gt, pred, _ = dr.depth_case(*dr.DEPTH_SHAPES[0])
    gt = gt.copy()
    gt[1] = -1.0
    sums = dm.depth_sums(dev(gt), dev(pred))
    n = gt[0].size
    assert sums[1].tolist() == [0.0] * 10 + [float(n)] and float(sums[0, 0]) == n - 8
    assert bool(torch.isnan(dm.metrics_from_sums(sums[1])).all())
    only = dm.compute_errors_torch(dev(gt[1:2]), dev(pred[1:2]))
    assert tuple(only) == dr.DEPTH_KEYS and all(math.isnan(v) for v in only.values())
    masked = dm.depth_sums(dev(gt), dev(pred), torch.zeros(gt.shape, dtype=torch.uint8, device="cuda"))
    assert torch.equal(masked[:, 0], torch.zeros(3, dtype=torch.float64, device="cuda")) and masked[:, 10].tolist() == [float(n)] * 3


def test_surface():
    B, H, W, kinds = SEG_SHAPES["small"]
    pred, target = dr.seg_case(B, H, W, 28, np.int64, 3, kinds)
    p, t = dev(pred), dev(target)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        dm.get_stats(p.cpu(), t, num_classes=28)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        dm.confusion_matrix(p, t.cpu(), 28)
    with pytest.raises(ValueError, match="elements per image"):
        dm.get_stats(p, t[:, :, :-1], num_classes=28)
    with pytest.raises(ValueError, match="batch"):
        dm.get_stats(p, t[:2], num_classes=28)
    with pytest.raises(TypeError, match="integer"):
        dm.get_stats(p.float(), t, num_classes=28)
    flat = dm.get_stats(p, t, num_classes=28, ignore_index=255)
    boxed = dm.get_stats(p[:, None], t[:, None], num_classes=28, ignore_index=255)
    mixed = dm.get_stats(p[:, None], t, num_classes=28, ignore_index=255)
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(flat, boxed, mixed))
    ps, ts = p[:, 3:30:2, 5:], t[:, 3:30:2, 5:]                       # a strided window of both maps
    assert not ps.is_contiguous()
    sliced = dm.get_stats(ps, ts, num_classes=28, ignore_index=255)
    assert all(torch.equal(a, b) for a, b in zip(sliced, dm.get_stats(ps.contiguous(), ts.contiguous(), num_classes=28,
                                                                      ignore_index=255)))
    assert torch.equal(dm.confusion_matrix(ps, ts, 28, 255), dm.confusion_matrix(ps.contiguous(), ts.contiguous(), 28, 255))
    assert int(sliced[0].sum()) > 0
    gt, dp, valid = (dev(a) for a in dr.depth_case(*dr.DEPTH_SHAPES[0]))
    with pytest.raises(RuntimeError, match="CPU tensors"):
        dm.depth_sums(gt.cpu(), dp)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        dm.compute_errors_torch(gt, dp, valid.cpu())
    with pytest.raises(ValueError, match="elements per image"):
        dm.depth_sums(gt, dp[:, :, :-1])
    whole = dm.depth_sums(gt, dp, valid)
    assert torch.equal(whole, dm.depth_sums(gt[:, None], dp[:, None], valid[:, None]))
    assert torch.equal(whole, dm.depth_sums(gt, dp, valid != 0))                   # a boolean mask is a mask
    gs, ds, vs = gt[:, 1::2, 3:], dp[:, 1::2, 3:], valid[:, 1::2, 3:]
    assert torch.equal(dm.depth_sums(gs, ds, vs), dm.depth_sums(gs.contiguous(), ds.contiguous(), vs.contiguous()))


@functools.lru_cache(maxsize=None)
def end_to_end():
    """KP2DTinyV2 config S with depth=True and 28 classes on seeded synthetic weights, three batches of two 64 x 96 frames
    with seeded labels -> (model, batches, host copies of the model's own class maps and depth maps per batch)."""
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import KP2DTinyV2, get_config
    from nano_vs_slam_amd.synthetic import spread_state_dict
    model = KP2DTinyV2(**get_config("S"), nClasses=28, depth=True)
    sd = spread_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to("cuda:0").eval()
    model.training = False
    model.device = "cuda:0"
    rng = np.random.default_rng(2024)
    batches, outs = [], []
    with torch.no_grad():
        for _ in range(3):
            img = torch.from_numpy(rng.uniform(-1, 1, (2, 3, 64, 96)).astype(np.float32))
            out = model.post_processing(model(img.cuda()), 64, 96)
            seg, depth = out["seg"].cpu().numpy(), out["depth"].cpu().numpy()
            labels = rng.integers(0, 28, seg.shape).astype(np.uint8)
            labels[rng.random(seg.shape) < 0.05] = 255
            gt = rng.uniform(0.05, 1.5, depth.shape).astype(np.float32)
            batches.append({"image": img, "seg": torch.from_numpy(labels), "depth": torch.from_numpy(gt)})
            outs.append((seg, depth))
    return model, batches, outs


def test_evaluate_segmentation_end_to_end():
    model, batches, outs = end_to_end()
    got = dm.evaluate_segmentation(model, batches, 28)
    want = dr.evaluate_segmentation([(seg.reshape(2, -1), b["seg"].numpy().reshape(2, -1)) for (seg, _), b in zip(outs, batches)], 28)
    assert list(got) == ["IoU", "accuracy", "f1", "IoU_macro"]
    for k, v in want.items():
        print(f"{k}: {got[k]!r} against {v!r}")
        assert isinstance(got[k], float) and abs(got[k] - v) <= 1e-12, k
    assert 0 < got["IoU"] < 1 and outs[0][0].shape == (2, 1, 32, 48)
    one = dm.evaluate_segmentation(model, batches[:1], 28)               # a single batch: the reference divides by zero here
    st = dr.seg_stats(outs[0][0].reshape(2, -1), batches[0]["seg"].numpy().reshape(2, -1), 28, 255)[0]
    assert abs(one["IoU"] - dr.score("iou", st, "micro-imagewise")) <= 1e-12


def test_evaluate_depth_estimation_end_to_end():
    model, batches, outs = end_to_end()
    got = dm.evaluate_depth_estimation(model, batches)
    per_batch = [dr.compute_errors(b["depth"].numpy(), depth) for (_, depth), b in zip(outs, batches)]
    assert tuple(got) == dr.DEPTH_KEYS
    for k in dr.DEPTH_KEYS:
        want = float(np.mean([m[k] for m in per_batch]))
        print(f"{k}: {got[k]!r} against {want!r}")
        assert isinstance(got[k], float) and abs(got[k] - want) <= 1e-10 * abs(want), k


def test_aliases_resolve_to_the_same_functions():
    src = os.path.join(ROOT, "src")
    sys.path.insert(0, src)
    try:
        for name in ("evaluation", "evaluation.segmentation", "evaluation.depth_estimation"):
            sys.modules.pop(name, None)
        seg = importlib.import_module("evaluation.segmentation")
        dep = importlib.import_module("evaluation.depth_estimation")
        assert seg.evaluate_segmentation is dm.evaluate_segmentation and seg.get_stats is dm.get_stats
        assert dep.evaluate_depth_estimation is dm.evaluate_depth_estimation and dep.compute_errors_torch is dm.compute_errors_torch
        assert not {"segmentation_models_pytorch", "cv2"} & set(sys.modules)
    finally:
        sys.path.remove(src)
