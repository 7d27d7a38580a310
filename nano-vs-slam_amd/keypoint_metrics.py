"""Keypoint scores on the device: repeatability, localisation error and matching score.

* ``repeatability_stats`` / ``matching_score_stats`` — batches of image pairs on the HIP kernels of
  csrc/keypoint_metrics.hip (kp2d_kp_repeatability, kp2d_kp_matching_score; include/kp2d.h states every rule): device
  tensors in, device tensors of exact integer counts and float64 sums out, nothing synchronised.
* ``compute_repeatability`` / ``compute_matching_score`` — the reference's functions for one pair
  (src/evaluation/detector.py:8-115, src/evaluation/descriptor.py:85-172) with its ``data`` keys and return values; numpy
  arrays or device tensors.
* ``evaluate_keypoint_net`` — drop-in for the reference's loop (src/evaluation/keypoints.py:57-175): score, coordinate and
  descriptor maps stay on the device; one host read at the end.

What the reference computes with numpy and OpenCV per pair on the host is restated here.  ``compute_repeatability`` is pinned
by the reference's own code (tests/golden/keypoints/rep_*.npz).  ``compute_matching_score`` calls cv2.BFMatcher, which is not
installed, so its matcher step is restated, not pinned: the nearest neighbours come from kp2d_match_descriptors_ex.
Reproduced quirk: the box test holds x against image_shape[0] and y against image_shape[1], and the reference passes
image_shape = (H, W).  Tie rule: among equal probabilities the lower row is kept (numpy's argsort defines no order).
Out of scope: ``compute_homography`` (mutual matches + cv2.findHomography's RANSAC, whose random stream cannot be pinned
without OpenCV) and the correctness@1/3/5 and AUC values built on it: it raises, and ``evaluate_keypoint_net`` returns nan in
their places.  There is no CPU path behind the kernels: CPU tensors raise.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _dev, _lib
from ._dev import ptr as _ptr, stream as _stream

DESC_WIDTHS = (32, 64, 128)
CONF_THRESHOLD = 0.7                          # keypoints.py:84


def _dev_tensor(name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    return _dev.require_device(name, t).detach()


def _sets(pts0, cnt0, pts1, cnt1, hom):
    pts0, pts1, hom = _dev_tensor("pts0", pts0), _dev_tensor("pts1", pts1), _dev_tensor("hom", hom)
    cnt0, cnt1 = _dev_tensor("cnt0", cnt0), _dev_tensor("cnt1", cnt1)
    for name, t in (("pts0", pts0), ("pts1", pts1)):
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"{name} must be [B, k, 3] rows (x, y, prob), got {tuple(t.shape)}")
    B = pts0.shape[0]
    if B < 1 or pts1.shape[0] != B or cnt0.numel() != B or cnt1.numel() != B or hom.numel() != 9 * B:
        raise ValueError(f"batch sizes differ or are empty: pts0 {tuple(pts0.shape)}, pts1 {tuple(pts1.shape)}, cnt0 "
                         f"{tuple(cnt0.shape)}, cnt1 {tuple(cnt1.shape)}, hom {tuple(hom.shape)}")
    dev = pts0.device
    if any(t.device != dev for t in (pts1, cnt0, cnt1, hom)):
        raise ValueError("all tensors must live on the same device")
    return (pts0.to(torch.float32).contiguous(), cnt0.reshape(B).to(torch.int32).contiguous(),
            pts1.to(torch.float32).contiguous(), cnt1.reshape(B).to(torch.int32).contiguous(),
            hom.reshape(B, 9).to(torch.float64).contiguous())


def repeatability_stats(pts0, cnt0, pts1, cnt1, hom, image_shape, keep_k=300, distance_thresh=3):
    """kp2d_kp_repeatability on device tensors: pts0 [B,k0,3] / pts1 [B,k1,3] rows (x, y, prob), cnt0 / cnt1 [B] rows that
    exist, hom [B,3,3] (image 0 -> image 1), image_shape = (b0, b1) as the reference passes it ((H, W); x is held against
    b0) -> (counts [B,4] int64 = (N1, N2, count1, count2), le [B,2] float64 = (le1, le2)); nothing is synchronised.
    Outputs are bit-identical from run to run and whether a pair is scored alone or inside a batch."""
    pts0, cnt0, pts1, cnt1, hom = _sets(pts0, cnt0, pts1, cnt1, hom)
    B, k0, k1 = pts0.shape[0], pts0.shape[1], pts1.shape[1]
    dev = pts0.device
    lib = _lib.load()
    counts = torch.empty(B, 4, dtype=torch.int64, device=dev)
    le = torch.empty(B, 2, dtype=torch.float64, device=dev)
    scratch = _dev.scratch(lib.kp2d_kp_scratch_bytes(B, k0, k1, 0, int(keep_k)), dev)
    with torch.cuda.device(dev):
        _lib.check(lib.kp2d_kp_repeatability(_ptr(pts0), _ptr(cnt0), _ptr(pts1), _ptr(cnt1), _ptr(hom), B, k0, k1,
                                             float(image_shape[0]), float(image_shape[1]), int(keep_k), float(distance_thresh),
                                             _ptr(counts), _ptr(le), _ptr(scratch), scratch.numel(), _stream(dev)))
    return counts, le


def matching_score_stats(pts0, cnt0, desc0, pts1, cnt1, desc1, hom, image_shape, keep_k=1000):
    """kp2d_kp_matching_score on device tensors: as repeatability_stats plus desc0 [B,k0,C] / desc1 [B,k1,C], C in
    DESC_WIDTHS -> counts [B,4] int64 = (vis1, hit1, vis2, hit2); nothing is synchronised."""
    pts0, cnt0, pts1, cnt1, hom = _sets(pts0, cnt0, pts1, cnt1, hom)
    desc0, desc1 = _dev_tensor("desc0", desc0), _dev_tensor("desc1", desc1)
    B, k0, k1 = pts0.shape[0], pts0.shape[1], pts1.shape[1]
    dev = pts0.device
    if desc0.dim() != 3 or desc1.dim() != 3 or tuple(desc0.shape[:2]) != (B, k0) or tuple(desc1.shape[:2]) != (B, k1) \
            or desc0.shape[2] != desc1.shape[2] or desc0.device != dev or desc1.device != dev:
        raise ValueError(f"descriptors must be [B, k0, C] and [B, k1, C] on the points' device, got {tuple(desc0.shape)} and "
                         f"{tuple(desc1.shape)}")
    Cd = desc0.shape[2]
    desc0, desc1 = desc0.to(torch.float32).contiguous(), desc1.to(torch.float32).contiguous()
    lib = _lib.load()
    counts = torch.empty(B, 4, dtype=torch.int64, device=dev)
    scratch = _dev.scratch(lib.kp2d_kp_scratch_bytes(B, k0, k1, Cd if Cd in DESC_WIDTHS else 0, int(keep_k)), dev)
    with torch.cuda.device(dev):
        _lib.check(lib.kp2d_kp_matching_score(_ptr(pts0), _ptr(cnt0), _ptr(desc0), _ptr(pts1), _ptr(cnt1), _ptr(desc1), _ptr(hom),
                                              B, k0, k1, Cd, float(image_shape[0]), float(image_shape[1]), int(keep_k),
                                              _ptr(counts), _ptr(scratch), scratch.numel(), _stream(dev)))
    return counts


def repeatability_from_stats(counts, le):
    """counts [B,4], le [B,2] -> (repeatability [B], loc_err [B]) float64 (any device): (count1 + count2) / (N1 + N2) and
    (le1 + le2) / (count1 + count2), both -1 where the reference returns -1 (no row, or no correct row)."""
    n = (counts[:, 0] + counts[:, 1]).to(torch.float64)
    c = (counts[:, 2] + counts[:, 3]).to(torch.float64)
    ok = (n > 0) & (c > 0)
    one = torch.ones_like(n)
    minus = torch.full_like(n, -1.0)
    rep = torch.where(ok, c / torch.where(ok, n, one), minus)
    loc = torch.where(ok, (le[:, 0] + le[:, 1]) / torch.where(ok, c, one), minus)
    return rep, loc


def matching_score_from_stats(counts):
    """counts [B,4] -> ms [B] float64: (hit1 / max(vis1, 1) + hit2 / max(vis2, 1)) / 2."""
    c = counts.to(torch.float64)
    return (c[:, 1] / torch.clamp_min(c[:, 0], 1.0) + c[:, 3] / torch.clamp_min(c[:, 2], 1.0)) / 2.0


def _one(x, dtype, cols, name, dev):
    """One pair's [N, cols] array (numpy or device tensor) -> ([1, N, cols] device tensor, count [1] int32)."""
    if isinstance(x, torch.Tensor):
        t = _dev_tensor(name, x)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float64 if dtype == torch.float64 else np.float32)).to(dev)
    if cols is not None:
        t = t.reshape(-1, cols)
    if t.dim() != 2:
        raise ValueError(f"{name} must be two-dimensional, got {tuple(t.shape)}")
    return t.to(dtype).unsqueeze(0), torch.full((1,), t.shape[0], dtype=torch.int32, device=t.device)


def _pair_device(data):
    for key in ("prob", "warped_prob", "homography"):
        if isinstance(data[key], torch.Tensor):
            return _dev_tensor(key, data[key]).device
    return torch.device("cuda", torch.cuda.current_device())


def compute_repeatability(data, keep_k_points=300, distance_thresh=3):
    """The reference's compute_repeatability (src/evaluation/detector.py:8-115): ``data`` holds "image_shape" (H, W),
    "homography" [3,3], "prob" [N,3] and "warped_prob" [M,3] rows (x, y, probability), numpy arrays or device tensors (rows
    are taken as float32, what the model produces) -> (N1, N2, repeatability, loc_err) as Python numbers, (N1, N2, -1, -1)
    where the reference gives that.  The two divisions are float64."""
    dev = _pair_device(data)
    p0, c0 = _one(data["prob"], torch.float32, 3, "prob", dev)
    p1, c1 = _one(data["warped_prob"], torch.float32, 3, "warped_prob", dev)
    hom, _ = _one(data["homography"], torch.float64, 3, "homography", dev)
    counts, le = repeatability_stats(p0, c0, p1, c1, hom, data["image_shape"], keep_k_points, distance_thresh)
    rep, loc = repeatability_from_stats(counts, le)
    n1, n2, _, _ = counts[0].tolist()
    rep, loc = rep.item(), loc.item()
    return (n1, n2, -1, -1) if rep == -1.0 else (n1, n2, rep, loc)


def compute_matching_score(data, keep_k_points=1000):
    """The reference's compute_matching_score (src/evaluation/descriptor.py:85-172): ``data`` as compute_repeatability plus
    "desc" [N,C] and "warped_desc" [M,C] -> ms, a Python float (0.0 when either set is empty)."""
    dev = _pair_device(data)
    p0, c0 = _one(data["prob"], torch.float32, 3, "prob", dev)
    p1, c1 = _one(data["warped_prob"], torch.float32, 3, "warped_prob", dev)
    hom, _ = _one(data["homography"], torch.float64, 3, "homography", dev)
    d0, _ = _one(data["desc"], torch.float32, None, "desc", dev)
    d1, _ = _one(data["warped_desc"], torch.float32, None, "warped_desc", dev)
    if d0.shape[1] == 0 or d1.shape[1] == 0:            # `if not matches: return 0` (an empty side may come without a width)
        return 0.0
    counts = matching_score_stats(p0, c0, d0, p1, c1, d1, hom, data["image_shape"], keep_k_points)
    return matching_score_from_stats(counts).item()


def compute_homography(data, keep_k_points=1000, debug=False):
    """Not built: the reference fits a homography to mutual matches with cv2.findHomography's RANSAC
    (src/evaluation/descriptor.py:175-285), whose random stream cannot be pinned without OpenCV."""
    raise NotImplementedError("compute_homography (mutual matches + RANSAC homography fit, correctness@1/3/5 and AUC) is out "
                              "of this build's scope: only the deterministic keypoint scores (repeatability, localisation "
                              "error, matching score) run on the device")


def keypoint_rows(score, coord, feat, conf_threshold=CONF_THRESHOLD):
    """post_processing's maps score [B,1,Hc,Wc], coord [B,2,Hc,Wc], feat [B,C,Hc,Wc] -> (pts [B,n,3], desc [B,n,C],
    cnt [B] int32) with n = Hc * Wc: per image the cells with score > conf_threshold first, in raster order (the order the
    reference's boolean mask leaves them in, keypoints.py:113-128); rows past cnt are padding.  Device plumbing only."""
    B = score.shape[0]
    pts = torch.cat([coord, score], dim=1).reshape(B, 3, -1).transpose(1, 2)
    desc = feat.reshape(B, feat.shape[1], -1).transpose(1, 2)
    keep = pts[:, :, 2] > conf_threshold
    order = torch.argsort((~keep).to(torch.uint8), dim=1, stable=True)
    pts = torch.gather(pts, 1, order.unsqueeze(2).expand(-1, -1, 3)).contiguous()
    desc = torch.gather(desc, 1, order.unsqueeze(2).expand(-1, -1, desc.shape[2])).contiguous()
    return pts, desc, keep.sum(1).to(torch.int32)


def evaluate_keypoint_net(data_loader, keypoint_net, output_shape=(320, 240), top_k=300, debug=False, offset=0, tflite=False):
    """Drop-in for the reference's evaluate_keypoint_net (src/evaluation/keypoints.py:57-175): every sample {"image",
    "image_aug", "homography"} goes through the model and its post_processing twice; cells with score > 0.7 become the
    (x, y, prob) and descriptor rows ON THE DEVICE; repeatability and localisation error (pairs where they are -1 are left
    out, as in the reference) and the matching score are computed there with keep_k = top_k and image_shape =
    output_shape[::-1] -> the reference's 7-tuple (repeatability, localization_err, correctness1, correctness3,
    correctness5, MScore, auc).  A sample may hold several pairs ([B,3,H,W]; the reference's reshapes allow one).
    The three correctness values and the AUC are nan: they rest on compute_homography's RANSAC fit, which is out of this
    build's scope (no OpenCV to pin its random stream against).  ``debug`` / ``tflite`` variants are not reproduced.
    One host read at the end."""
    keypoint_net.eval()
    keypoint_net.training = False
    dev = _dev.model_device(keypoint_net)
    shape = tuple(output_shape[::-1])
    reps, locs, mss = [], [], []
    with torch.no_grad():
        for i, sample in enumerate(data_loader):
            if i < offset:
                continue
            image = sample["image"].to(dev)
            warped = sample["image_aug"].to(dev)
            B, _, H, W = image.shape
            hom = sample["homography"].to(dev).reshape(B, 3, 3)
            out = keypoint_net.post_processing(keypoint_net(image), H, W)
            p0, d0, c0 = keypoint_rows(out["score"], out["coord"], out["feat"])
            out = keypoint_net.post_processing(keypoint_net(warped), H, W)
            p1, d1, c1 = keypoint_rows(out["score"], out["coord"], out["feat"])
            rep, loc = repeatability_from_stats(*repeatability_stats(p0, c0, p1, c1, hom, shape, top_k, 3))
            reps.append(rep)
            locs.append(loc)
            mss.append(matching_score_from_stats(matching_score_stats(p0, c0, d0, p1, c1, d1, hom, shape, top_k)))
    nan = float("nan")
    if not reps:
        return nan, nan, nan, nan, nan, nan, nan
    rep, loc, ms = torch.cat(reps), torch.cat(locs), torch.cat(mss)
    ok = ((rep != -1.0) & (loc != -1.0)).to(torch.float64)
    n = ok.sum()
    res = torch.stack([(rep * ok).sum() / n, (loc * ok).sum() / n, ms.mean()]).tolist()     # 0 / 0 = nan: np.mean([])
    return res[0], res[1], nan, nan, nan, res[2], nan
