"""Scores of the two dense heads on the device: segmentation and depth.

* ``get_stats`` / ``confusion_matrix`` — per-image, per-class tp / fp / fn / tn with segmentation_models_pytorch's
  surface (``smp.metrics.get_stats(mode="multiclass")``) on the HIP kernels of csrc/dense_metrics.hip (kp2d_seg_stats,
  include/kp2d.h).  ``iou_score``, ``accuracy``, ``f1_score`` reduce those counts as smp.metrics does: a few float64
  torch operations on [B, C] tensors, on whichever device the counts live (these alone also run on CPU tensors).
* ``depth_sums`` / ``compute_errors_torch`` — the sums behind the reference's nine depth metrics
  (src/evaluation/depth_estimation.py:58-83) in float64 (kp2d_depth_sums), and the metrics formed from them.
* ``evaluate_segmentation`` / ``evaluate_depth_estimation`` — drop-ins for the reference's functions
  (src/evaluation/segmentation.py:8-91, src/evaluation/depth_estimation.py:85-126); no class map or depth map is copied
  to the host, one read at the end fetches the scores.

smp is not a dependency and was not available to compare with: the counting rule and the reductions are restated from its
definitions (include/kp2d.h states the rule).  There is no CPU path behind the kernels: CPU tensors raise.
"""
from __future__ import annotations

import torch

from . import _dev, _lib
from ._dev import ptr as _ptr, stream as _stream

SEG_MAX_CLASSES = 1024
SEG_CONF_MAX_CLASSES = 256
SEG_NO_IGNORE = -2 ** 63                      # KP2D_SEG_NO_IGNORE
DEPTH_NSUMS = 11                              # KP2D_DEPTH_NSUMS
DEPTH_SUMS = ("count", "a1", "a2", "a3", "abs_rel", "sq_rel", "sq", "log_sq", "log_diff", "log_10", "n_invalid")
DEPTH_KEYS = ("a1", "a2", "a3", "abs_rel", "sq_rel", "rmse", "rmse_log", "silog", "log_10")
_TARGET_DTYPES = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}      # KP2D_SEG_U8 / _I32 / _I64
_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
REDUCTIONS = (None, "micro", "macro", "micro-imagewise", "macro-imagewise")


def seg_conf_lds_max() -> int:
    """Largest class count whose confusion matrix is gathered in an LDS tile; above it (up to SEG_CONF_MAX_CLASSES) the
    kernel adds to global memory per pixel.  Same results on both sides (kp2d_seg_conf_lds_max)."""
    return int(_lib.load().kp2d_seg_conf_lds_max())


def _maps(output, target):
    """[B, H, W] / [B, 1, H, W] integer class maps -> (pred [B, n] int64, target [B, n] uint8 / int32 / int64), contiguous."""
    for name, t in (("output", output), ("target", target)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor")
        _dev.require_device(name, t)
        if t.dtype not in _INT_DTYPES:
            raise TypeError(f"{name} must hold integer class ids, got {t.dtype}")
        if t.dim() < 2:
            raise ValueError(f"{name} must be [B, H, W] or [B, 1, H, W], got {tuple(t.shape)}")
    if output.device != target.device:
        raise ValueError("output and target must live on the same device")
    B = output.shape[0]
    if target.shape[0] != B or B < 1:
        raise ValueError(f"batch sizes differ or are empty: output {tuple(output.shape)}, target {tuple(target.shape)}")
    pred = output.detach().reshape(B, -1).to(torch.int64).contiguous()
    tgt = target.detach().reshape(B, -1)
    tgt = (tgt if tgt.dtype in _TARGET_DTYPES else tgt.to(torch.int64)).contiguous()
    if pred.shape[1] != tgt.shape[1] or pred.shape[1] < 1:
        raise ValueError(f"output has {pred.shape[1]} elements per image, target {tgt.shape[1]}")
    return pred, tgt


def seg_stats(output, target, num_classes, ignore_index=None, confusion=False):
    """kp2d_seg_stats on device tensors -> (stats [B, C, 4] int64 = (tp, fp, fn, tn), confusion [B, C, C] int64 or None,
    ignored [B], stray [B]); nothing is synchronised.  Pixels whose target is ``ignore_index`` count as ignored only;
    other pixels with a class outside [0, C) on either side count as stray only."""
    C_ = int(num_classes)
    if C_ < 1 or C_ > SEG_MAX_CLASSES:
        raise ValueError(f"num_classes = {num_classes} outside [1, {SEG_MAX_CLASSES}]")
    if confusion and C_ > SEG_CONF_MAX_CLASSES:
        raise ValueError(f"the confusion matrix is built for num_classes <= {SEG_CONF_MAX_CLASSES}, got {C_}")
    ignore = SEG_NO_IGNORE if ignore_index is None else int(ignore_index)
    if ignore_index is not None and not -2 ** 63 < ignore < 2 ** 63:
        raise ValueError(f"ignore_index = {ignore_index} is no int64 (or is the 'none' sentinel)")
    pred, tgt = _maps(output, target)
    B, n = pred.shape
    dev = pred.device
    stats = torch.empty(B, C_, 4, dtype=torch.int64, device=dev)
    conf = torch.empty(B, C_, C_, dtype=torch.int64, device=dev) if confusion else None
    ignored = torch.empty(B, dtype=torch.int64, device=dev)
    stray = torch.empty(B, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().kp2d_seg_stats(_ptr(pred), _ptr(tgt), _TARGET_DTYPES[tgt.dtype], B, n, C_, ignore, _ptr(stats),
                                              _ptr(conf), _ptr(ignored), _ptr(stray), _stream(dev)))
    return stats, conf, ignored, stray


def get_stats(output, target, mode="multiclass", num_classes=None, ignore_index=None):
    """smp.metrics.get_stats for class maps: -> tp, fp, fn, tn, each [B, C] int64 on the device.  ``output`` / ``target``:
    [B, H, W] or [B, 1, H, W] integer tensors with the same number of elements per image."""
    if mode != "multiclass":
        raise ValueError(f"mode {mode!r} is not built: only 'multiclass' (integer class maps) is")
    if num_classes is None:
        raise ValueError("num_classes is required for mode 'multiclass'")
    stats, _, _, _ = seg_stats(output, target, num_classes, ignore_index)
    return stats[..., 0], stats[..., 1], stats[..., 2], stats[..., 3]


def confusion_matrix(output, target, num_classes, ignore_index=None):
    """-> [B, C, C] int64, row = target class, column = predicted class, of the counted pixels (see seg_stats)."""
    return seg_stats(output, target, num_classes, ignore_index, confusion=True)[1]


# ---- reductions: smp.metrics.functional._compute_metric restated; plain torch, float64, any device ----------------
def _score(num, den, zero_division):
    num, den = num.to(torch.float64), den.to(torch.float64)
    zero = den == 0
    out = num / torch.where(zero, torch.ones_like(den), den)
    return torch.where(zero, torch.full_like(out, float(zero_division)), out)


def _reduce(ratio, tp, fp, fn, tn, reduction, zero_division):
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction {reduction!r} is not built (weighted reductions are not); one of {REDUCTIONS}")
    if isinstance(zero_division, str):
        raise ValueError(f"zero_division={zero_division!r} is not built: pass the number a 0/0 score becomes")
    if not (tp.dim() == 2 and tp.shape == fp.shape == fn.shape == tn.shape):
        raise ValueError("tp, fp, fn, tn must be four [B, C] tensors")
    if reduction == "micro":
        tp, fp, fn, tn = (t.sum() for t in (tp, fp, fn, tn))
    elif reduction == "macro":
        tp, fp, fn, tn = (t.sum(0) for t in (tp, fp, fn, tn))
    elif reduction == "micro-imagewise":
        tp, fp, fn, tn = (t.sum(1) for t in (tp, fp, fn, tn))
    score = _score(*ratio(tp, fp, fn, tn), zero_division)
    return score if reduction is None else score.mean()


def iou_score(tp, fp, fn, tn, reduction=None, zero_division=1.0):
    """tp / (tp + fp + fn).  ``reduction``: None -> [B, C]; "micro": counts summed over images and classes, then scored;
    "macro": summed over images, scored per class, mean; "micro-imagewise": summed over classes, scored per image, mean;
    "macro-imagewise": scored per image and class, mean.  A 0/0 score becomes ``zero_division``."""
    return _reduce(lambda tp, fp, fn, tn: (tp, tp + fp + fn), tp, fp, fn, tn, reduction, zero_division)


def accuracy(tp, fp, fn, tn, reduction=None, zero_division=1.0):
    """(tp + tn) / (tp + fp + fn + tn); reductions as iou_score."""
    return _reduce(lambda tp, fp, fn, tn: (tp + tn, tp + fp + fn + tn), tp, fp, fn, tn, reduction, zero_division)


def f1_score(tp, fp, fn, tn, reduction=None, zero_division=1.0):
    """2 tp / (2 tp + fn + fp); reductions as iou_score."""
    return _reduce(lambda tp, fp, fn, tn: (2 * tp, 2 * tp + fn + fp), tp, fp, fn, tn, reduction, zero_division)


def evaluate_segmentation(model, dataloader, n_classes, debug=False):
    """Drop-in for the reference's evaluate_segmentation (src/evaluation/segmentation.py:8-91): every sample
    {"image", "seg"} goes through the model and its post_processing, the class map is scored against ``seg`` with
    ``ignore_index=255``, and the per-batch "micro-imagewise" IoU / accuracy / F1 and "macro-imagewise" IoU are averaged
    -> {"IoU", "accuracy", "f1", "IoU_macro"}.  The batch scores accumulate on the device; one host read at the end.
    Deviation: the sums are divided by the NUMBER OF BATCHES.  The reference divides by the last loop index, one less than
    that, which overstates every score and divides by zero on a single batch.  ``debug`` windows are not reproduced."""
    model.eval()
    model.training = False
    dev = _dev.model_device(model)
    total, batches = None, 0
    with torch.no_grad():
        for sample in dataloader:
            img = sample["image"].to(dev)
            seg_gt = sample["seg"].to(dev)
            H, W = img.shape[2], img.shape[3]
            out = model.post_processing(model(img), H, W)
            st = get_stats(out["seg"], seg_gt, mode="multiclass", num_classes=n_classes, ignore_index=255)
            scores = torch.stack([iou_score(*st, reduction="micro-imagewise"), accuracy(*st, reduction="micro-imagewise"),
                                  f1_score(*st, reduction="micro-imagewise"), iou_score(*st, reduction="macro-imagewise")])
            total = scores if total is None else total + scores
            batches += 1
    if batches == 0:
        raise ValueError("evaluate_segmentation: the dataloader is empty")
    iou, acc, f1, iou_macro = (total / batches).tolist()
    return {"IoU": iou, "accuracy": acc, "f1": f1, "IoU_macro": iou_macro}


# ---- depth ------------------------------------------------------------------------------------------------------
def _depth_maps(gt, pred, valid):
    for name, t in (("gt", gt), ("pred", pred)) + ((("valid", valid),) if valid is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor")
        _dev.require_device(name, t)
        if t.dim() < 2 or t.shape[0] != gt.shape[0] or t.device != gt.device:
            raise ValueError(f"{name} must be [B, ...] on gt's device with gt's batch size, got {tuple(t.shape)}")
    B = gt.shape[0]
    g = gt.detach().reshape(B, -1).to(torch.float32).contiguous()
    p = pred.detach().reshape(B, -1).to(torch.float32).contiguous()
    if B < 1 or g.shape[1] < 1 or g.shape[1] != p.shape[1]:
        raise ValueError(f"gt has {g.shape[1]} elements per image, pred {p.shape[1]}")
    v = None
    if valid is not None:
        v = valid.detach().reshape(B, -1)
        if v.shape[1] != g.shape[1]:
            raise ValueError(f"valid has {v.shape[1]} elements per image, gt {g.shape[1]}")
        v = (v if v.dtype == torch.uint8 else (v != 0).to(torch.uint8)).contiguous()
    return g, p, v


def depth_sums(gt, pred, valid=None, min_depth=None, max_depth=None):
    """kp2d_depth_sums on device tensors -> [B, DEPTH_NSUMS] float64, per image the sums named in DEPTH_SUMS over its
    valid pixels; nothing is synchronised.  A pixel is invalid (left out, tallied in the last slot) when gt or pred is
    non-finite or <= 0, gt lies outside [min_depth, max_depth] (None: no limit), or ``valid`` is 0 there.  Rows are
    bit-identical from run to run and whether an image is evaluated alone or inside a batch."""
    g, p, v = _depth_maps(gt, pred, valid)
    B, n = g.shape
    dev = g.device
    lib = _lib.load()
    sums = torch.empty(B, DEPTH_NSUMS, dtype=torch.float64, device=dev)
    ws = _dev.scratch(lib.kp2d_depth_scratch_bytes(B, n), dev)
    lo = float("nan") if min_depth is None else float(min_depth)
    hi = float("nan") if max_depth is None else float(max_depth)
    with torch.cuda.device(dev):
        _lib.check(lib.kp2d_depth_sums(_ptr(g), _ptr(p), _ptr(v), B, n, lo, hi, _ptr(sums), _ptr(ws), ws.numel(),
                                       _stream(dev)))
    return sums


def metrics_from_sums(sums):
    """One row of DEPTH_NSUMS sums -> the nine metrics [9] float64 in DEPTH_KEYS order (any device).  count = 0 gives NaN.
    silog = 100 sqrt(mean(e^2) - mean(e)^2), the difference clamped at 0 (rounding can leave it a hair below)."""
    s = sums.to(torch.float64)
    cnt = s[0]
    m = s[1:10] / cnt
    silog = 100.0 * torch.sqrt(torch.clamp_min(m[6] - m[7] * m[7], 0.0))
    return torch.stack([m[0], m[1], m[2], m[3], m[4], torch.sqrt(m[5]), torch.sqrt(m[6]), silog, m[8]])


def _batch_metrics(gt, pred, valid=None, min_depth=None, max_depth=None):
    rows = depth_sums(gt, pred, valid, min_depth, max_depth)
    tot = rows[0]
    for b in range(1, rows.shape[0]):          # the image rows in index order: the total is reproducible too
        tot = tot + rows[b]
    return metrics_from_sums(tot)


def compute_errors_torch(gt, pred, valid=None, min_depth=None, max_depth=None):
    """The reference's compute_errors_torch (src/evaluation/depth_estimation.py:58-83) over the valid pixels of the whole
    batch -> {a1, a2, a3, abs_rel, sq_rel, rmse, rmse_log, silog, log_10} as Python floats (one host read).  Sums and
    metrics are float64 where the reference's are float32, and invalid pixels are left out where the reference lets them
    turn the result into NaN or inf (depth_sums states the rule)."""
    return dict(zip(DEPTH_KEYS, _batch_metrics(gt, pred, valid, min_depth, max_depth).tolist()))


def evaluate_depth_estimation(model, dataloader, debug=False):
    """Drop-in for the reference's evaluate_depth_estimation (src/evaluation/depth_estimation.py:85-126): every sample
    {"image", "depth"} goes through the model and its post_processing, out["depth"] is scored against ``depth`` with
    compute_errors_torch's metrics, and the mean over batches of the per-batch metrics is returned, which is what the
    reference's RunningAverageDict yields.  The metrics accumulate on the device; one host read at the end.  ``debug``
    windows are not reproduced."""
    model.eval()
    model.training = False
    dev = _dev.model_device(model)
    total, batches = None, 0
    with torch.no_grad():
        for sample in dataloader:
            img = sample["image"].to(dev)
            depth_gt = sample["depth"].to(dev)
            H, W = img.shape[2], img.shape[3]
            out = model.post_processing(model(img), H, W)
            m = _batch_metrics(depth_gt, out["depth"])
            total = m if total is None else total + m
            batches += 1
    if batches == 0:
        raise ValueError("evaluate_depth_estimation: the dataloader is empty")
    return dict(zip(DEPTH_KEYS, (total / batches).tolist()))
