"""Fine-tuning the depth head on the device: what the reference's ``train_multitask.py`` moves in ``depth_head`` (the V2
``SegmentationHead`` with one class, modules/decoders/segmentation.py:8-157, followed by ``.sigmoid()``, kp2dtiny.py:588-590)
under ``_compute_depth_loss`` (KeypointNetwithIOLoss.py:907-916), on the HIP kernels of csrc/depth_train.hip, csrc/seg_train.hip
and csrc/vpr_head_train.hip (include/kp2d.h).

* ``depth_loss`` — ``silog_weight * SILogLoss + huber_weight * HuberLoss`` over the pixels with ``gt > 0``, taken from the
  logits before the sigmoid, with its gradient.
* ``DepthHeadTrainer`` — forward, loss, backward and Adam for the head's 26 tensors (``train="head"``) or for the last layer's
  two (``train="last"``); the walk over the nine layers is ``seg_training``'s, shared with ``SegHeadTrainer``; the layer calls
  and the Adam core under it live in ``train_ops``.

Conventions kept from the reference: SILog's constants 10 and 0.15 and torch's unbiased variance, Huber's delta 1 and mean
reduction, ``huber_loss_factor`` 1.0, the mask ``gt > 0``, ``torch.optim.Adam``'s update, the parameters' registration order,
exact fp32 arithmetic.  The outer ``depth_loss`` weight 0.5 is the caller's; ``step`` / ``step_features`` take one view, and
``step_pair`` / ``step_pair_features`` / ``pair_gradients`` take the plain and the augmented view with the reference's
cross-view term ``MSE(depth_aug, warp(depth, H)) * 0.5`` (KeypointNetwithIOLoss.py:587-603; the warp is ``augment``'s).
Frozen: the backbone and every other head.  Deviations: the head runs as
``depth_head.eval()`` under autograd (BatchNorm on its running statistics, no ``Dropout2d``); the loss is formed from the
logits, so it stays finite where torch's ``log(sigmoid(z))`` is ``-inf``; no valid pixel gives loss 0 and a zero gradient
(torch: NaN); one valid pixel gives Huber alone (torch: NaN); ``Dg = 0`` gives a zero SILog gradient (torch: NaN); a pixel
whose ground truth or logit is not finite is treated as invalid and counted in ``stray`` (torch: NaN for the whole batch).

There is no CPU path: CPU tensors raise ValueError.
"""
from __future__ import annotations

import torch

from . import _dev, _lib, train_ops as _ops
from ._dev import ptr as _ptr, stream as _stream
from .seg_training import _DenseHeadTrainer


def _check_gt(where, gt, shape, device):
    """The ground truth as a float32 device tensor of the logits' [N, Hs, Ws] (or [N, 1, Hs, Ws]) -> [N, Hs, Ws]."""
    if not isinstance(gt, torch.Tensor) or not _ops._is_device(gt):
        raise ValueError(f"{where}: depth_gt must be a device tensor (there is no CPU path)")
    if gt.dtype != torch.float32:
        raise ValueError(f"{where}: depth_gt must be float32, got {gt.dtype}")
    N, H, W = (int(v) for v in shape)
    if tuple(gt.shape) not in ((N, H, W), (N, 1, H, W)):
        raise ValueError(f"{where}: depth_gt must have the logits' size {(N, H, W)} (or {(N, 1, H, W)}), got {tuple(gt.shape)}")
    if gt.device != device:
        raise ValueError(f"{where}: depth_gt and logits must live on one device")
    return gt.reshape(N, H, W)


def depth_loss(logits, gt, silog_weight=1.0, huber_weight=1.0, scratch=None, return_parts=False):
    """logits [N, 1, H, W] or [N, H, W] BEFORE the sigmoid, gt of the same size (float32) -> (loss, dlogits, valid, stray): the
    device scalar ``silog_weight * SILog + huber_weight * Huber`` over the valid pixels (gt finite and > 0, logit finite;
    formulas: include/kp2d.h), its gradient with respect to the logits (shaped like them), and the int64 device scalars of
    valid pixels and of stray ones (gt or logit not finite: treated as invalid).  ``return_parts=True`` appends the float32
    device tensor [SILog, Huber], unweighted.  No valid pixel: loss 0, gradient 0."""
    where = "depth_loss"
    if not isinstance(logits, torch.Tensor) or not _ops._is_device(logits):
        raise ValueError(f"{where}: logits must be a device tensor (there is no CPU path)")
    if logits.dtype != torch.float32 or not (logits.dim() == 3 or (logits.dim() == 4 and logits.shape[1] == 1)):
        raise ValueError(f"{where}: logits must be float32 [N, 1, H, W] or [N, H, W], got {logits.dtype} {tuple(logits.shape)}")
    N, H, W = logits.shape[0], logits.shape[-2], logits.shape[-1]
    g = _check_gt(where, gt, (N, H, W), logits.device)
    if not (1 <= N <= 65535 and H >= 1 and W >= 1):
        raise ValueError(f"{where}: needs 1 <= N <= 65535 and H, W >= 1, got logits {tuple(logits.shape)}")
    silog_weight, huber_weight = float(silog_weight), float(huber_weight)
    if not (0.0 <= silog_weight < float("inf") and 0.0 <= huber_weight < float("inf")):
        raise ValueError(f"{where}: weights must be finite and >= 0, got {silog_weight}, {huber_weight}")
    lib = _lib.load()
    dev = logits.device
    if scratch is None:
        nbytes = int(lib.kp2d_depth_loss_scratch_bytes(N, H * W))
        if nbytes == 0:
            raise ValueError(f"{where}: logits {tuple(logits.shape)} are not supported (H * W above 2^30)")
        scratch = _dev.scratch(nbytes, dev)
    z, g = logits.contiguous(), g.contiguous()
    out = torch.empty(3, dtype=torch.float32, device=dev)        # loss, SILog, Huber
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    dz = torch.empty_like(z)
    _lib.check(lib.kp2d_depth_loss(_ptr(z), _ptr(g), N, H * W, silog_weight, huber_weight, _ptr(out[0:1]), _ptr(out[1:3]), _ptr(dz),
                                   _ptr(counts[0:1]), _ptr(counts[1:2]), _ptr(scratch), scratch.numel(), _stream(dev)))
    res = (out[0], dz, counts[0], counts[1])
    return res + (out[1:3],) if return_parts else res


def _no_depth_head(model):
    if getattr(model, "_version_id", 2) != 2:
        return ("DepthHeadTrainer: V3 models are not supported: their depth is featD on a channel slice of the segmentation "
                "trunk, there is no depth_head")
    return "DepthHeadTrainer: the model was built without depth=True: it has no depth_head"


class DepthHeadTrainer(_DenseHeadTrainer):
    """Adam on ``model.depth_head`` under the reference's depth loss, on a frozen backbone.

        trainer = DepthHeadTrainer(model, lr=1e-4, train="head", silog_weight=1.0, huber_weight=1.0)
        loss = trainer.step(frames, depth_gt)             # frames [N, 3, H, W]; depth_gt float32 [N, Hs, Ws] or [N, 1, Hs, Ws]
        x, skip = model.backbone_maps(frames)             # the frozen backbone, once
        loss = trainer.step_features(x, skip, depth_gt)   # a device scalar; no host synchronisation
        logits = trainer.forward_features(x, skip)        # before the sigmoid: torch.sigmoid(logits) is out["depth"]

    ``depth_gt`` is given at the logits' size; a pixel with ``gt <= 0`` carries no ground truth.  ``train="head"``: all nine
    layers of the V2 non-attention head, 26 tensors in the reference's registration order, the last layer through
    ``conv_bias_forward`` / ``conv_bias_backward`` with one output channel.  ``train="last"``: ``depth_head.convs.8.weight`` and
    ``.bias`` alone (on the attention head its last layer); ``step`` then takes that layer's input from the engine (a tap on
    the layer before it) and ``step_features(feat, None, depth_gt)`` takes it from the caller.  After a step ``valid``,
    ``stray`` (int64 device scalars) and ``parts`` (float32 [SILog, Huber], unweighted) describe it, and every updated
    parameter's version counter is bumped, so the engine re-packs its weights on its next call.  A model without
    ``depth=True``, V3 models, an attention head in "head" mode, ``to_mcu`` models, channel counts the conv kernels do not
    take, odd backbone maps, CPU tensors, non-contiguous parameters, and ground truth that is not float32 or not of the
    logits' size raise ValueError.  ``seg_head`` and ``depth_head`` read the same maps and share no parameter: a
    ``SegHeadTrainer`` step and a ``DepthHeadTrainer`` step on one batch are the reference's one optimizer step over the
    summed losses."""

    _WHO, _ATTR = "DepthHeadTrainer", "depth_head"

    def __init__(self, model, lr=1e-4, train="head", silog_weight=1.0, huber_weight=1.0, betas=(0.9, 0.999), eps=1e-8):
        self._init_walk(model, lr, train, betas, eps, no_head=_no_depth_head)
        if self.convs[-1].weight.shape[0] != 1:
            raise ValueError(f"DepthHeadTrainer: the last layer must have one output channel, got {self.convs[-1].weight.shape[0]}")
        if not (0 <= silog_weight < float("inf") and 0 <= huber_weight < float("inf")):
            raise ValueError(f"DepthHeadTrainer: silog_weight {silog_weight} and huber_weight {huber_weight} must be finite and >= 0")
        self.silog_weight, self.huber_weight = float(silog_weight), float(huber_weight)
        self.parts = None       # float32 device tensor [SILog, Huber] of the last step, unweighted
        self.pair_parts = self.inside = None      # of the last pair step: [SILog, Huber, SILog_aug, Huber_aug, cross]; inside pixels

    def _check_target(self, gt, shape, device):
        return _check_gt("DepthHeadTrainer", gt, shape, device)

    def _loss(self, logits, gt):
        loss, dz, self.valid, self.stray, self.parts = depth_loss(logits, gt, self.silog_weight, self.huber_weight, return_parts=True)
        return loss, dz

    # ---- the pair step: both views and the cross-view term ------------------------------------------------------------------
    def pair_gradients(self, maps, maps_aug, gt, gt_aug, homography, cross_weight=0.5, inside_only=False):
        """The reference's depth loss over a view pair (KeypointNetwithIOLoss.py:587-603), without an update:

            L(z, gt) + L(z_aug, gt_aug) + cross_weight · MSE(sigmoid(z_aug), warp(sigmoid(z), homography))

        ``maps`` = (x, skip) of the plain view and ``maps_aug`` of the augmented one ("last" mode: (feat, None)), each of N
        frames; both go through the head as one batch of 2 N.  ``gt``, ``gt_aug`` at the logits' size; ``homography``
        [N, 3, 3] float32 or float64 in normalised coordinates, as ``augment.view_pair`` returns it.  L is ``depth_loss``,
        once per view (each view has its own SILog statistics); the cross term is ``augment.cross_view_mse`` on the two
        sigmoids (nearest warp, outside pixels 0; ``inside_only`` as there), its gradients chained through p (1 - p) and
        added to the logits' -> (loss, logits [2 N, 1, Hs, Ws], the gradients in ``parameters()`` order).  Afterwards
        ``pair_parts`` is float32 [SILog, Huber, SILog_aug, Huber_aug, cross] (unweighted; cross is the MSE), ``inside`` the
        int64 count of inside pixels, ``valid`` and ``stray`` the two views' sums, ``parts`` the plain view's."""
        from .augment import cross_view_mse
        who = "DepthHeadTrainer.pair_gradients"
        (x, skip), (xa, skipa) = maps, maps_aug
        for a, b in ((x, xa), (skip, skipa)):
            if (a is None) != (b is None) or (a is not None and (not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor) or
                                                                 a.shape != b.shape or a.device != b.device)):
                raise ValueError(f"{who}: the two views' maps must have one shape and one device")
        cross_weight = float(cross_weight)
        if not (0.0 <= cross_weight < float("inf")):
            raise ValueError(f"{who}: cross_weight must be finite and >= 0, got {cross_weight}")
        N = x.shape[0]
        for name, g in (("gt", gt), ("gt_aug", gt_aug)):
            if not isinstance(g, torch.Tensor) or not _ops._is_device(g) or g.dim() not in (3, 4) or g.shape[0] != N:
                raise ValueError(f"{who}: {name} must be a device tensor [N, Hs, Ws] or [N, 1, Hs, Ws] of the {N} frames")
        if gt.shape != gt_aug.shape:
            raise ValueError(f"{who}: gt {tuple(gt.shape)} and gt_aug {tuple(gt_aug.shape)} must have one shape")

        def pair_loss(logits, target):
            z, za = logits[:N], logits[N:]
            l0, dz0, v0, s0, p0 = depth_loss(z, target[:N], self.silog_weight, self.huber_weight, return_parts=True)
            l1, dz1, v1, s1, p1 = depth_loss(za, target[N:], self.silog_weight, self.huber_weight, return_parts=True)
            p, pa = torch.sigmoid(z), torch.sigmoid(za)
            mse, dp, dpa, self.inside = cross_view_mse(p, pa, homography, weight=1.0, inside_only=inside_only)
            dz = torch.cat([dz0 + cross_weight * dp * (p * (1.0 - p)), dz1 + cross_weight * dpa * (pa * (1.0 - pa))])
            self.valid, self.stray, self.parts = v0 + v1, s0 + s1, p0
            self.pair_parts = torch.cat([p0, p1, mse.reshape(1)])
            return (l0 + l1) + cross_weight * mse, dz

        both = lambda a, b: None if a is None else torch.cat([a, b])
        return self.gradients(both(x, xa), both(skip, skipa), torch.cat([gt, gt_aug]), loss_fn=pair_loss)

    def step_pair_features(self, maps, maps_aug, gt, gt_aug, homography, cross_weight=0.5, inside_only=False):
        """``pair_gradients`` and one Adam update (one step, one version bump per parameter) -> the loss before the update."""
        loss, _, grads = self.pair_gradients(maps, maps_aug, gt, gt_aug, homography, cross_weight, inside_only)
        self._apply(self.parameters(), grads)
        return loss

    def step_pair(self, frames, frames_aug, gt, gt_aug, homography, cross_weight=0.5, inside_only=False):
        """Both views' frames [N, 3, H, W] (``augment.view_pair``'s image and image_aug) -> the loss before the update.  The
        frozen backbone runs on the two views as one batch, as ``step`` runs it on one."""
        for name, f in (("frames", frames), ("frames_aug", frames_aug)):
            if not isinstance(f, torch.Tensor) or not _ops._is_device(f):
                raise ValueError(f"DepthHeadTrainer.step_pair: {name} must be a device tensor (there is no CPU path)")
        if frames.shape != frames_aug.shape:
            raise ValueError(f"DepthHeadTrainer.step_pair: frames {tuple(frames.shape)} and frames_aug {tuple(frames_aug.shape)} differ")
        N = frames.shape[0]
        both = torch.cat([frames, frames_aug])
        with torch.no_grad():
            if self.train == "head":
                x, skip = self.model.backbone_maps(both)
                return self.step_pair_features((x[:N], skip[:N]), (x[N:], skip[N:]), gt, gt_aug, homography, cross_weight, inside_only)
            half = self.model.cell // 2
            shape = (self.convs[-1].weight.shape[1], both.shape[2] // half, both.shape[3] // half)
            _, feat = self.model.forward_with_tap(both, f"{self._ATTR}.convs.{len(self.convs) - 2}", shape)
        return self.step_pair_features((feat[:N], None), (feat[N:], None), gt, gt_aug, homography, cross_weight, inside_only)
