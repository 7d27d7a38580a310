"""Fine-tuning the whole place-recognition head on the device: what the reference's ``train_visloc.py --freeze_backbone``
moves, on the HIP kernels of csrc/vpr_head_train.hip and csrc/vlad_train.hip (kp2d_cbr_forward_train, kp2d_cbr_backward,
kp2d_vlad_backward_input and the four calls of ``vlad_training``; include/kp2d.h).

* ``cbr_forward`` / ``cbr_backward`` / ``netvlad_backward_input`` — the three layer calls on device tensors.
* ``cbr_forward_batch`` / ``cbr_backward_batch`` / ``dropout2d_scale`` — the layer on the batch's own statistics, and the
  Dropout2d factors (kp2d_cbr_forward_batchnorm, kp2d_cbr_backward_batchnorm, kp2d_dropout2d_mask).
  The cbr calls, ``dropout2d_scale``, ``bn_vectors`` and ``adam_step`` live in ``train_ops`` and are imported here;
  ``netvlad_backward_input`` is this module's own.
* ``VPRHeadTrainer`` — forward, loss, backward and Adam for ``vlad_head.convlad{1,2,3}.conv.weight``, ``.bn.weight``,
  ``.bn.bias``, ``vlad_head.netvlad.conv.weight`` and ``vlad_head.netvlad.centroids`` of a KP2DTiny model; the step's own
  calls make no host synchronisation.

Conventions kept from the reference and from ``NetVLADTrainer``: ``TripletMarginLoss(margin ** 0.5, p=2, reduction="sum")``
divided by the number of negatives, rows ordered queries, positives, negatives in query order, ``torch.optim.Adam``'s
update, exact fp32 arithmetic.  Frozen: the backbone (the reference's own ``freeze_backbone()``) and every other head.
By default BatchNorm runs with its running statistics, which are not updated, and ``Dropout2d`` is off: ``vlad_head.eval()``
under autograd.  ``VPRHeadTrainer(model, bn="batch", dropout=0.2)`` is the reference's own mode, the head under
``model.train()``: batch statistics with their gradient terms, the running statistics' update, and ``Dropout2d`` behind
``convlad1`` (``cbr_forward_batch`` / ``cbr_backward_batch`` / ``dropout2d_scale``).  Stated deviations that remain: the
frozen backbone stays on the inference engine's running statistics (under the reference's ``model.train()`` its BatchNorm
layers use batch statistics too); the dropout stream is the library's counter-based hash, not torch's generator; and "a
frame with zero gradient changes no bit" holds in ``bn="running"`` mode only, since every frame enters the batch statistics.

There is no CPU path: CPU tensors raise, like the rest of the product.
"""
from __future__ import annotations

import torch

from . import _dev, _lib
from ._dev import ptr as _ptr, stream as _stream
from .train_ops import (LEAKY_SLOPE, MAX_CH, MIN_CH, AdamTrainer, _cbr_scratch, adam_step, bn_vectors, cbr_backward,  # noqa: F401
                        _views_loss, cbr_backward_batch, cbr_forward, cbr_forward_batch, cbr_layer_backward, cbr_layer_forward,
                        dropout2d_scale)
from .vlad_training import _check_layer, _scratch as _vlad_scratch, netvlad_backward, netvlad_forward, triplet_margin_loss


def netvlad_backward_input(enc, weight, centroids, saved, dvlad, scratch=None):
    """The gradient ``vlad_training.netvlad_backward`` does not form: with respect to the map ``enc`` the layer read
    (arguments as there) -> dx, shaped like ``enc``.  A frame whose ``dvlad`` row is zero gets exact zeros."""
    x, w, N, S, C, K = _check_layer(enc, weight, centroids)
    for name, t, shape in (("saved", saved, (N, K * C + 2 * K + 4)), ("dvlad", dvlad, (N, K * C))):
        _dev.require_device(f"netvlad_backward_input: {name}", t)
        if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != x.device:
            raise ValueError(f"{name} must be float32 {shape} on {x.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if C > MAX_CH:
        raise ValueError(f"netvlad_backward_input needs C <= {MAX_CH}, got {C}")
    cent = centroids.detach().contiguous()
    lib = _lib.load()
    scratch = _vlad_scratch(lib, N, S, C, K, x.device) if scratch is None else scratch
    dx = torch.empty_like(x)
    _lib.check(lib.kp2d_vlad_backward_input(_ptr(x), _ptr(w), _ptr(cent), _ptr(saved.contiguous()), _ptr(dvlad.contiguous()), N, S, C,
                                            K, _ptr(dx), _ptr(scratch), scratch.numel(), _stream(x.device)))
    return dx.view(enc.shape)


class VPRHeadTrainer(AdamTrainer):
    """Adam on the whole ``vlad_head`` of ``model`` under the reference's triplet loss.

        trainer = VPRHeadTrainer(model, lr=1e-4, margin=0.1)
        loss = trainer.step(query, positives, negatives, neg_counts)      # frames [., 3, H, W]; loss: a device scalar
        feat = model.backbone_features(frames)                            # the frozen backbone, once
        loss = trainer.step_features(feat, B, neg_counts)

    Trained, in the reference's registration order: ``convlad{1,2,3}.conv.weight``, ``.bn.weight``, ``.bn.bias``,
    ``netvlad.conv.weight``, ``netvlad.centroids``.  By default BatchNorm runs on its running statistics, which stay as they
    are, and there is no dropout (``vlad_head.eval()`` under autograd).  ``bn="batch"`` is the reference's ``model.train()``:
    every layer normalises with the batch's own statistics (each layer's ``bn.eps``), the gradients carry the terms through
    the mean and the variance, ``running_mean`` / ``running_var`` move with each layer's ``bn.momentum`` on the device,
    ``num_batches_tracked`` rises by one, and the buffers' version counters are bumped with the parameters'.  ``dropout=p``
    (the reference: 0.2) zeroes whole channels of ``convlad1``'s output with a fresh mask per step,
    ``dropout2d_scale(N, C, p, seed, step, 1, device)`` with ``step`` = ``self.steps`` of that step (1, 2, ...); it needs a
    model built ``with_drop`` and works in either ``bn`` mode (on running statistics the factor is a torch multiplication
    of the map and of its gradient).  ``step_features(..., drop=mask)`` takes the step's mask from the caller instead.
    The trainer's own calls make no host synchronisation and the loss stays on the device.  After a step every updated parameter's version counter is bumped, so the engine re-packs its
    weights on its next call, re-folding BatchNorm into the packed conv weights through its ordinary upload path;
    ``backbone_features`` is such a call, so a loop over ``step`` pays that upload once per step and a loop over
    ``step_features`` does not.  ``step_views`` / ``step_views_features`` are the multitask run's step on a batch of view
    pairs, under the batch-hard triplet loss (``vlad_training.hard_triplet_loss``); ``ht_stats`` holds its ``stats``.
    GeM / ConvAP poolers and ``remove_netvlad`` models raise ValueError."""

    _WHO = "VPRHeadTrainer"

    def __init__(self, model, lr=1e-4, margin=0.1, betas=(0.9, 0.999), eps=1e-8, bn="running", dropout=0.0, seed=0):
        if getattr(model, "global_descriptor_method", None) != "netvlad":
            raise ValueError(f"VPRHeadTrainer needs a NetVLAD pooler, the model has {getattr(model, 'global_descriptor_method', None)!r}")
        if getattr(model, "remove_netvlad", False) or not hasattr(model.vlad_head, "netvlad"):
            raise ValueError("VPRHeadTrainer: the model was built with remove_netvlad")
        self._init_adam(lr, betas, eps, margin)
        self.model = model
        self.slope = LEAKY_SLOPE if getattr(model, "leaky_relu", True) else 0.0
        if bn not in ("running", "batch"):
            raise ValueError(f"VPRHeadTrainer: bn must be 'running' or 'batch', got {bn!r}")
        if not (0.0 <= dropout < 1.0 and 0 <= int(seed) < 2 ** 64):
            raise ValueError(f"VPRHeadTrainer: dropout {dropout} outside [0, 1) or seed {seed} outside [0, 2^64)")
        if dropout > 0 and not getattr(model, "with_drop", False):
            raise ValueError("VPRHeadTrainer: dropout > 0 on a model built without with_drop, whose head has no dropout")
        if bn == "batch" and any(layer.bn.momentum is None for layer in self.layers):
            raise ValueError("VPRHeadTrainer: bn='batch' needs a numeric bn.momentum (None, the cumulative average, is not built)")
        self.bn, self.dropout, self.seed = bn, float(dropout), int(seed)
        self.n_active = None          # device int32 scalar of the last step
        self.ht_stats = None          # device int64 [4] of the last view step

    @property
    def layers(self):
        head = self.model.vlad_head
        return (head.convlad1, head.convlad2, head.convlad3)

    def parameters(self):
        """The eleven trained parameters in the reference's registration order."""
        out = []
        for layer in self.layers:
            out += [layer.conv.weight, layer.bn.weight, layer.bn.bias]
        netvlad = self.model.vlad_head.netvlad
        return out + [netvlad.conv.weight, netvlad.centroids]

    def step(self, query, positives, negatives, neg_counts):
        """Frames [B, 3, H, W], [B, 3, H, W], [n_neg, 3, H, W] and the negatives per query -> the loss before the update."""
        for name, t in (("query", query), ("positives", positives), ("negatives", negatives)):
            _dev.require_device(f"VPRHeadTrainer.step: {name}", t)
        if query.dim() != 4 or positives.shape != query.shape or negatives.dim() != 4 or negatives.shape[1:] != query.shape[1:]:
            raise ValueError("query and positives must be [B, 3, H, W], negatives [n_neg, 3, H, W]")
        with torch.no_grad():
            feat = self.model.backbone_features(torch.cat([query, positives, negatives]))
        return self.step_features(feat, query.shape[0], neg_counts)

    def forward_features(self, feat, scratch=None, drop=None):
        """The head's training forward on backbone maps -> [(x, y, c, (scale, shift, mean, invstd)) per layer]; the last
        ``y`` is the map NetVLAD reads (``only_encoder``'s map before its L2 normalisation).  On running statistics, whatever
        ``self.bn`` says (``_forward_batch`` is the batch-statistics forward, which moves the running statistics);
        ``drop``: the [N, C] factors behind ``convlad1``, None: no dropout."""
        acts, x = [], feat
        for i, layer in enumerate(self.layers):
            acts.append(cbr_layer_forward(layer, x, self.slope, scratch))
            x = acts[-1][1] if i > 0 or drop is None else acts[-1][1] * drop[:, :, None, None]
        return acts

    def _forward_batch(self, feat, scratch, drop):
        """-> [(x, y, c, (mean, invstd)) per layer] on batch statistics; the running statistics move."""
        acts, x = [], feat
        for i, layer in enumerate(self.layers):
            bn = layer.bn
            y, c, mean, invstd = cbr_forward_batch(x, layer.conv.weight, bn.weight, bn.bias, bn.eps, self.slope, drop if i == 0 else None,
                                                   (bn.running_mean, bn.running_var) if bn.track_running_stats else None, bn.momentum,
                                                   scratch)
            acts.append((x, y, c, (mean, invstd)))
            x = y
        return acts

    def step_features(self, feat, B, neg_counts, drop=None):
        """``feat`` = ``model.backbone_features`` of (queries, positives, negatives) -> the loss before the update.
        ``drop``: this step's [N, C] dropout factors from the caller, in place of the trainer's own draw."""
        params = self.parameters()
        _dev.require_device("VPRHeadTrainer.step_features: feat", feat)
        if feat.dim() != 4 or feat.dtype != torch.float32 or feat.shape[1] != self.layers[0].conv.weight.shape[1]:
            raise ValueError(f"feat must be float32 [N, {self.layers[0].conv.weight.shape[1]}, Hc, Wc], got {feat.dtype} {tuple(feat.shape)}")
        self._check_contiguous(params, "the head's")
        lib = _lib.load()
        N, _, H, W = feat.shape
        batch = self.bn == "batch"
        if batch and N * H * W < 2:
            raise ValueError(f"bn='batch' needs more than 1 value per channel, got feat {tuple(feat.shape)}")
        scratch = self._layer_scratch(lib, feat)
        if drop is None and self.dropout > 0:
            drop = dropout2d_scale(N, self.layers[0].conv.weight.shape[0], self.dropout, self.seed, self.steps + 1, 1, feat.device)
        if batch:
            acts = self._forward_batch(feat.contiguous(), scratch, drop)
        else:
            acts = self.forward_features(feat.contiguous(), scratch, drop)

        def loss_fn(vlad, vscratch):
            loss, dvlad, self.n_active = triplet_margin_loss(vlad, B, neg_counts, self.margin, vscratch)
            return loss, dvlad
        return self._finish_step(params, [(acts, drop)], loss_fn, scratch)

    def _layer_scratch(self, lib, feat):
        N, _, H, W = feat.shape
        cmax = max(max(l.conv.weight.shape[:2]) for l in self.layers)
        return _cbr_scratch(lib, N, H, W, cmax, cmax, feat.device)        # the largest layer's: every layer call fits

    def _finish_step(self, params, passes, loss_fn, scratch):
        """What follows the head's forward: NetVLAD on the maps of ``passes`` = [(acts, drop)], one entry per forward in row
        order, ``loss_fn(vlad, scratch) -> (loss, dvlad)``, the backward chain of every pass with the passes' parameter
        gradients added in order, one Adam step and the version bumps (``num_batches_tracked`` rises once per pass)."""
        netvlad = self.model.vlad_head.netvlad
        weight, cent = netvlad.conv.weight, netvlad.centroids
        lib = _lib.load()
        batch = self.bn == "batch"
        enc = passes[0][0][-1][1] if len(passes) == 1 else torch.cat([acts[-1][1] for acts, _ in passes])
        x, w, N, S, C, K = _check_layer(enc, weight, cent)
        vscratch = _vlad_scratch(lib, N, S, C, K, x.device)
        vlad, saved = netvlad_forward(x, w, cent, vscratch)
        loss, dvlad = loss_fn(vlad, vscratch)
        dW, dcent = netvlad_backward(x, w, cent, saved, dvlad, vscratch)
        dy_all = netvlad_backward_input(enc, w, cent, saved, dvlad, vscratch)
        total, row = None, 0
        for acts, drop in passes:
            n = acts[0][0].shape[0]
            dy = dy_all if len(passes) == 1 else dy_all[row:row + n].contiguous()
            row += n
            grads = [None] * 9
            for i in (2, 1, 0):
                layer = self.layers[i]
                if batch:
                    lx, ly, lc, (mean, invstd) = acts[i]
                    dw, dgamma, dbeta, dy = cbr_backward_batch(lx, layer.conv.weight, layer.bn.weight, mean, invstd, ly, lc, dy, self.slope,
                                                               drop if i == 0 else None, need_dx=i > 0, scratch=scratch)
                else:
                    if i == 0 and drop is not None:
                        dy = dy * drop[:, :, None, None]
                    dw, dgamma, dbeta, dy = cbr_layer_backward(layer, acts[i], dy, self.slope, need_dx=i > 0,
                                                               scratch=scratch)               # (the backbone is frozen: no dx of layer 1)
                grads[3 * i:3 * i + 3] = [dw, dgamma, dbeta]
            total = grads if total is None else [a + b for a, b in zip(total, grads)]
        self._apply(params, total + [dW, dcent])
        if batch:
            with torch.no_grad():     # the kernel wrote the running statistics through their addresses: bump those too
                for layer in self.layers:
                    if layer.bn.track_running_stats:
                        torch.autograd.graph.increment_version(layer.bn.running_mean)
                        torch.autograd.graph.increment_version(layer.bn.running_var)
                        layer.bn.num_batches_tracked.add_(len(passes))
        return loss

    def step_views(self, frames, frames_aug, margin=0.1, weight=1.0):
        """A batch of view pairs, frames and frames_aug [N, 3, H, W] (``augment.view_pair``) -> the loss before the update."""
        for name, t in (("frames", frames), ("frames_aug", frames_aug)):
            _dev.require_device(f"VPRHeadTrainer.step_views: {name}", t)
        if frames.dim() != 4 or frames_aug.shape != frames.shape:
            raise ValueError("frames and frames_aug must both be [N, 3, H, W]")
        with torch.no_grad():
            feat = self.model.backbone_features(torch.cat([frames, frames_aug]))
        N = frames.shape[0]
        return self.step_views_features(feat[:N], feat[N:], margin, weight)

    def step_views_features(self, feat, feat_aug, margin=0.1, weight=1.0, drop=None):
        """``feat``, ``feat_aug`` = ``model.backbone_features`` of the plain and of the augmented views -> the loss before the
        update: ``weight * hard_triplet_loss(cat(vlad, vlad_aug), view_labels(N), margin, hardest=True)``, the multitask run's
        ``vlad`` term.  ``bn="running"``: both views run through ``convlad1..3`` as one batch of 2 N.  ``bn="batch"``: each view
        is its own forward and backward through the three layers, as the reference's two ``keypoint_net(...)`` calls under
        ``model.train()``: its own batch statistics, the running statistics moved twice, plain view first,
        ``num_batches_tracked`` + 2, the two views' parameter gradients added, plain first; NetVLAD and the loss see all 2 N
        rows.  ``dropout=p``: one mask per view, ``dropout2d_scale(N, C, p, seed, step, 1, device)`` for the plain view and layer
        id 2 for the augmented one; ``drop=(mask, mask_aug)`` injects both.  ``ht_stats`` holds the loss call's ``stats``."""
        params = self.parameters()
        cin = self.layers[0].conv.weight.shape[1]
        for name, t in (("feat", feat), ("feat_aug", feat_aug)):
            _dev.require_device(f"VPRHeadTrainer.step_views_features: {name}", t)
            if t.dim() != 4 or t.dtype != torch.float32 or t.shape[1] != cin:
                raise ValueError(f"{name} must be float32 [N, {cin}, Hc, Wc], got {t.dtype} {tuple(t.shape)}")
        if feat_aug.shape != feat.shape:
            raise ValueError(f"feat and feat_aug must have one shape, got {tuple(feat.shape)} and {tuple(feat_aug.shape)}")
        self._check_contiguous(params, "the head's")
        N, _, H, W = feat.shape
        loss_fn = _views_loss(self, N, margin, weight)
        batch = self.bn == "batch"
        if batch and N * H * W < 2:
            raise ValueError(f"bn='batch' needs more than 1 value per channel, got feat {tuple(feat.shape)}")
        cout = self.layers[0].conv.weight.shape[0]
        if drop is not None:
            if len(drop) != 2 or any(tuple(d.shape) != (N, cout) for d in drop):
                raise ValueError(f"drop must be (mask, mask_aug), both [{N}, {cout}]")
        elif self.dropout > 0:
            drop = tuple(dropout2d_scale(N, cout, self.dropout, self.seed, self.steps + 1, layer, feat.device) for layer in (1, 2))
        lib = _lib.load()
        if batch:
            scratch = self._layer_scratch(lib, feat)
            passes = [(self._forward_batch(f.contiguous(), scratch, d), d)
                      for f, d in ((feat, None if drop is None else drop[0]), (feat_aug, None if drop is None else drop[1]))]
        else:
            both = torch.cat([feat, feat_aug])
            d = None if drop is None else torch.cat(list(drop))
            scratch = self._layer_scratch(lib, both)
            passes = [(self.forward_features(both, scratch, d), d)]
        return self._finish_step(params, passes, loss_fn, scratch)
