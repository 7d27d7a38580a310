"""Fine-tuning the segmentation head on the device: what the reference's ``train_multitask.py`` moves in its V2
``SegmentationHead`` (modules/decoders/segmentation.py:8-157) under ``_compute_segmentation_loss``
(KeypointNetwithIOLoss.py:880-884), on the HIP kernels of csrc/seg_train.hip and csrc/vpr_head_train.hip (include/kp2d.h).

* ``segmentation_loss`` — ``ce_weight * CrossEntropyLoss(ignore_index) + dice_weight * DiceLoss`` with its gradient.
* ``SegHeadTrainer`` — forward, loss, backward and Adam for the head's 26 tensors (``train="head"``) or for the last layer's
  two (``train="last"``, the reference's ``freeze_segmentation(except_last_layer=True)``).
* The layer calls live in ``train_ops`` and are imported here: ``conv_bias_forward`` / ``conv_bias_backward`` (the head's last
  layer, a 3x3 convolution with bias and any class count), ``maxpool2_forward`` / ``maxpool2_backward`` and
  ``shuffle_cat_forward`` / ``shuffle_cat_backward`` (the head's two scale changes), ``cbr_forward`` / ``cbr_backward`` (the
  Conv + BatchNorm + (Leaky)ReLU layers) and ``adam_step``.

Conventions kept from the reference: the loss weights 0.5 (CE) and 1.5 (Dice), ``ignore_index`` 255, ``torch.optim.Adam``'s
update, the parameters' registration order, exact fp32 arithmetic.  Frozen: the backbone and every other head.  Deviations:
the head runs as ``seg_head.eval()`` under autograd, BatchNorm on its running statistics, which do not move, and without the
head's two ``Dropout2d`` sites (the reference trains under ``model.train()``); a batch without a valid pixel gives loss 0 and
a zero gradient (torch: NaN); a label outside [0, C) that is not ``ignore_index`` is treated as ignored and counted
(torch raises).  CE is pinned to torch; Dice is restated from smp's definition (include/kp2d.h), smp was not available.

There is no CPU path: CPU tensors raise ValueError.
"""
from __future__ import annotations

import torch

from . import _dev, _lib, train_ops as _ops
from ._dev import ptr as _ptr, stream as _stream
from .train_ops import (LEAKY_SLOPE, MAX_CH, MIN_CH, AdamTrainer, adam_step, bn_vectors, cbr_backward, cbr_forward,  # noqa: F401
                        cbr_layer_backward, cbr_layer_forward, conv_bias_backward, conv_bias_forward, maxpool2_backward,
                        maxpool2_forward, shuffle_cat_backward, shuffle_cat_forward)

MAX_CLASSES = 128
_LABEL_DTYPES = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}      # KP2D_SEG_U8 / _I32 / _I64
SEG_NO_IGNORE = -2 ** 63                                              # KP2D_SEG_NO_IGNORE


def _check_label_tensor(where, labels, shape, device):
    if not isinstance(labels, torch.Tensor) or not _ops._is_device(labels):
        raise ValueError(f"{where}: labels must be a device tensor (there is no CPU path)")
    if labels.dtype not in _LABEL_DTYPES:
        raise ValueError(f"{where}: labels must be uint8, int32 or int64, got {labels.dtype}")
    if tuple(labels.shape) != tuple(shape):
        raise ValueError(f"{where}: labels must have the logits' size {tuple(shape)}, got {tuple(labels.shape)}")
    if labels.device != device:
        raise ValueError(f"{where}: labels and logits must live on one device")


def _check_labels(where, logits, labels):
    _ops._f32_maps(where, (("logits", logits),))
    N, C, H, W = logits.shape
    _check_label_tensor(where, labels, (N, H, W), logits.device)
    if not (1 <= N <= 65535 and 1 <= C <= MAX_CLASSES and H >= 1 and W >= 1):
        raise ValueError(f"{where}: needs 1 <= N <= 65535, 1 <= C <= {MAX_CLASSES}, got logits {tuple(logits.shape)}")
    return N, C, H, W


def segmentation_loss(logits, labels, ce_weight=0.5, dice_weight=1.5, ignore_index=255, scratch=None):
    """logits [N, C, H, W], labels [N, H, W] (uint8, int32 or int64) -> (loss, dlogits, valid, stray): the device scalar
    ``ce_weight * CE + dice_weight * Dice`` (formulas: include/kp2d.h), its gradient with respect to the logits, and the
    int64 device scalars of valid pixels and of stray ones (label outside [0, C) and not ``ignore_index``: treated as
    ignored).  ``ignore_index=None`` ignores nothing.  No valid pixel: loss 0, gradient 0."""
    N, C, H, W = _check_labels("segmentation_loss", logits, labels)
    ce_weight, dice_weight = float(ce_weight), float(dice_weight)
    if not (0.0 <= ce_weight < float("inf") and 0.0 <= dice_weight < float("inf")):
        raise ValueError(f"segmentation_loss: weights must be finite and >= 0, got {ce_weight}, {dice_weight}")
    ignore = SEG_NO_IGNORE if ignore_index is None else int(ignore_index)
    if not -2 ** 63 <= ignore < 2 ** 63:
        raise ValueError(f"segmentation_loss: ignore_index {ignore_index} is no int64")
    lib = _lib.load()
    dev = logits.device
    if scratch is None:
        scratch = _dev.scratch(int(lib.kp2d_seg_loss_scratch_bytes(N, H * W, C)), dev)
    z, lab = logits.contiguous(), labels.contiguous()
    loss = torch.empty((), dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    dz = torch.empty_like(z)
    _lib.check(lib.kp2d_seg_loss(_ptr(z), _ptr(lab), _LABEL_DTYPES[lab.dtype], N, H * W, C, ignore, ce_weight, dice_weight, _ptr(loss),
                                 _ptr(dz), _ptr(counts[0:1]), _ptr(counts[1:2]), _ptr(scratch), scratch.numel(), _stream(dev)))
    return loss, dz, counts[0], counts[1]


def _check_head(model, train, who="SegHeadTrainer", attr="seg_head", no_head=None, attention_walk=False):
    """The refusals of a dense head's trainer (``who``, on ``model.<attr>``), each with its reason -> the head's layers.
    ``attention_walk``: the trainer is one of ``attention_training``'s, which take the attention head and nothing else."""
    if train not in ("head", "last"):
        raise ValueError(f"{who}: train must be 'head' or 'last', got {train!r}")
    head = getattr(model, attr, None)
    if head is None or not hasattr(head, "convs"):
        raise ValueError(no_head(model) if no_head else f"{who}: the model has no {attr} (the depth head is not trained)")
    if getattr(model, "_version_id", 2) != 2 or hasattr(head, "featB"):
        raise ValueError(f"{who}: V3 heads are not supported: their last layer reads a channel slice of the trunk")
    if getattr(model, "upscale_method", "pixelshuffle") != "pixelshuffle" or hasattr(head, "upsample"):
        raise ValueError(f"{who}: upscale_method='convtranspose' (to_mcu) is not supported: only pixel shuffle has a backward")
    attention = bool(getattr(model, "use_attention", False))
    if attention_walk and not attention:
        raise ValueError(f"{who}: the model has no attention head (use_attention is off): its head is "
                         f"{'DepthHeadTrainer' if attr == 'depth_head' else 'SegHeadTrainer'}'s")
    if attention and train == "head" and not attention_walk:
        raise ValueError(f"{who}: train='head' on an attention head is not supported (no attention backward exists in this "
                         f"trainer: attention_training.Attention{who} has it); train='last' is")
    convs = list(head.convs)
    if len(convs) != (8 if attention else 9):
        raise ValueError(f"{who}: unexpected head of {len(convs)} layers")
    last = convs[-1]
    if last.bias is None:
        raise ValueError(f"{who}: the last layer has no bias")
    Cout, Cin = last.weight.shape[:2]
    if Cin % 16 or not (MIN_CH <= Cin <= MAX_CH and 1 <= Cout <= MAX_CH):
        raise ValueError(f"{who}: the last layer's channel counts ({Cin} -> {Cout}) are not supported by the conv kernels: "
                         f"needs Cin % 16 == 0, {MIN_CH} <= Cin <= {MAX_CH}, 1 <= Cout <= {MAX_CH}")
    if train == "head":
        for i, layer in enumerate(convs[:-1]):
            if attention and i in (1, 2):
                c = layer.att.fn.to_q.weight.shape[0]
                if c not in (48, 64):
                    raise ValueError(f"{who}: {attr}.convs.{i} is an attention module of {c} channels; the attention kernels take 48 or 64")
                continue
            co, ci = layer.conv.weight.shape[:2]
            if ci % 16 or co % 16 or not (MIN_CH <= ci <= MAX_CH and MIN_CH <= co <= MAX_CH):
                raise ValueError(f"{who}: {attr}.convs.{i} has channel counts {ci} -> {co}, which the conv kernels do not take "
                                 f"(C % 16 == 0, {MIN_CH} <= C <= {MAX_CH}); train='last' does not run this layer")
        k = 3 if attention else 4       # the layer before the first pixel shuffle
        c_in, c_hidden, d1 = convs[0].conv.weight.shape[1], convs[0].conv.weight.shape[0], convs[k].conv.weight.shape[0]
        if d1 % 4 or convs[k + 1].conv.weight.shape[1] != d1 // 4 + c_in or convs[k + 2].conv.weight.shape[0] % 4 \
                or convs[k + 3].conv.weight.shape[1] <= convs[k + 2].conv.weight.shape[0] // 4:
            raise ValueError(f"{who}: the head's channel counts (c_in {c_in}, c_hidden {c_hidden}, d1 {d1}) do not chain")
    return convs


class _DenseHeadTrainer(AdamTrainer):
    """The walk both dense heads' trainers share (``SegHeadTrainer`` here, ``depth_training.DepthHeadTrainer``): the V2
    SegmentationHead's nine layers forward and backward, the checks of the model and of the maps, and the update.  A
    trainer names its head (``_ATTR``), the prefix of its messages (``_WHO``) and what it calls the ground truth
    (``_TARGET``), and supplies ``_check_target`` and ``_loss``."""

    _WHO = _ATTR = None
    _ATTENTION = False      # attention_training's trainers: the V2 SegmentationHeadATT's walk

    def _init_walk(self, model, lr, train, betas, eps, no_head=None):
        self.convs = _check_head(model, train, self._WHO, self._ATTR, no_head, attention_walk=self._ATTENTION)
        self._init_adam(lr, betas, eps)
        self.model, self.train = model, train
        self.slope = LEAKY_SLOPE if getattr(model, "leaky_relu", True) else 0.0
        self.valid = self.stray = None      # int64 device scalars of the last step

    def _check_target(self, target, shape, device):
        """The ground truth against the logits' [N, Hs, Ws] -> what ``_loss`` takes; ValueError with the reason."""
        raise NotImplementedError

    def _loss(self, logits, target):
        """-> (loss, dlogits); sets ``valid`` and ``stray``."""
        raise NotImplementedError

    def parameters(self):
        """The trained parameters in the reference's registration order: 26 in "head" mode (47 on the attention head), 2 in
        "last" mode."""
        out = []
        if self.train == "head":
            for layer in self.convs[:-1]:
                out += _ops.attention_module_parameters(layer) if hasattr(layer, "att") else [layer.conv.weight, layer.bn.weight, layer.bn.bias]
        return out + [self.convs[-1].weight, self.convs[-1].bias]

    # ---- shapes ----------------------------------------------------------------------------------------------------------
    def _check_maps(self, x, skip):
        who, last = self._WHO, self.convs[-1]
        if self.train == "last":
            if skip is not None:
                raise ValueError(f"{who}: in train='last' mode pass the last layer's input and skip=None")
            _ops._f32_maps(who, (("x", x),))
            if x.shape[1] != last.weight.shape[1]:
                raise ValueError(f"{who}: the last layer reads [N, {last.weight.shape[1]}, Hs, Ws], got {tuple(x.shape)}")
            return
        if skip is None:
            raise ValueError(f"{who}: train='head' needs both backbone maps (model.backbone_maps)")
        _ops._f32_maps(who, (("x", x), ("skip", skip)))
        c_in = self.convs[0].conv.weight.shape[1]
        c_skip = self.convs[-2].conv.weight.shape[1] - self.convs[-3].conv.weight.shape[0] // 4
        N, _, H, W = x.shape
        if H % 2 or W % 2:
            raise ValueError(f"{who}: the backbone map must have even height and width, got {H} x {W} "
                             "(the pooled and shuffled map would not concatenate with it; the reference's own cat fails there)")
        if x.shape[1] != c_in or tuple(skip.shape) != (N, c_skip, 2 * H, 2 * W):
            raise ValueError(f"{who}: needs x [N, {c_in}, H, W] and skip [N, {c_skip}, 2 H, 2 W], got {tuple(x.shape)}, {tuple(skip.shape)}")
        if self._ATTENTION and (H < 4 or W < 4):
            raise ValueError(f"{who}: the backbone map must be at least 4 x 4, got {H} x {W} (the pooled map needs one 2 x 2 key patch)")

    def _scratch(self, x, skip):
        """One buffer for every cbr call of the walk: the largest layer at the largest map."""
        lib = _lib.load()
        N = x.shape[0]
        cmax = max(max(l.conv.weight.shape[:2]) for l in self.convs[:-1] if hasattr(l, "conv"))
        nbytes = int(lib.kp2d_cbr_train_scratch_bytes(N, skip.shape[2], skip.shape[3], cmax, cmax))
        if nbytes == 0:
            raise ValueError(f"{self._WHO}: maps {tuple(x.shape)}, {tuple(skip.shape)} are not supported")
        return _dev.scratch(nbytes, x.device)

    def _forward(self, x, skip):
        """-> (logits, saved activations)"""
        last = self.convs[-1]
        if self.train == "last":
            feat = x.contiguous()
            return conv_bias_forward(feat, last.weight, last.bias), {"feat": feat}
        x, skip = x.contiguous(), skip.contiguous()
        scratch = self._scratch(x, skip)
        a = {}

        def cbr(i, x):
            return cbr_layer_forward(self.convs[i], x, self.slope, scratch)

        if self._ATTENTION:
            return self._forward_attention(x, skip, scratch, cbr)
        a[0] = cbr(0, x)
        a[1] = cbr(1, a[0][1])
        pooled = maxpool2_forward(a[1][1])
        a[2] = cbr(2, pooled)
        a[3] = cbr(3, a[2][1])
        a[4] = cbr(4, a[3][1])
        a[5] = cbr(5, shuffle_cat_forward(a[4][1], x))
        a[6] = cbr(6, a[5][1])
        a[7] = cbr(7, shuffle_cat_forward(a[6][1], skip))
        feat = a[7][1]
        a["feat"], a["scratch"] = feat, scratch
        return conv_bias_forward(feat, last.weight, last.bias), a

    def _forward_attention(self, x, skip, scratch, cbr):
        """The V2 SegmentationHeadATT: convs[1] and convs[2] are attention modules, one before and one after the pooling."""
        last = self.convs[-1]
        a = {}
        a[0] = cbr(0, x)
        y1, a[1] = _ops.attention_module_forward(self.convs[1], a[0][1])
        y2, a[2] = _ops.attention_module_forward(self.convs[2], maxpool2_forward(y1))
        a["pool_in"] = y1
        a[3] = cbr(3, y2)
        a[4] = cbr(4, shuffle_cat_forward(a[3][1], x))
        a[5] = cbr(5, a[4][1])
        a[6] = cbr(6, shuffle_cat_forward(a[5][1], skip))
        feat = a[6][1]
        a["feat"], a["scratch"] = feat, scratch
        return conv_bias_forward(feat, last.weight, last.bias), a

    def _backward_attention(self, a, dy, grads, back):
        """``back(i, dy)`` undoes Conv + BatchNorm layer i into grads[slot(i)]; the modules' 15 gradients go to 3 ... 32."""
        dy = back(6, dy)
        dy = back(5, shuffle_cat_backward(dy, self.convs[5].conv.weight.shape[0] // 4))
        dy = back(4, dy)
        dy = back(3, shuffle_cat_backward(dy, self.convs[3].conv.weight.shape[0] // 4))      # (x is a frozen backbone map: no gradient)
        grads[18:33], dy = _ops.attention_module_backward(self.convs[2], a[2], dy)
        grads[3:18], dy = _ops.attention_module_backward(self.convs[1], a[1], maxpool2_backward(a["pool_in"], dy))
        back(0, dy, need_dx=False)                                                           # (the backbone is frozen: no dx)

    def forward_features(self, x, skip=None):
        """The head's training forward -> logits [N, classes, Hs, Ws].  "head" mode: the two backbone maps; "last" mode: the
        last layer's input alone."""
        self._check_maps(x, skip)
        return self._forward(x, skip)[0]

    def gradients(self, x, skip, target, loss_fn=None):
        """One forward, loss and backward without an update -> (loss, logits, the gradients in ``parameters()`` order).
        ``loss_fn(logits, target) -> (loss, dlogits)`` stands in for the trainer's own loss (the depth trainer's pair step)."""
        self._check_maps(x, skip)
        params = self.parameters()
        self._check_contiguous(params, "the head's")
        Hs, Ws = (x.shape[2], x.shape[3]) if self.train == "last" else (skip.shape[2], skip.shape[3])
        target = self._check_target(target, (x.shape[0], Hs, Ws), x.device)
        logits, a = self._forward(x, skip)
        loss, dz = (loss_fn or self._loss)(logits, target)
        last = self.convs[-1]
        head = self.train == "head"
        dw, db, dy = conv_bias_backward(a["feat"], last.weight, dz, need_dx=head)
        if not head:
            return loss, logits, [dw, db]
        grads = [None] * (45 if self._ATTENTION else 24) + [dw, db]
        scratch = a["scratch"]

        def back(i, dy, need_dx=True):
            g = cbr_layer_backward(self.convs[i], a[i], dy, self.slope, need_dx=need_dx, scratch=scratch)
            at = 3 * i if not self._ATTENTION or i == 0 else 3 * i + 24      # (two modules of 15 tensors stand where two layers of 3 did)
            grads[at:at + 3] = g[:3]
            return g[3]

        if self._ATTENTION:
            self._backward_attention(a, dy, grads, back)
            return loss, logits, grads

        dy = back(7, dy)
        dy = back(6, shuffle_cat_backward(dy, self.convs[6].conv.weight.shape[0] // 4))
        dy = back(5, dy)
        dy = back(4, shuffle_cat_backward(dy, self.convs[4].conv.weight.shape[0] // 4))      # (x is a frozen backbone map: no gradient)
        dy = back(3, dy)
        dy = back(2, dy)
        dy = back(1, maxpool2_backward(a[1][1], dy))
        back(0, dy, need_dx=False)                                                           # (the backbone is frozen: no dx)
        return loss, logits, grads

    def step_features(self, x, skip, target):
        """``model.backbone_maps`` of the frames ("last" mode: the last layer's input and None) and the ground truth -> the
        loss before the update, a device scalar."""
        loss, _, grads = self.gradients(x, skip, target)
        self._apply(self.parameters(), grads)
        return loss

    def step(self, frames, target):
        """Frames [N, 3, H, W] and the ground truth at the logits' size -> the loss before the update.  "head" mode runs the
        frozen backbone through ``model.backbone_maps`` (two only-encoder forwards); "last" mode one full forward with a tap
        on the last layer's input."""
        if not isinstance(frames, torch.Tensor) or not _ops._is_device(frames):
            raise ValueError(f"{self._WHO}.step: frames must be a device tensor (there is no CPU path)")
        with torch.no_grad():
            if self.train == "head":
                x, skip = self.model.backbone_maps(frames)
                return self.step_features(x, skip, target)
            n = len(self.convs)
            half = self.model.cell // 2
            shape = (self.convs[-1].weight.shape[1], frames.shape[2] // half, frames.shape[3] // half)
            _, feat = self.model.forward_with_tap(frames, f"{self._ATTR}.convs.{n - 2}", shape)
        return self.step_features(feat, None, target)


class SegHeadTrainer(_DenseHeadTrainer):
    """Adam on ``model.seg_head`` under the reference's segmentation loss, on a frozen backbone.

        trainer = SegHeadTrainer(model, lr=1e-4, train="head", ce_weight=0.5, dice_weight=1.5, ignore_index=255)
        loss = trainer.step(frames, labels)              # frames [N, 3, H, W]; labels [N, Hs, Ws] at the logits' size
        x, skip = model.backbone_maps(frames)            # the frozen backbone, once
        loss = trainer.step_features(x, skip, labels)    # a device scalar; no host synchronisation
        logits = trainer.forward_features(x, skip)       # the training forward alone

    ``train="head"``: all nine layers of the V2 non-attention head, 26 tensors in the reference's registration order
    (``convs.{0..7}.conv.weight``, ``.bn.weight``, ``.bn.bias``, ``convs.8.weight``, ``.bias``).  ``train="last"``: the last
    layer's weight and bias alone, the reference's ``freeze_segmentation(except_last_layer=True)``; ``step`` then takes that
    layer's input from the engine (a tap on the layer before it), so it also works on the V2 attention head, and
    ``step_features(feat, None, labels)`` / ``forward_features(feat)`` take that input [N, c_hidden, Hs, Ws] directly.
    BatchNorm runs on its running statistics, which stay as they are, and there is no dropout (``seg_head.eval()`` under
    autograd).  V3 heads, an attention head in "head" mode, ``to_mcu`` models, channel counts the conv kernels do not take
    (config N in "head" mode: its 72-channel concatenation) and odd backbone maps raise ValueError.  After a step every
    updated parameter's version counter is bumped, so the engine re-packs its weights on its next call.  The depth head of a
    ``depth=True`` model is ``depth_training.DepthHeadTrainer``'s; this trainer never touches it."""

    _WHO, _ATTR = "SegHeadTrainer", "seg_head"

    def __init__(self, model, lr=1e-4, train="head", ce_weight=0.5, dice_weight=1.5, ignore_index=255, betas=(0.9, 0.999), eps=1e-8):
        self._init_walk(model, lr, train, betas, eps)
        if not (0 <= ce_weight < float("inf") and 0 <= dice_weight < float("inf")):
            raise ValueError(f"SegHeadTrainer: ce_weight {ce_weight} and dice_weight {dice_weight} must be finite and >= 0")
        self.ce_weight, self.dice_weight, self.ignore_index = float(ce_weight), float(dice_weight), ignore_index

    def _check_target(self, labels, shape, device):
        _check_label_tensor("SegHeadTrainer", labels, shape, device)
        return labels

    def _loss(self, logits, labels):
        loss, dz, self.valid, self.stray = segmentation_loss(logits, labels, self.ce_weight, self.dice_weight, self.ignore_index)
        return loss, dz
