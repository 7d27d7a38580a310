"""Fine-tuning the segmentation head on the device: what the reference's ``train_multitask.py`` moves in its V2
``SegmentationHead`` (modules/decoders/segmentation.py:8-157) under ``_compute_segmentation_loss``
(KeypointNetwithIOLoss.py:880-884), on the HIP kernels of csrc/seg_train.hip and csrc/vpr_head_train.hip (include/kp2d.h).

* ``conv_bias_forward`` / ``conv_bias_backward`` — the head's last layer, a 3x3 convolution with bias and any class count.
* ``segmentation_loss`` — ``ce_weight * CrossEntropyLoss(ignore_index) + dice_weight * DiceLoss`` with its gradient.
* ``maxpool2_forward`` / ``maxpool2_backward``, ``shuffle_cat_forward`` / ``shuffle_cat_backward`` — the head's two scale changes.
* ``SegHeadTrainer`` — forward, loss, backward and Adam for the head's 26 tensors (``train="head"``) or for the last layer's
  two (``train="last"``, the reference's ``freeze_segmentation(except_last_layer=True)``); the Conv + BatchNorm + (Leaky)ReLU
  layers and Adam are ``vpr_head_training``'s ``cbr_forward`` / ``cbr_backward`` and ``adam_step``, as they are.

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

from . import _dev, _lib
from ._dev import ptr as _ptr, stream as _stream
from .vlad_training import adam_step
from .vpr_head_training import LEAKY_SLOPE, MAX_CH, MIN_CH, bn_vectors, cbr_backward, cbr_forward

MAX_CLASSES = 128
_LABEL_DTYPES = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}      # KP2D_SEG_U8 / _I32 / _I64
SEG_NO_IGNORE = -2 ** 63                                              # KP2D_SEG_NO_IGNORE


def _is_device(t):
    """There is no CPU path behind the kernels."""
    return t.device.type == "cuda"


def _f32_maps(where, named, dims=4):
    """Every (name, tensor) is a float32 device tensor of ``dims`` dimensions on one device, else ValueError."""
    for name, t in named:
        if not isinstance(t, torch.Tensor) or not _is_device(t):
            raise ValueError(f"{where}: {name} must be a device tensor (there is no CPU path)")
        if t.dtype != torch.float32 or t.dim() != dims:
            raise ValueError(f"{where}: {name} must be float32 with {dims} dimensions, got {t.dtype} {tuple(t.shape)}")
    if any(t.device != named[0][1].device for _, t in named):
        raise ValueError(f"{where}: every tensor of a call must live on one device")


def _check_conv_bias(where, x, weight, bias, maps=()):
    """-> (N, H, W, Cin, Cout), everything checked before any library call; ``maps``: (name, tensor) of [N, Cout, H, W]."""
    _f32_maps(where, (("x", x), ("weight", weight)) + tuple(maps))
    N, Cin, H, W = x.shape
    if weight.shape[1:] != (Cin, 3, 3):
        raise ValueError(f"{where}: weight must be [Cout, {Cin}, 3, 3], got {tuple(weight.shape)}")
    Cout = weight.shape[0]
    if N < 1 or N > 65535 or H < 1 or W < 1:
        raise ValueError(f"{where}: x must be [1 <= N <= 65535, Cin, H >= 1, W >= 1], got {tuple(x.shape)}")
    if Cin % 16 or not (MIN_CH <= Cin <= MAX_CH and 1 <= Cout <= MAX_CH):
        raise ValueError(f"{where}: needs Cin % 16 == 0, {MIN_CH} <= Cin <= {MAX_CH} and 1 <= Cout <= {MAX_CH} (got Cin {Cin}, Cout {Cout})")
    if bias is not None:
        _f32_maps(where, (("bias", bias),), dims=1)
        if tuple(bias.shape) != (Cout,) or bias.device != x.device:
            raise ValueError(f"{where}: bias must be float32 [{Cout}] on {x.device}, got {tuple(bias.shape)} on {bias.device}")
    for name, t in maps:
        if tuple(t.shape) != (N, Cout, H, W):
            raise ValueError(f"{where}: {name} must be {(N, Cout, H, W)}, got {tuple(t.shape)}")
    return N, H, W, Cin, Cout


def _bias_scratch(lib, N, H, W, Cin, Cout, dev):
    nbytes = int(lib.kp2d_conv_bias_scratch_bytes(N, H, W, Cin, Cout))
    if nbytes == 0:
        raise ValueError(f"the last layer does not support N {N}, H {H}, W {W}, Cin {Cin}, Cout {Cout}")
    return _dev.scratch(nbytes, dev)


def conv_bias_forward(x, weight, bias, scratch=None):
    """x [N, Cin, H, W], weight [Cout, Cin, 3, 3], bias [Cout] -> conv3x3(x, weight) (stride 1, padding 1) + bias,
    [N, Cout, H, W]; Cin % 16 == 0, 16 <= Cin <= 128, any 1 <= Cout <= 128."""
    if bias is None:
        raise ValueError("conv_bias_forward: bias must be a float32 [Cout] device tensor")
    N, H, W, Cin, Cout = _check_conv_bias("conv_bias_forward", x, weight, bias)
    lib = _lib.load()
    scratch = _bias_scratch(lib, N, H, W, Cin, Cout, x.device) if scratch is None else scratch
    y = torch.empty(N, Cout, H, W, dtype=torch.float32, device=x.device)
    _lib.check(lib.kp2d_conv_bias_forward_train(_ptr(x.contiguous()), _ptr(weight.detach().contiguous()), _ptr(bias.detach().contiguous()),
                                                N, H, W, Cin, Cout, _ptr(y), _ptr(scratch), scratch.numel(), _stream(x.device)))
    return y


def conv_bias_backward(x, weight, dy, need_dx=True, scratch=None):
    """The gradients of a scalar given its gradient ``dy`` [N, Cout, H, W] with respect to ``conv_bias_forward``'s result ->
    (dweight [Cout, Cin, 3, 3], dbias [Cout], dx [N, Cin, H, W] or None).  Bit-reproducible; dweight and dbias have the same
    bits with and without dx."""
    N, H, W, Cin, Cout = _check_conv_bias("conv_bias_backward", x, weight, None, (("dy", dy),))
    lib = _lib.load()
    scratch = _bias_scratch(lib, N, H, W, Cin, Cout, x.device) if scratch is None else scratch
    dw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=x.device)
    db = torch.empty(Cout, dtype=torch.float32, device=x.device)
    dx = torch.empty(N, Cin, H, W, dtype=torch.float32, device=x.device) if need_dx else None
    _lib.check(lib.kp2d_conv_bias_backward(_ptr(x.contiguous()), _ptr(weight.detach().contiguous()), _ptr(dy.contiguous()), N, H, W, Cin,
                                           Cout, _ptr(dw), _ptr(db), _ptr(dx), _ptr(scratch), scratch.numel(), _stream(x.device)))
    return dw, db, dx


def _check_label_tensor(where, labels, shape, device):
    if not isinstance(labels, torch.Tensor) or not _is_device(labels):
        raise ValueError(f"{where}: labels must be a device tensor (there is no CPU path)")
    if labels.dtype not in _LABEL_DTYPES:
        raise ValueError(f"{where}: labels must be uint8, int32 or int64, got {labels.dtype}")
    if tuple(labels.shape) != tuple(shape):
        raise ValueError(f"{where}: labels must have the logits' size {tuple(shape)}, got {tuple(labels.shape)}")
    if labels.device != device:
        raise ValueError(f"{where}: labels and logits must live on one device")


def _check_labels(where, logits, labels):
    _f32_maps(where, (("logits", logits),))
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


def maxpool2_forward(x):
    """x [N, C, H, W] -> 2 x 2 stride-2 max pooling, [N, C, H // 2, W // 2]: torch's ``max_pool2d(x, 2, 2)`` bit for bit."""
    _f32_maps("maxpool2_forward", (("x", x),))
    N, C, H, W = x.shape
    if N < 1 or C < 1 or H < 2 or W < 2:
        raise ValueError(f"maxpool2_forward: needs N, C >= 1 and H, W >= 2, got {tuple(x.shape)}")
    y = torch.empty(N, C, H // 2, W // 2, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().kp2d_maxpool2_forward_train(_ptr(x.contiguous()), N, C, H, W, _ptr(y), _stream(x.device)))
    return y


def maxpool2_backward(x, dy):
    """The forward's input and the gradient of its result -> dx like ``x``: the gradient goes to each window's maximum,
    found again from ``x``; of equal maxima the first in row-major order takes it (torch's rule)."""
    _f32_maps("maxpool2_backward", (("x", x), ("dy", dy)))
    N, C, H, W = x.shape
    if N < 1 or C < 1 or H < 2 or W < 2 or tuple(dy.shape) != (N, C, H // 2, W // 2):
        raise ValueError(f"maxpool2_backward: needs x [N, C, H >= 2, W >= 2] and dy [N, C, H // 2, W // 2], got {tuple(x.shape)}, {tuple(dy.shape)}")
    dx = torch.empty(N, C, H, W, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().kp2d_maxpool2_backward(_ptr(x.contiguous()), _ptr(dy.contiguous()), N, C, H, W, _ptr(dx), _stream(x.device)))
    return dx


def shuffle_cat_forward(a, b):
    """a [N, 4 C, h, w], b [N, Cb, 2 h, 2 w] -> ``cat([pixel_shuffle(a, 2), b], dim=1)``, [N, C + Cb, 2 h, 2 w]."""
    _f32_maps("shuffle_cat_forward", (("a", a), ("b", b)))
    N, C4, h, w = a.shape
    if N < 1 or C4 < 4 or C4 % 4 or h < 1 or w < 1:
        raise ValueError(f"shuffle_cat_forward: a must be [N >= 1, 4 C, h >= 1, w >= 1], got {tuple(a.shape)}")
    if b.shape[0] != N or b.shape[1] < 1 or tuple(b.shape[2:]) != (2 * h, 2 * w):
        raise ValueError(f"shuffle_cat_forward: b must be [{N}, Cb >= 1, {2 * h}, {2 * w}], got {tuple(b.shape)} (odd maps do not concatenate)")
    C, Cb = C4 // 4, b.shape[1]
    out = torch.empty(N, C + Cb, 2 * h, 2 * w, dtype=torch.float32, device=a.device)
    _lib.check(_lib.load().kp2d_shuffle_cat_forward(_ptr(a.contiguous()), _ptr(b.contiguous()), N, C, Cb, h, w, _ptr(out), _stream(a.device)))
    return out


def shuffle_cat_backward(dout, C):
    """dout [N, C + Cb, 2 h, 2 w] -> the gradient of the shuffled operand, [N, 4 C, h, w]; the other operand's is not formed."""
    _f32_maps("shuffle_cat_backward", (("dout", dout),))
    N, Ct, H, W = dout.shape
    C = int(C)
    if N < 1 or not 1 <= C <= Ct or H % 2 or W % 2 or H < 2 or W < 2:
        raise ValueError(f"shuffle_cat_backward: needs dout [N, C + Cb, 2 h, 2 w] with 1 <= C <= C + Cb, got {tuple(dout.shape)}, C {C}")
    da = torch.empty(N, 4 * C, H // 2, W // 2, dtype=torch.float32, device=dout.device)
    _lib.check(_lib.load().kp2d_shuffle_cat_backward(_ptr(dout.contiguous()), N, C, Ct - C, H // 2, W // 2, _ptr(da), _stream(dout.device)))
    return da


def _check_head(model, train, who="SegHeadTrainer", attr="seg_head", no_head=None):
    """The refusals of a dense head's trainer (``who``, on ``model.<attr>``), each with its reason -> the head's layers."""
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
    if attention and train == "head":
        raise ValueError(f"{who}: train='head' on an attention head is not supported (no attention backward exists); "
                         "train='last' is")
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
            co, ci = layer.conv.weight.shape[:2]
            if ci % 16 or co % 16 or not (MIN_CH <= ci <= MAX_CH and MIN_CH <= co <= MAX_CH):
                raise ValueError(f"{who}: {attr}.convs.{i} has channel counts {ci} -> {co}, which the conv kernels do not take "
                                 f"(C % 16 == 0, {MIN_CH} <= C <= {MAX_CH}); train='last' does not run this layer")
        c_in, c_hidden, d1 = convs[0].conv.weight.shape[1], convs[0].conv.weight.shape[0], convs[4].conv.weight.shape[0]
        if d1 % 4 or convs[5].conv.weight.shape[1] != d1 // 4 + c_in or convs[6].conv.weight.shape[0] % 4 \
                or convs[7].conv.weight.shape[1] <= convs[6].conv.weight.shape[0] // 4:
            raise ValueError(f"{who}: the head's channel counts (c_in {c_in}, c_hidden {c_hidden}, d1 {d1}) do not chain")
    return convs


class _DenseHeadTrainer:
    """The walk both dense heads' trainers share (``SegHeadTrainer`` here, ``depth_training.DepthHeadTrainer``): the V2
    SegmentationHead's nine layers forward and backward, the checks of the model and of the maps, and the Adam loop.  A
    trainer names its head (``_ATTR``), the prefix of its messages (``_WHO``) and what it calls the ground truth
    (``_TARGET``), and supplies ``_check_target`` and ``_loss``."""

    _WHO = _ATTR = None

    def _init_walk(self, model, lr, train, betas, eps, no_head=None):
        self.convs = _check_head(model, train, self._WHO, self._ATTR, no_head)
        if not (lr >= 0 and 0 <= betas[0] < 1 and 0 <= betas[1] < 1 and eps >= 0):
            raise ValueError(f"{self._WHO}: lr {lr}, betas {betas}, eps {eps}")
        self.model, self.train, self.lr, self.betas, self.eps = model, train, float(lr), tuple(betas), float(eps)
        self.slope = LEAKY_SLOPE if getattr(model, "leaky_relu", True) else 0.0
        self.steps = 0
        self.valid = self.stray = None      # int64 device scalars of the last step
        self._state = {}

    def _check_target(self, target, shape, device):
        """The ground truth against the logits' [N, Hs, Ws] -> what ``_loss`` takes; ValueError with the reason."""
        raise NotImplementedError

    def _loss(self, logits, target):
        """-> (loss, dlogits); sets ``valid`` and ``stray``."""
        raise NotImplementedError

    def parameters(self):
        """The trained parameters in the reference's registration order: 26 in "head" mode, 2 in "last" mode."""
        out = []
        if self.train == "head":
            for layer in self.convs[:-1]:
                out += [layer.conv.weight, layer.bn.weight, layer.bn.bias]
        return out + [self.convs[-1].weight, self.convs[-1].bias]

    def _moments(self, p):
        st = self._state.get(id(p))
        if st is None or st[0].device != p.device or st[0].shape != p.shape:
            st = (torch.zeros_like(p.data), torch.zeros_like(p.data))
            self._state[id(p)] = st
        return st

    # ---- shapes ----------------------------------------------------------------------------------------------------------
    def _check_maps(self, x, skip):
        who, last = self._WHO, self.convs[-1]
        if self.train == "last":
            if skip is not None:
                raise ValueError(f"{who}: in train='last' mode pass the last layer's input and skip=None")
            _f32_maps(who, (("x", x),))
            if x.shape[1] != last.weight.shape[1]:
                raise ValueError(f"{who}: the last layer reads [N, {last.weight.shape[1]}, Hs, Ws], got {tuple(x.shape)}")
            return
        if skip is None:
            raise ValueError(f"{who}: train='head' needs both backbone maps (model.backbone_maps)")
        _f32_maps(who, (("x", x), ("skip", skip)))
        c_in = self.convs[0].conv.weight.shape[1]
        c_skip = self.convs[7].conv.weight.shape[1] - self.convs[6].conv.weight.shape[0] // 4
        N, _, H, W = x.shape
        if H % 2 or W % 2:
            raise ValueError(f"{who}: the backbone map must have even height and width, got {H} x {W} "
                             "(the pooled and shuffled map would not concatenate with it; the reference's own cat fails there)")
        if x.shape[1] != c_in or tuple(skip.shape) != (N, c_skip, 2 * H, 2 * W):
            raise ValueError(f"{who}: needs x [N, {c_in}, H, W] and skip [N, {c_skip}, 2 H, 2 W], got {tuple(x.shape)}, {tuple(skip.shape)}")

    def _cbr(self, i, x, scratch):
        layer = self.convs[i]
        vec = bn_vectors(layer.bn)
        y, c = cbr_forward(x, layer.conv.weight, vec[0], vec[1], self.slope, scratch)
        return (x, y, c, vec)

    def _scratch(self, x, skip):
        """One buffer for every cbr call of the walk: the largest layer at the largest map."""
        lib = _lib.load()
        N = x.shape[0]
        cmax = max(max(l.conv.weight.shape[:2]) for l in self.convs[:-1])
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
        a[0] = self._cbr(0, x, scratch)
        a[1] = self._cbr(1, a[0][1], scratch)
        pooled = maxpool2_forward(a[1][1])
        a[2] = self._cbr(2, pooled, scratch)
        a[3] = self._cbr(3, a[2][1], scratch)
        a[4] = self._cbr(4, a[3][1], scratch)
        a[5] = self._cbr(5, shuffle_cat_forward(a[4][1], x), scratch)
        a[6] = self._cbr(6, a[5][1], scratch)
        a[7] = self._cbr(7, shuffle_cat_forward(a[6][1], skip), scratch)
        feat = a[7][1]
        a["feat"], a["scratch"] = feat, scratch
        return conv_bias_forward(feat, last.weight, last.bias), a

    def forward_features(self, x, skip=None):
        """The head's training forward -> logits [N, classes, Hs, Ws].  "head" mode: the two backbone maps; "last" mode: the
        last layer's input alone."""
        self._check_maps(x, skip)
        return self._forward(x, skip)[0]

    def gradients(self, x, skip, target):
        """One forward, loss and backward without an update -> (loss, logits, the gradients in ``parameters()`` order)."""
        self._check_maps(x, skip)
        params = self.parameters()
        if not all(p.is_contiguous() for p in params):
            raise ValueError(f"{self._WHO}: the head's parameters must be contiguous")
        Hs, Ws = (x.shape[2], x.shape[3]) if self.train == "last" else (skip.shape[2], skip.shape[3])
        target = self._check_target(target, (x.shape[0], Hs, Ws), x.device)
        logits, a = self._forward(x, skip)
        loss, dz = self._loss(logits, target)
        last = self.convs[-1]
        head = self.train == "head"
        dw, db, dy = conv_bias_backward(a["feat"], last.weight, dz, need_dx=head)
        if not head:
            return loss, logits, [dw, db]
        grads = [None] * 24 + [dw, db]
        scratch = a["scratch"]

        def back(i, dy, need_dx=True):
            lx, ly, lc, (scale, _, mean, invstd) = a[i]
            g = cbr_backward(lx, self.convs[i].conv.weight, scale, mean, invstd, ly, lc, dy, self.slope, need_dx=need_dx, scratch=scratch)
            grads[3 * i:3 * i + 3] = g[:3]
            return g[3]

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
        self.steps += 1
        for p, g in zip(self.parameters(), grads):
            m, v = self._moments(p)
            adam_step(p.data, g.view(p.shape), m, v, self.steps, self.lr, self.betas, self.eps)
            with torch.no_grad():     # ``p.data`` counts versions on its own: bump the parameter's, which the engine watches
                torch.autograd.graph.increment_version(p)
        return loss

    def step(self, frames, target):
        """Frames [N, 3, H, W] and the ground truth at the logits' size -> the loss before the update.  "head" mode runs the
        frozen backbone through ``model.backbone_maps`` (two only-encoder forwards); "last" mode one full forward with a tap
        on the last layer's input."""
        if not isinstance(frames, torch.Tensor) or not _is_device(frames):
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
