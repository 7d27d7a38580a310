"""Fine-tuning the whole place-recognition head on the device: what the reference's ``train_visloc.py --freeze_backbone``
moves, on the HIP kernels of csrc/vpr_head_train.hip and csrc/vlad_train.hip (kp2d_cbr_forward_train, kp2d_cbr_backward,
kp2d_vlad_backward_input and the four calls of ``vlad_training``; include/kp2d.h).

* ``cbr_forward`` / ``cbr_backward`` / ``netvlad_backward_input`` — the three layer calls on device tensors.
* ``cbr_forward_batch`` / ``cbr_backward_batch`` / ``dropout2d_scale`` — the layer on the batch's own statistics, and the
  Dropout2d factors (kp2d_cbr_forward_batchnorm, kp2d_cbr_backward_batchnorm, kp2d_dropout2d_mask).
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
from .vlad_training import (_check_layer, _scratch as _vlad_scratch, adam_step, netvlad_backward, netvlad_forward,
                            triplet_margin_loss)

MIN_CH, MAX_CH = 16, 128
LEAKY_SLOPE = 0.01          # nn.LeakyReLU's default, the reference's (modules/base.py:33)


def _check_cbr(x, weight, vectors, maps=()):
    """-> (N, H, W, Cin, Cout); placement first, then shapes: all before any library call.  ``vectors``: (name, tensor)
    per-channel [Cout]; ``maps``: (name, tensor) of the output's shape [N, Cout, H, W]."""
    named = (("x", x), ("weight", weight)) + tuple(vectors) + tuple(maps)
    for name, t in named:
        _dev.require_device(f"vpr_head_training: {name}", t)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"x must be float32 [N, Cin, H, W], got {x.dtype} {tuple(x.shape)}")
    N, Cin, H, W = x.shape
    if weight.dim() != 4 or weight.dtype != torch.float32 or weight.shape[1:] != (Cin, 3, 3):
        raise ValueError(f"weight must be float32 [Cout, {Cin}, 3, 3], got {weight.dtype} {tuple(weight.shape)}")
    Cout = weight.shape[0]
    if N < 1 or N > 65535 or H < 1 or W < 1:
        raise ValueError(f"x must be [1 <= N <= 65535, Cin, H >= 1, W >= 1], got {tuple(x.shape)}")
    if Cin % 16 or Cout % 16 or not (MIN_CH <= Cin <= MAX_CH and MIN_CH <= Cout <= MAX_CH):
        raise ValueError(f"head training needs Cin % 16 == 0, Cout % 16 == 0 and {MIN_CH} <= Cin, Cout <= {MAX_CH} "
                         f"(got Cin {Cin}, Cout {Cout})")
    for name, t in vectors:
        if tuple(t.shape) != (Cout,) or t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32 [{Cout}], got {t.dtype} {tuple(t.shape)}")
    for name, t in maps:
        if tuple(t.shape) != (N, Cout, H, W) or t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32 {(N, Cout, H, W)}, got {t.dtype} {tuple(t.shape)}")
    if any(t.device != x.device for _, t in named):
        raise ValueError("every tensor of a layer call must live on one device")
    return N, H, W, Cin, Cout


def _check_slope(slope):
    slope = float(slope)
    if not 0.0 <= slope < 1.0:
        raise ValueError(f"slope must be in [0, 1), got {slope}")
    return slope


def _scratch(lib, N, H, W, Cin, Cout, dev):
    nbytes = int(lib.kp2d_cbr_train_scratch_bytes(N, H, W, Cin, Cout))
    if nbytes == 0:
        raise ValueError(f"head training does not support N {N}, H {H}, W {W}, Cin {Cin}, Cout {Cout}")
    return _dev.scratch(nbytes, dev)


def bn_vectors(bn):
    """A BatchNorm2d on its running statistics as the four per-channel vectors the layer calls take ->
    (scale = gamma / sqrt(var + eps), shift = beta - mean scale, mean, invstd = 1 / sqrt(var + eps)).  Formed with torch on
    the parameters' device."""
    with torch.no_grad():
        invstd = 1.0 / torch.sqrt(bn.running_var.float() + bn.eps)
        scale = bn.weight.detach().float() * invstd
        mean = bn.running_mean.float().contiguous()
        shift = bn.bias.detach().float() - mean * scale
    return scale.contiguous(), shift.contiguous(), mean, invstd.contiguous()


def cbr_forward(x, weight, scale, shift, slope=LEAKY_SLOPE, scratch=None):
    """x [N, Cin, H, W], weight [Cout, Cin, 3, 3], scale and shift [Cout] -> (y, c), both [N, Cout, H, W]:
    c = conv3x3(x, weight) (stride 1, padding 1, no bias) and y = act(scale c + shift), act(v) = v if v > 0 else slope v
    (slope 0.01: LeakyReLU, 0: ReLU).  ``c`` is what ``cbr_backward`` reads."""
    N, H, W, Cin, Cout = _check_cbr(x, weight, (("scale", scale), ("shift", shift)))
    slope = _check_slope(slope)
    x, w = x.contiguous(), weight.detach().contiguous()
    lib = _lib.load()
    scratch = _scratch(lib, N, H, W, Cin, Cout, x.device) if scratch is None else scratch
    y = torch.empty(N, Cout, H, W, dtype=torch.float32, device=x.device)
    c = torch.empty_like(y)
    _lib.check(lib.kp2d_cbr_forward_train(_ptr(x), _ptr(w), _ptr(scale.contiguous()), _ptr(shift.contiguous()), slope, N, H, W,
                                          Cin, Cout, _ptr(y), _ptr(c), _ptr(scratch), scratch.numel(), _stream(x.device)))
    return y, c


def cbr_backward(x, weight, scale, mean, invstd, y, c, dy, slope=LEAKY_SLOPE, need_dx=True, scratch=None):
    """The gradients of a scalar given its gradient ``dy`` with respect to ``cbr_forward``'s ``y`` ->
    (dweight [Cout, Cin, 3, 3], dgamma [Cout], dbeta [Cout], dx [N, Cin, H, W] or None when ``need_dx`` is false).
    dgamma is formed from ``c`` itself, so it is right for a channel whose gamma is 0.  Bit-reproducible, and dweight, dgamma
    and dbeta have the same bits with and without dx."""
    N, H, W, Cin, Cout = _check_cbr(x, weight, (("scale", scale), ("mean", mean), ("invstd", invstd)),
                                    (("y", y), ("c", c), ("dy", dy)))
    slope = _check_slope(slope)
    x, w = x.contiguous(), weight.detach().contiguous()
    lib = _lib.load()
    scratch = _scratch(lib, N, H, W, Cin, Cout, x.device) if scratch is None else scratch
    dw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=x.device)
    dgamma = torch.empty(Cout, dtype=torch.float32, device=x.device)
    dbeta = torch.empty_like(dgamma)
    dx = torch.empty_like(x) if need_dx else None
    _lib.check(lib.kp2d_cbr_backward(_ptr(x), _ptr(w), _ptr(scale.contiguous()), _ptr(mean.contiguous()), _ptr(invstd.contiguous()),
                                     slope, _ptr(y.contiguous()), _ptr(c.contiguous()), _ptr(dy.contiguous()), N, H, W, Cin, Cout,
                                     _ptr(dw), _ptr(dgamma), _ptr(dbeta), _ptr(dx), _ptr(scratch), scratch.numel(),
                                     _stream(x.device)))
    return dw, dgamma, dbeta, dx


def _check_drop(drop, N, Cout, x):
    if drop is None:
        return None
    _dev.require_device("vpr_head_training: drop", drop)
    if tuple(drop.shape) != (N, Cout) or drop.dtype != torch.float32 or drop.device != x.device:
        raise ValueError(f"drop must be float32 {(N, Cout)} on {x.device}, got {drop.dtype} {tuple(drop.shape)} on {drop.device}")
    return drop.contiguous()


def cbr_forward_batch(x, weight, gamma, beta, eps=1e-5, slope=LEAKY_SLOPE, drop=None, running=None, momentum=0.1, scratch=None):
    """``cbr_forward`` with BatchNorm on the batch's own statistics -> (y, c, mean, invstd): over the M = N H W values of a
    channel, mean = sum c / M, var = sum (c - mean)^2 / M (biased), invstd = 1 / sqrt(var + eps),
    y = act(gamma invstd (c - mean) + beta) drop[n, co].  ``drop``: [N, Cout] of 0 or 1 / (1 - p) (``dropout2d_scale``), None:
    no dropout.  ``running`` = (running_mean, running_var), float32 [Cout] contiguous, updated in place on the device:
    (1 - momentum) running + momentum (mean, var M / (M - 1)).  M < 2 raises, as torch does."""
    vectors = (("gamma", gamma), ("beta", beta)) + ((("running_mean", running[0]), ("running_var", running[1])) if running is not None else ())
    N, H, W, Cin, Cout = _check_cbr(x, weight, vectors)
    slope = _check_slope(slope)
    eps, momentum = float(eps), float(momentum)
    if not (0.0 <= eps < float("inf") and 0.0 <= momentum <= 1.0):
        raise ValueError(f"eps must be finite and >= 0 and momentum in [0, 1], got {eps}, {momentum}")
    if N * H * W < 2:
        raise ValueError(f"batch statistics need more than 1 value per channel, got x {tuple(x.shape)}")
    if running is not None and not all(t.is_contiguous() for t in running):
        raise ValueError("running_mean and running_var must be contiguous: they are updated in place")
    drop = _check_drop(drop, N, Cout, x)
    x, w = x.contiguous(), weight.detach().contiguous()
    lib = _lib.load()
    scratch = _scratch(lib, N, H, W, Cin, Cout, x.device) if scratch is None else scratch
    y = torch.empty(N, Cout, H, W, dtype=torch.float32, device=x.device)
    c = torch.empty_like(y)
    mean = torch.empty(Cout, dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    rm, rv = (running[0].detach(), running[1].detach()) if running is not None else (None, None)
    _lib.check(lib.kp2d_cbr_forward_batchnorm(_ptr(x), _ptr(w), _ptr(gamma.detach().contiguous()), _ptr(beta.detach().contiguous()), eps,
                                              slope, _ptr(drop), momentum, _ptr(rm), _ptr(rv), N, H, W, Cin, Cout, _ptr(y), _ptr(c),
                                              _ptr(mean), _ptr(invstd), _ptr(scratch), scratch.numel(), _stream(x.device)))
    return y, c, mean, invstd


def cbr_backward_batch(x, weight, gamma, mean, invstd, y, c, dy, slope=LEAKY_SLOPE, drop=None, need_dx=True, scratch=None):
    """``cbr_backward`` for ``cbr_forward_batch`` (its mean, invstd, y, c and the same ``drop``) -> (dweight, dgamma, dbeta, dx
    or None): g = dy drop (y > 0 ? 1 : slope), dbeta = sum g, dgamma = sum g xhat, dc = gamma invstd (g - dbeta / M -
    xhat dgamma / M) with xhat = (c - mean) invstd: the two terms through the batch mean and variance included.
    Bit-reproducible, and dweight, dgamma and dbeta have the same bits with and without dx."""
    N, H, W, Cin, Cout = _check_cbr(x, weight, (("gamma", gamma), ("mean", mean), ("invstd", invstd)), (("y", y), ("c", c), ("dy", dy)))
    slope = _check_slope(slope)
    if N * H * W < 2:
        raise ValueError(f"batch statistics need more than 1 value per channel, got x {tuple(x.shape)}")
    drop = _check_drop(drop, N, Cout, x)
    x, w = x.contiguous(), weight.detach().contiguous()
    lib = _lib.load()
    scratch = _scratch(lib, N, H, W, Cin, Cout, x.device) if scratch is None else scratch
    dw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=x.device)
    dgamma = torch.empty(Cout, dtype=torch.float32, device=x.device)
    dbeta = torch.empty_like(dgamma)
    dx = torch.empty_like(x) if need_dx else None
    _lib.check(lib.kp2d_cbr_backward_batchnorm(_ptr(x), _ptr(w), _ptr(gamma.detach().contiguous()), _ptr(mean.contiguous()),
                                               _ptr(invstd.contiguous()), slope, _ptr(drop), _ptr(y.contiguous()), _ptr(c.contiguous()),
                                               _ptr(dy.contiguous()), N, H, W, Cin, Cout, _ptr(dw), _ptr(dgamma), _ptr(dbeta), _ptr(dx),
                                               _ptr(scratch), scratch.numel(), _stream(x.device)))
    return dw, dgamma, dbeta, dx


def dropout2d_scale(N, C, p, seed, step, layer, device):
    """The Dropout2d factors of one step -> float32 [N, C] on ``device``: 0 for a dropped (frame, channel) plane, 1 / (1 - p)
    for a kept one.  A counter-based draw of (seed, step, layer, n, c) (include/kp2d.h states the layout), not torch's
    random stream: the same arguments give the same mask anywhere."""
    N, C, p, seed, step, layer = int(N), int(C), float(p), int(seed), int(step), int(layer)
    if N < 1 or C < 1 or N * C >= 2 ** 31:
        raise ValueError(f"dropout2d_scale needs N, C >= 1 and N * C < 2^31, got {N}, {C}")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout2d_scale: p must be in [0, 1), got {p}")
    if not (0 <= seed < 2 ** 64 and 0 <= step < 2 ** 32 and 0 <= layer < 2 ** 31):
        raise ValueError(f"dropout2d_scale: seed {seed} outside [0, 2^64), step {step} outside [0, 2^32) or layer {layer} outside [0, 2^31)")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"dropout2d_scale: there is no CPU path, got device {device}")
    drop = torch.empty(N, C, dtype=torch.float32, device=device)
    _lib.check(_lib.load().kp2d_dropout2d_mask(_ptr(drop), N, C, p, seed, step, layer, _stream(drop.device)))
    return drop


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


class VPRHeadTrainer:
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
    ``step_features`` does not.  GeM / ConvAP poolers and ``remove_netvlad`` models raise ValueError."""

    def __init__(self, model, lr=1e-4, margin=0.1, betas=(0.9, 0.999), eps=1e-8, bn="running", dropout=0.0, seed=0):
        if getattr(model, "global_descriptor_method", None) != "netvlad":
            raise ValueError(f"VPRHeadTrainer needs a NetVLAD pooler, the model has {getattr(model, 'global_descriptor_method', None)!r}")
        if getattr(model, "remove_netvlad", False) or not hasattr(model.vlad_head, "netvlad"):
            raise ValueError("VPRHeadTrainer: the model was built with remove_netvlad")
        if not (lr >= 0 and margin >= 0 and 0 <= betas[0] < 1 and 0 <= betas[1] < 1 and eps >= 0):
            raise ValueError(f"VPRHeadTrainer: lr {lr}, margin {margin}, betas {betas}, eps {eps}")
        self.model, self.lr, self.margin, self.betas, self.eps = model, float(lr), float(margin), tuple(betas), float(eps)
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
        self.steps = 0
        self.n_active = None          # device int32 scalar of the last step
        self._state = {}

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

    def _moments(self, p):
        st = self._state.get(id(p))
        if st is None or st[0].device != p.device or st[0].shape != p.shape:
            st = (torch.zeros_like(p.data), torch.zeros_like(p.data))
            self._state[id(p)] = st
        return st

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
            vec = bn_vectors(layer.bn)
            y, c = cbr_forward(x, layer.conv.weight, vec[0], vec[1], self.slope, scratch)
            acts.append((x, y, c, vec))
            x = y if i > 0 or drop is None else y * drop[:, :, None, None]
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
        if not all(p.is_contiguous() for p in params):
            raise ValueError("VPRHeadTrainer: the head's parameters must be contiguous")
        netvlad = self.model.vlad_head.netvlad
        weight, cent = netvlad.conv.weight, netvlad.centroids
        lib = _lib.load()
        N, _, H, W = feat.shape
        batch = self.bn == "batch"
        if batch and N * H * W < 2:
            raise ValueError(f"bn='batch' needs more than 1 value per channel, got feat {tuple(feat.shape)}")
        cmax = max(max(l.conv.weight.shape[:2]) for l in self.layers)
        scratch = _scratch(lib, N, H, W, cmax, cmax, feat.device)        # the largest layer's: every layer call fits
        if drop is None and self.dropout > 0:
            drop = dropout2d_scale(N, self.layers[0].conv.weight.shape[0], self.dropout, self.seed, self.steps + 1, 1, feat.device)
        if batch:
            acts = self._forward_batch(feat.contiguous(), scratch, drop)
        else:
            acts = self.forward_features(feat.contiguous(), scratch, drop)
        enc = acts[-1][1]
        x, w, N, S, C, K = _check_layer(enc, weight, cent)
        vscratch = _vlad_scratch(lib, N, S, C, K, x.device)
        vlad, saved = netvlad_forward(x, w, cent, vscratch)
        loss, dvlad, self.n_active = triplet_margin_loss(vlad, B, neg_counts, self.margin, vscratch)
        dW, dcent = netvlad_backward(x, w, cent, saved, dvlad, vscratch)
        dy = netvlad_backward_input(enc, w, cent, saved, dvlad, vscratch)
        grads = [None] * 9 + [dW, dcent]
        for i in (2, 1, 0):
            layer = self.layers[i]
            if batch:
                lx, ly, lc, (mean, invstd) = acts[i]
                dw, dgamma, dbeta, dy = cbr_backward_batch(lx, layer.conv.weight, layer.bn.weight, mean, invstd, ly, lc, dy, self.slope,
                                                           drop if i == 0 else None, need_dx=i > 0, scratch=scratch)
            else:
                lx, ly, lc, (scale, _, mean, invstd) = acts[i]
                if i == 0 and drop is not None:
                    dy = dy * drop[:, :, None, None]
                dw, dgamma, dbeta, dy = cbr_backward(lx, layer.conv.weight, scale, mean, invstd, ly, lc, dy, self.slope,
                                                     need_dx=i > 0, scratch=scratch)      # (the backbone is frozen: no dx of layer 1)
            grads[3 * i:3 * i + 3] = [dw, dgamma, dbeta]
        self.steps += 1
        for p, g in zip(params, grads):
            m, v = self._moments(p)
            adam_step(p.data, g.view(p.shape), m, v, self.steps, self.lr, self.betas, self.eps)
            with torch.no_grad():     # ``p.data`` counts versions on its own: bump the parameter's, which the engine watches
                torch.autograd.graph.increment_version(p)
        if batch:
            with torch.no_grad():     # the kernel wrote the running statistics through their addresses: bump those too
                for layer in self.layers:
                    if layer.bn.track_running_stats:
                        torch.autograd.graph.increment_version(layer.bn.running_mean)
                        torch.autograd.graph.increment_version(layer.bn.running_var)
                        layer.bn.num_batches_tracked.add_(1)
        return loss
