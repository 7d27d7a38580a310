"""What the five on-device trainers share (``vlad_training``, ``vpr_head_training``, ``seg_training``, ``depth_training``,
``keypoint_training``): the layer calls on device tensors, and the Adam core of a trainer.

* ``cbr_forward`` / ``cbr_backward``, ``cbr_forward_batch`` / ``cbr_backward_batch``, ``dropout2d_scale`` — a Conv + BatchNorm +
  (Leaky)ReLU layer on running or on batch statistics, and the Dropout2d factors (csrc/vpr_head_train.hip); ``bn_vectors`` and
  ``cbr_layer_forward`` / ``cbr_layer_backward`` run one such layer of a model and undo it from what the forward kept.
* ``conv_bias_forward`` / ``conv_bias_backward``, ``maxpool2_forward`` / ``maxpool2_backward``, ``shuffle_cat_forward`` /
  ``shuffle_cat_backward`` — a 3x3 convolution with bias and the dense heads' two scale changes (csrc/seg_train.hip).
* ``layernorm_*``, ``pointwise_*``, ``patch2_*``, ``dwconv3_*``, ``attention_*`` and ``attention_module_forward`` /
  ``attention_module_backward`` — the stages of the attention head's SegFormerAttentionModule (csrc/attention_train.hip).
* ``adam_step`` (csrc/vlad_train.hip) and ``AdamTrainer``, the base of every trainer: settings, moments, the one update loop.
* ``hard_triplet_loss`` / ``HardTripletLoss`` / ``view_labels`` (csrc/hard_triplet.hip) — the multitask run's batch-hard triplet
  loss on view pairs, the one loss two trainers step on (``NetVLADTrainer`` and ``VPRHeadTrainer``); ``vlad_training`` is where
  callers import it from.

The other losses and the NetVLAD layer calls stay with their trainers.  The two styles of refusal stay as they were: the cbr calls and
``adam_step`` raise RuntimeError for a CPU tensor (``_dev.require_device``), the others ValueError (``_is_device``, the one
place that says what a device tensor is).  Every check runs before the library is loaded.
"""
from __future__ import annotations

import torch

from . import _dev, _lib
from ._dev import ptr as _ptr, stream as _stream

MIN_CH, MAX_CH = 16, 128
LEAKY_SLOPE = 0.01          # nn.LeakyReLU's default, the reference's (modules/base.py:33)


# ---- checks ------------------------------------------------------------------------------------------------------------
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


def _check_drop(drop, N, Cout, x):
    if drop is None:
        return None
    _dev.require_device("vpr_head_training: drop", drop)
    if tuple(drop.shape) != (N, Cout) or drop.dtype != torch.float32 or drop.device != x.device:
        raise ValueError(f"drop must be float32 {(N, Cout)} on {x.device}, got {drop.dtype} {tuple(drop.shape)} on {drop.device}")
    return drop.contiguous()


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


def _cbr_scratch(lib, N, H, W, Cin, Cout, dev):
    nbytes = int(lib.kp2d_cbr_train_scratch_bytes(N, H, W, Cin, Cout))
    if nbytes == 0:
        raise ValueError(f"head training does not support N {N}, H {H}, W {W}, Cin {Cin}, Cout {Cout}")
    return _dev.scratch(nbytes, dev)


def _bias_scratch(lib, N, H, W, Cin, Cout, dev):
    nbytes = int(lib.kp2d_conv_bias_scratch_bytes(N, H, W, Cin, Cout))
    if nbytes == 0:
        raise ValueError(f"the last layer does not support N {N}, H {H}, W {W}, Cin {Cin}, Cout {Cout}")
    return _dev.scratch(nbytes, dev)


# ---- Adam --------------------------------------------------------------------------------------------------------------
def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's update (no weight decay, no amsgrad) of ``param`` and its two moment buffers in place;
    ``step`` counts from 1.  The kernel writes through raw pointers, so afterwards the tensors' version counters are bumped:
    whatever caches by version (the engine's packed weights) sees the change."""
    tensors = (("param", param), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq))
    for name, t in tensors:
        _dev.require_device(f"adam_step: {name}", t)
    for name, t in tensors:
        if t.dtype != torch.float32 or t.numel() != param.numel() or t.device != param.device or not t.is_contiguous():
            raise ValueError(f"adam_step: {name} must be a contiguous float32 tensor of {param.numel()} elements on {param.device}")
    if int(step) < 1:
        raise ValueError("adam_step: steps count from 1")
    lib = _lib.load()
    _lib.check(lib.kp2d_adam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), int(step), float(lr),
                                  float(betas[0]), float(betas[1]), float(eps), _stream(param.device)))
    with torch.no_grad():
        for t in (param, exp_avg, exp_avg_sq):
            torch.autograd.graph.increment_version(t)
    return param


class AdamTrainer:
    """The optimizer half of a trainer: ``lr``, ``betas``, ``eps``, ``steps`` (the updates made so far), the two moment
    buffers of every parameter and the update loop.  A trainer names itself in ``_WHO``, the prefix of its messages, calls
    ``_init_adam`` where its settings' refusal belongs among its others, and ends a step with ``_apply``."""

    _WHO = None

    def _init_adam(self, lr, betas, eps, margin=None):
        """``margin``: the triplet trainers' hinge margin, refused together with the optimizer's settings in one message."""
        if not (lr >= 0 and (margin is None or margin >= 0) and 0 <= betas[0] < 1 and 0 <= betas[1] < 1 and eps >= 0):
            raise ValueError(f"{self._WHO}: lr {lr}, " + ("" if margin is None else f"margin {margin}, ") + f"betas {betas}, eps {eps}")
        self.lr, self.betas, self.eps = float(lr), tuple(betas), float(eps)
        if margin is not None:
            self.margin = float(margin)
        self.steps = 0
        self._state = {}

    def _moments(self, p):
        """-> (exp_avg, exp_avg_sq) of ``p``, zeros on first use and again when ``p`` changed its device or shape."""
        st = self._state.get(id(p))
        if st is None or st[0].device != p.device or st[0].shape != p.shape:
            st = (torch.zeros_like(p.data), torch.zeros_like(p.data))
            self._state[id(p)] = st
        return st

    def _check_contiguous(self, params, whose):
        if not all(p.is_contiguous() for p in params):
            raise ValueError(f"{self._WHO}: {whose} parameters must be contiguous")

    def _apply(self, params, grads):
        """One Adam update of ``params`` from ``grads``, in that order, on the device."""
        self.steps += 1
        for p, g in zip(params, grads):
            m, v = self._moments(p)
            adam_step(p.data, g.view(p.shape), m, v, self.steps, self.lr, self.betas, self.eps)
            with torch.no_grad():     # ``p.data`` counts versions on its own: bump the parameter's, which the engine watches
                torch.autograd.graph.increment_version(p)       # (_weights_signature: it re-packs its weights)


# ---- the view loss of the two place-recognition trainers -----------------------------------------------------------------
MAX_HT_ROWS = 512
QUIRK_MARGIN = 0.1      # what the reference's hardest branch adds, whatever margin its HardTripletLoss was built with


def view_labels(N, device):
    """The labels of a batch of N view pairs, rows ordered plain views then augmented views: cat(arange(N), arange(N)) int32."""
    r = torch.arange(int(N), dtype=torch.int32, device=device)
    return torch.cat([r, r])


def hard_triplet_loss(emb, labels, margin=0.1, hardest=True, squared=False, weight=1.0, scratch=None):
    """emb [M, dim] float32, labels [M] integers, both on the device, M <= 512 ->
    (loss [], demb like emb, stats [4] int64): the reference's HardTripletLoss (src/kp2dtiny/utils/losses.py) times
    ``weight``, with its gradient.  ``hardest``: per anchor the hardest positive against the hardest negative, the mean of
    relu(hp - hn + margin); else the sum over all valid triplets divided by the number of hard ones.  ``margin`` is used as
    given in both modes (``HardTripletLoss`` below keeps the reference's quirk).  ``stats``: anchors with a positive hinge
    (``hardest``) or hard triplets, anchors without a positive, anchors without a negative, zero off-diagonal distances.
    The formulas, the tie rule (lowest index) and the summation orders are include/kp2d.h's; bit-reproducible.
    Labels are compared as int32: wider integers must fit its range (they are converted on the device and not read back, so
    values outside it wrap and two of them may then compare equal)."""
    for name, t in (("emb", emb), ("labels", labels)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise ValueError(f"hard_triplet_loss: {name} must be a device tensor (there is no CPU path)")
    if emb.dim() != 2 or emb.dtype != torch.float32 or emb.shape[0] < 1 or emb.shape[1] < 1:
        raise ValueError(f"emb must be float32 [M, dim], got {emb.dtype} {tuple(emb.shape)}")
    M, dim = emb.shape
    if labels.dim() != 1 or labels.numel() != M or labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise ValueError(f"labels must be an integer tensor of length {M}, got {labels.dtype} {tuple(labels.shape)}")
    if M > MAX_HT_ROWS:
        raise ValueError(f"hard_triplet_loss supports at most {MAX_HT_ROWS} rows, got {M}")
    if labels.device != emb.device:
        raise ValueError("emb and labels must live on one device")
    margin, weight = float(margin), float(weight)
    if not (0 <= margin < float("inf")) or weight != weight or abs(weight) == float("inf"):
        raise ValueError(f"margin must be finite and >= 0 and weight finite, got margin {margin}, weight {weight}")
    emb = emb.detach().contiguous()
    lab = labels.detach().to(torch.int32).contiguous()      # (labels beyond int32 wrap: see the docstring)
    lib = _lib.load()
    dev = emb.device
    scratch = _dev.scratch(lib.kp2d_hard_triplet_scratch_bytes(M, dim), dev) if scratch is None else scratch
    loss = torch.empty((), dtype=torch.float32, device=dev)
    demb = torch.empty_like(emb)
    stats = torch.empty(4, dtype=torch.int64, device=dev)
    flags = (_lib.KP2D_HT_HARDEST if hardest else 0) | (_lib.KP2D_HT_SQUARED if squared else 0)
    _lib.check(lib.kp2d_hard_triplet_loss(_ptr(emb), _ptr(lab), M, dim, margin, flags, weight, _ptr(loss), _ptr(demb), _ptr(stats),
                                          _ptr(scratch), scratch.numel(), _stream(dev)))
    return loss, demb, stats


class HardTripletLoss:
    """The reference's class surface: ``crit = HardTripletLoss(margin=0.1, hardest=False, squared=False)``,
    ``crit(emb, labels)`` -> the loss (a device scalar); ``crit.grad`` and ``crit.stats`` are the gradient with respect to
    ``emb`` and the ``stats`` of the last call.  The reference's quirk is reproduced: its ``hardest`` branch adds the
    literal 0.1 and never reads ``self.margin``, so ``hardest=True`` uses 0.1 whatever ``margin`` says (the multitask run
    builds ``HardTripletLoss(margin=0.5, hardest=True)`` and trains with 0.1).  ``hard_triplet_loss`` takes the margin it
    is given."""

    def __init__(self, margin=0.1, hardest=False, squared=False):
        self.margin, self.hardest, self.squared = margin, bool(hardest), bool(squared)
        self.grad = self.stats = None

    def __call__(self, embeddings, labels):
        margin = QUIRK_MARGIN if self.hardest else self.margin
        loss, self.grad, self.stats = hard_triplet_loss(embeddings, labels, margin, self.hardest, self.squared)
        return loss

    forward = __call__


def _views_loss(trainer, N, margin, weight):
    """-> the view step's ``loss_fn(vlad [2 N, dim], scratch)``; the call's ``stats`` land in ``trainer.ht_stats``.  (The
    loss takes a scratch of its own: its [2 N, 2 N] matrices need not fit the layer's.)"""
    if 2 * N > MAX_HT_ROWS:
        raise ValueError(f"{trainer._WHO}: a view step takes at most {MAX_HT_ROWS // 2} pairs, got {N}")

    def loss_fn(vlad, scratch):
        loss, dvlad, trainer.ht_stats = hard_triplet_loss(vlad, view_labels(N, vlad.device), margin, True, False, weight)
        return loss, dvlad
    return loss_fn


# ---- Conv + BatchNorm + (Leaky)ReLU -----------------------------------------------------------------------------------------
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
    scratch = _cbr_scratch(lib, N, H, W, Cin, Cout, x.device) if scratch is None else scratch
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
    scratch = _cbr_scratch(lib, N, H, W, Cin, Cout, x.device) if scratch is None else scratch
    dw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=x.device)
    dgamma = torch.empty(Cout, dtype=torch.float32, device=x.device)
    dbeta = torch.empty_like(dgamma)
    dx = torch.empty_like(x) if need_dx else None
    _lib.check(lib.kp2d_cbr_backward(_ptr(x), _ptr(w), _ptr(scale.contiguous()), _ptr(mean.contiguous()), _ptr(invstd.contiguous()),
                                     slope, _ptr(y.contiguous()), _ptr(c.contiguous()), _ptr(dy.contiguous()), N, H, W, Cin, Cout,
                                     _ptr(dw), _ptr(dgamma), _ptr(dbeta), _ptr(dx), _ptr(scratch), scratch.numel(),
                                     _stream(x.device)))
    return dw, dgamma, dbeta, dx


def cbr_layer_forward(layer, x, slope, scratch=None):
    """A model's Conv + BatchNorm layer (``layer.conv``, ``layer.bn``) on its running statistics ->
    (x, y, c, (scale, shift, mean, invstd)): what ``cbr_layer_backward`` takes."""
    vec = bn_vectors(layer.bn)
    y, c = cbr_forward(x, layer.conv.weight, vec[0], vec[1], slope, scratch)
    return (x, y, c, vec)


def cbr_layer_backward(layer, saved, dy, slope, need_dx=True, scratch=None):
    """``cbr_layer_forward``'s tuple and the gradient of its ``y`` -> (dweight, dgamma, dbeta, dx or None)."""
    x, y, c, (scale, _, mean, invstd) = saved
    return cbr_backward(x, layer.conv.weight, scale, mean, invstd, y, c, dy, slope, need_dx=need_dx, scratch=scratch)


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
    scratch = _cbr_scratch(lib, N, H, W, Cin, Cout, x.device) if scratch is None else scratch
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
    scratch = _cbr_scratch(lib, N, H, W, Cin, Cout, x.device) if scratch is None else scratch
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


# ---- convolution with bias, pooling, pixel shuffle ------------------------------------------------------------------------
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


# ---- the attention head's SegFormerAttentionModule, stage by stage (csrc/attention_train.hip) -------------------------------
ATT_CH = (48, 64, 96, 128)      # the channel counts the stage calls take
ATT_HEADS = 4
LN_EPS = 1e-5                   # the reference's LayerNorm(dim, eps=1e-5)


def _check_att(where, maps, weights=(), vectors=(), attention=False):
    """``maps``: (name, tensor, channels or None) float32 [N, C, H, W] of one N, H, W; ``weights``: (name, tensor, shape);
    ``vectors``: (name, tensor, numel) -> (N, H, W).  Placement, dtype, contiguity, then shapes: all before any library call."""
    _f32_maps(where, tuple((n, t) for n, t, _ in maps))
    for name, t, _ in tuple(weights) + tuple(vectors):
        if not isinstance(t, torch.Tensor) or not _is_device(t):
            raise ValueError(f"{where}: {name} must be a device tensor (there is no CPU path)")
        if t.dtype != torch.float32 or t.device != maps[0][1].device:
            raise ValueError(f"{where}: {name} must be float32 on {maps[0][1].device}, got {t.dtype} on {t.device}")
    for name, t in tuple((n, t) for n, t, _ in maps) + tuple((n, t) for n, t, _ in weights) + tuple((n, t) for n, t, _ in vectors):
        if not t.is_contiguous():
            raise ValueError(f"{where}: {name} must be contiguous")
    N, _, H, W = maps[0][1].shape
    if not (1 <= N <= 65535 and H >= 1 and W >= 1 and H * W <= 2 ** 24):
        raise ValueError(f"{where}: needs 1 <= N <= 65535, H, W >= 1 and H W <= 2^24, got {tuple(maps[0][1].shape)}")
    for name, t, c in maps:
        if c is not None and t.shape[1] != c:
            raise ValueError(f"{where}: {name} must have {c} channels, got {tuple(t.shape)}")
        if t.shape[1] not in ATT_CH:
            raise ValueError(f"{where}: {name} has {t.shape[1]} channels; the kernels take {ATT_CH}")
    for name, t, shape in weights:
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{where}: {name} must be {tuple(shape)}, got {tuple(t.shape)}")
    for name, t, n in vectors:
        if t.numel() != n:
            raise ValueError(f"{where}: {name} must have {n} elements, got {tuple(t.shape)}")
    if attention and (H < 2 or W < 2 or maps[0][1].shape[1] > 64):
        raise ValueError(f"{where}: needs H, W >= 2 (one 2 x 2 key patch) and 48 or 64 channels, got {tuple(maps[0][1].shape)}")
    return N, H, W


def _att_channels(x):
    """The channel count of a call's first map, which ``_check_att`` then checks in full."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"the first argument must be a float32 device tensor [N, C, H, W], got {type(x).__name__} "
                         f"{tuple(x.shape) if isinstance(x, torch.Tensor) else ''}")
    return x.shape[1]


def _same(where, name, t, shape):
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{where}: {name} must be {tuple(shape)}, got {tuple(t.shape)}")


def _att_scratch(lib, N, H, W, Cin, Cout, dev):
    nbytes = int(lib.kp2d_att_train_scratch_bytes(N, H, W, Cin, Cout))
    if nbytes == 0:
        raise ValueError(f"attention training does not support N {N}, H {H}, W {W}, channels {Cin}, {Cout}")
    return _dev.scratch(nbytes, dev)


def layernorm_forward(x, g, b, eps=LN_EPS):
    """The reference's channel LayerNorm: x [N, C, H, W], g and b of C elements -> (y, mean, rinv):
    y = (x - mean) / (sqrt(var_biased) + eps) g + b over the channels of each pixel; mean and rinv = 1 / (sqrt(var) + eps)
    are [N, H, W], what ``layernorm_backward`` reads."""
    C = _att_channels(x)
    N, H, W = _check_att("layernorm_forward", (("x", x, None),), vectors=(("g", g, C), ("b", b, C)))
    y = torch.empty_like(x)
    mean = torch.empty(N, H, W, dtype=torch.float32, device=x.device)
    rinv = torch.empty_like(mean)
    _lib.check(_lib.load().kp2d_layernorm_forward_train(_ptr(x), _ptr(g.detach()), _ptr(b.detach()), N, C, H, W, float(eps), _ptr(y), _ptr(mean),
                                                        _ptr(rinv), _stream(x.device)))
    return y, mean, rinv


def layernorm_backward(x, g, mean, rinv, dy, eps=LN_EPS):
    """-> (dx, dg, db), dg and db shaped like ``g``.  A pixel whose channels are all equal (sqrt(var) = 0) takes the term
    through the deviation as 0, where torch gives NaN.  Bit-reproducible."""
    C = _att_channels(x)
    N, H, W = _check_att("layernorm_backward", (("x", x, None), ("dy", dy, C)), vectors=(("g", g, C),))
    for name, t in (("mean", mean), ("rinv", rinv)):
        if not isinstance(t, torch.Tensor) or not _is_device(t) or t.dtype != torch.float32 or tuple(t.shape) != (N, H, W) or not t.is_contiguous():
            raise ValueError(f"layernorm_backward: {name} must be a contiguous float32 device tensor {(N, H, W)}")
    _same("layernorm_backward", "dy", dy, x.shape)
    lib = _lib.load()
    scratch = _att_scratch(lib, N, H, W, C, C, x.device)
    dx, dg, db = torch.empty_like(x), torch.empty_like(g.detach()), torch.empty_like(g.detach())
    _lib.check(lib.kp2d_layernorm_backward(_ptr(x), _ptr(g.detach()), _ptr(mean), _ptr(rinv), _ptr(dy), N, C, H, W, float(eps), _ptr(dx), _ptr(dg),
                                           _ptr(db), _ptr(scratch), scratch.numel(), _stream(x.device)))
    return dx, dg, db


def pointwise_forward(x, weight, bias=None, gelu=False):
    """x [N, Cin, H, W], weight [Cout, Cin, 1, 1], bias [Cout] or None -> (y, pre): the 1 x 1 convolution; with ``gelu`` y is
    nn.GELU()'s exact (erf) form of it and ``pre`` the value before, else ``pre`` is None."""
    Cin = _att_channels(x)
    if not isinstance(weight, torch.Tensor) or weight.dim() != 4:
        raise ValueError("pointwise_forward: weight must be a [Cout, Cin, 1, 1] device tensor")
    Cout = weight.shape[0]
    N, H, W = _check_att("pointwise_forward", (("x", x, None),), weights=(("weight", weight, (Cout, Cin, 1, 1)),),
                         vectors=(("bias", bias, Cout),) if bias is not None else ())
    if Cout not in ATT_CH:
        raise ValueError(f"pointwise_forward: Cout {Cout} is not one of {ATT_CH}")
    y = torch.empty(N, Cout, H, W, dtype=torch.float32, device=x.device)
    pre = torch.empty_like(y) if gelu else None
    _lib.check(_lib.load().kp2d_pointwise_forward_train(_ptr(x), _ptr(weight.detach()), _ptr(None if bias is None else bias.detach()), N, H, W,
                                                        Cin, Cout, int(bool(gelu)), _ptr(y), _ptr(pre), _stream(x.device)))
    return y, pre


def pointwise_backward(x, weight, dy, pre=None, need_dx=True, need_dbias=True):
    """``pointwise_forward``'s input and weight, the gradient ``dy`` of its ``y`` and, for a call with ``gelu``, its ``pre`` ->
    (dx or None, dweight [Cout, Cin, 1, 1], dbias [Cout] or None).  Bit-reproducible."""
    Cin = _att_channels(x)
    if not isinstance(weight, torch.Tensor) or weight.dim() != 4:
        raise ValueError("pointwise_backward: weight must be a [Cout, Cin, 1, 1] device tensor")
    Cout = weight.shape[0]
    maps = (("x", x, None), ("dy", dy, Cout)) + ((("pre", pre, Cout),) if pre is not None else ())
    N, H, W = _check_att("pointwise_backward", maps, weights=(("weight", weight, (Cout, Cin, 1, 1)),))
    for name, t, _ in maps[1:]:
        _same("pointwise_backward", name, t, (N, Cout, H, W))
    lib = _lib.load()
    dev = x.device
    if pre is not None:
        dpre = torch.empty_like(dy)
        _lib.check(lib.kp2d_gelu_backward(_ptr(pre), _ptr(dy), dy.numel(), _ptr(dpre), _stream(dev)))
        dy = dpre
    scratch = _att_scratch(lib, N, H, W, Cin, Cout, dev)
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(weight.detach())
    db = torch.empty(Cout, dtype=torch.float32, device=dev) if need_dbias else None
    _lib.check(lib.kp2d_pointwise_backward(_ptr(x), _ptr(weight.detach()), _ptr(dy), N, H, W, Cin, Cout, _ptr(dx), _ptr(dw), _ptr(db),
                                           _ptr(scratch), scratch.numel(), _stream(dev)))
    return dx, dw, db


def _check_patch2(where, x, weight, dy=None):
    C = _att_channels(x)
    N, H, W = _check_att(where, (("x", x, None),), weights=(("weight", weight, (2 * C, C, 2, 2)),), attention=True)
    if dy is not None:
        _f32_maps(where, (("dy", dy),))
        if tuple(dy.shape) != (N, 2 * C, H // 2, W // 2) or dy.device != x.device or not dy.is_contiguous():
            raise ValueError(f"{where}: dy must be contiguous {(N, 2 * C, H // 2, W // 2)} on {x.device}, got {tuple(dy.shape)}")
    return N, C, H, W


def patch2_forward(x, weight):
    """``to_kv``: x [N, C, H, W], weight [2 C, C, 2, 2] -> the 2 x 2 stride-2 convolution without padding or bias,
    [N, 2 C, H // 2, W // 2]; an odd map's last row or column feeds nothing."""
    N, C, H, W = _check_patch2("patch2_forward", x, weight)
    y = torch.empty(N, 2 * C, H // 2, W // 2, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().kp2d_patch2_forward_train(_ptr(x), _ptr(weight.detach()), N, C, H, W, _ptr(y), _stream(x.device)))
    return y


def patch2_backward(x, weight, dy, need_dx=True):
    """-> (dx or None, dweight [2 C, C, 2, 2]); the dx of an odd map's last row or column is written as exact zeros."""
    N, C, H, W = _check_patch2("patch2_backward", x, weight, dy)
    lib = _lib.load()
    scratch = _att_scratch(lib, N, H, W, C, 2 * C, x.device)
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(weight.detach())
    _lib.check(lib.kp2d_patch2_backward(_ptr(x), _ptr(weight.detach()), _ptr(dy), N, C, H, W, _ptr(dx), _ptr(dw), _ptr(scratch), scratch.numel(),
                                        _stream(x.device)))
    return dx, dw


def dwconv3_forward(x, weight, bias):
    """x [N, C, H, W], weight [C, 1, 3, 3], bias [C] -> the depthwise 3 x 3 convolution (padding 1) + bias."""
    C = _att_channels(x)
    N, H, W = _check_att("dwconv3_forward", (("x", x, None),), weights=(("weight", weight, (C, 1, 3, 3)),), vectors=(("bias", bias, C),))
    y = torch.empty_like(x)
    _lib.check(_lib.load().kp2d_dwconv3_forward_train(_ptr(x), _ptr(weight.detach()), _ptr(bias.detach()), N, C, H, W, _ptr(y), _stream(x.device)))
    return y


def dwconv3_backward(x, weight, dy, need_dx=True):
    """-> (dx or None, dweight [C, 1, 3, 3], dbias [C]).  Bit-reproducible."""
    C = _att_channels(x)
    N, H, W = _check_att("dwconv3_backward", (("x", x, None), ("dy", dy, C)), weights=(("weight", weight, (C, 1, 3, 3)),))
    _same("dwconv3_backward", "dy", dy, x.shape)
    lib = _lib.load()
    scratch = _att_scratch(lib, N, H, W, C, C, x.device)
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(weight.detach())
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    _lib.check(lib.kp2d_dwconv3_backward(_ptr(x), _ptr(weight.detach()), _ptr(dy), N, C, H, W, _ptr(dx), _ptr(dw), _ptr(db), _ptr(scratch),
                                         scratch.numel(), _stream(x.device)))
    return dx, dw, db


def _check_attention(where, q, kv, others=()):
    C = _att_channels(q)
    N, H, W = _check_att(where, (("q", q, None),) + tuple((n, t, C) for n, t in others), attention=True)
    _f32_maps(where, (("kv", kv),))
    if tuple(kv.shape) != (N, 2 * C, H // 2, W // 2) or kv.device != q.device or not kv.is_contiguous():
        raise ValueError(f"{where}: kv must be contiguous {(N, 2 * C, H // 2, W // 2)} on {q.device}, got {tuple(kv.shape)}")
    for name, t in others:
        _same(where, name, t, q.shape)
    return N, C, H, W


def attention_forward(q, kv):
    """q [N, C, H, W], kv [N, 2 C, H // 2, W // 2] (keys, then values) -> (o [N, C, H, W], lse [2, N, 4, H W]): four heads of
    C / 4 channels, softmax(q k^T (C / 4)^-0.5) v by an online softmax; lse[0] is each query's log-sum-exp of its scaled
    logits and lse[1] what rounding it to float32 dropped (the backward's probabilities would carry it)."""
    N, C, H, W = _check_attention("attention_forward", q, kv)
    o = torch.empty_like(q)
    lse = torch.empty(2, N, ATT_HEADS, H * W, dtype=torch.float32, device=q.device)
    _lib.check(_lib.load().kp2d_attention_forward_train(_ptr(q), _ptr(kv), N, C, H, W, _ptr(o), _ptr(lse), _stream(q.device)))
    return o, lse


def attention_backward(q, kv, o, lse, do):
    """-> (dq like ``q``, dkv like ``kv``).  The probabilities are formed again from q, k and ``lse``; dq is owned by query
    tiles, dk and dv by key tiles, each walking the other axis in ascending order.  Bit-reproducible."""
    N, C, H, W = _check_attention("attention_backward", q, kv, (("o", o), ("do", do)))
    if not isinstance(lse, torch.Tensor) or not _is_device(lse) or lse.dtype != torch.float32 or tuple(lse.shape) != (2, N, ATT_HEADS, H * W) \
            or not lse.is_contiguous():
        raise ValueError(f"attention_backward: lse must be a contiguous float32 device tensor {(2, N, ATT_HEADS, H * W)}")
    lib = _lib.load()
    scratch = _att_scratch(lib, N, H, W, C, C, q.device)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    _lib.check(lib.kp2d_attention_backward(_ptr(q), _ptr(kv), _ptr(o), _ptr(lse), _ptr(do), N, C, H, W, _ptr(dq), _ptr(dkv), _ptr(scratch),
                                           scratch.numel(), _stream(q.device)))
    return dq, dkv


def attention_module_parameters(module):
    """A SegFormerAttentionModule's 15 tensors in the reference's registration order (``module.parameters()``'s)."""
    att, mff = module.att, module.mff
    net = mff.fn.net
    return [att.fn.to_q.weight, att.fn.to_kv.weight, att.fn.to_out.weight, att.norm.g, att.norm.b, net[0].weight, net[0].bias,
            net[1].net[0].weight, net[1].net[0].bias, net[1].net[1].weight, net[1].net[1].bias, net[3].weight, net[3].bias, mff.norm.g,
            mff.norm.b]


def attention_module_forward(module, x):
    """One SegFormerAttentionModule (LayerNorm, to_q / to_kv, attention, to_out, LayerNorm, 1 x 1, depthwise 3 x 3, 1 x 1, GELU,
    1 x 1; no residuals) on x [N, C, H, W] -> (y, saved): the stage calls chained; ``saved`` is what the backward reads."""
    p = attention_module_parameters(module)
    s = {"x": x}
    s["n1"], s["mean1"], s["rinv1"] = layernorm_forward(x, p[3], p[4])
    s["q"] = pointwise_forward(s["n1"], p[0])[0]
    s["kv"] = patch2_forward(s["n1"], p[1])
    s["o"], s["lse"] = attention_forward(s["q"], s["kv"])
    s["a"] = pointwise_forward(s["o"], p[2])[0]
    s["n2"], s["mean2"], s["rinv2"] = layernorm_forward(s["a"], p[13], p[14])
    s["h0"] = pointwise_forward(s["n2"], p[5], p[6])[0]
    s["h1"] = dwconv3_forward(s["h0"], p[7], p[8])
    s["h2"], s["pre"] = pointwise_forward(s["h1"], p[9], p[10], gelu=True)
    y = pointwise_forward(s["h2"], p[11], p[12])[0]
    return y, s


def attention_module_backward(module, saved, dy, need_dx=True):
    """``attention_module_forward``'s ``saved`` and the gradient of its ``y`` -> (the 15 gradients in registration order, dx or
    None).  The LayerNorm's dx is the sum of the query branch's and the key/value branch's, in that order."""
    p, s = attention_module_parameters(module), saved
    g = [None] * 15
    d, g[11], g[12] = pointwise_backward(s["h2"], p[11], dy)
    d, g[9], g[10] = pointwise_backward(s["h1"], p[9], d, pre=s["pre"])
    d, g[7], g[8] = dwconv3_backward(s["h0"], p[7], d)
    d, g[5], g[6] = pointwise_backward(s["n2"], p[5], d)
    d, g[13], g[14] = layernorm_backward(s["a"], p[13], s["mean2"], s["rinv2"], d)
    d, g[2], _ = pointwise_backward(s["o"], p[2], d, need_dbias=False)
    dq, dkv = attention_backward(s["q"], s["kv"], s["o"], s["lse"], d)
    dn_q, g[0], _ = pointwise_backward(s["n1"], p[0], dq, need_dbias=False)
    dn_kv, g[1] = patch2_backward(s["n1"], p[1], dkv)
    dx, g[3], g[4] = layernorm_backward(s["x"], p[3], s["mean1"], s["rinv1"], dn_q + dn_kv)
    return g, (dx if need_dx else None)
