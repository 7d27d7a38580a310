"""Fine-tuning the NetVLAD layer on the device: the gradient step of the reference's place-recognition training
(train_visloc.py:249-282) on the HIP kernels of csrc/vlad_train.hip (kp2d_vlad_forward_train, kp2d_triplet_loss,
kp2d_vlad_backward, kp2d_adam_step; include/kp2d.h).

* ``netvlad_forward`` / ``triplet_margin_loss`` / ``netvlad_backward`` / ``adam_step`` — the four calls on device tensors;
  ``adam_step`` and the trainers' Adam core (``AdamTrainer``) live in ``train_ops`` and are imported here.
* ``NetVLADTrainer`` — forward, loss, backward and Adam for ``vlad_head.netvlad.conv.weight`` and
  ``vlad_head.netvlad.centroids`` of a KP2DTiny model; the step's own calls make no host synchronisation.
* ``hard_triplet_loss`` / ``HardTripletLoss`` / ``view_labels`` — the multitask run's ``vlad`` term, the reference's
  batch-hard triplet loss on labelled embeddings with its gradient (csrc/hard_triplet.hip, kp2d_hard_triplet_loss; defined in
  ``train_ops`` beside ``adam_step``, since ``VPRHeadTrainer`` steps on it too), and ``NetVLADTrainer.step_views``, the step that
  feeds it a batch of view pairs.

Conventions kept from the reference: ``TripletMarginLoss(margin ** 0.5, p=2, reduction="sum")`` divided by the number of
negatives, rows ordered queries, positives, negatives in query order, ``torch.optim.Adam``'s update.  Stated deviation: only
the NetVLAD layer is trained; the backbone and ``convlad1..3`` are frozen and run with inference semantics (running
BatchNorm statistics, no dropout) through ``model.only_encoder``, where the reference trains every head that requires
grad with BatchNorm and Dropout2d in training mode.

There is no CPU path: CPU tensors raise, like the rest of the product.
"""
from __future__ import annotations

import torch

from . import _dev, _lib
from ._dev import ptr as _ptr, stream as _stream
from .train_ops import AdamTrainer, adam_step  # noqa: F401  (adam_step: this module's fourth call, as it always was)
from .train_ops import MAX_HT_ROWS, QUIRK_MARGIN, HardTripletLoss, _views_loss, hard_triplet_loss, view_labels  # noqa: F401  (the
#                       view loss: both place-recognition trainers step on it, so it lives with what the trainers share)

MAX_KC = 8192


def _check_layer(enc, weight, centroids):
    """-> (enc [N, C, S] view, weight [K, C] view, N, S, C, K); placement first, then shapes: all before any library call."""
    for name, t in (("enc", enc), ("weight", weight), ("centroids", centroids)):
        _dev.require_device(f"vlad_training: {name}", t)
    if enc.dim() not in (3, 4) or enc.dtype != torch.float32:
        raise ValueError(f"enc must be float32 [N, C, Hc, Wc] or [N, C, S], got {enc.dtype} {tuple(enc.shape)}")
    if centroids.dim() != 2 or centroids.dtype != torch.float32 or weight.dtype != torch.float32:
        raise ValueError("weight [K, C, 1, 1] and centroids [K, C] must be float32")
    K, C = centroids.shape
    if tuple(weight.shape) not in ((K, C), (K, C, 1, 1)):
        raise ValueError(f"weight must be [{K}, {C}, 1, 1], got {tuple(weight.shape)}")
    N = enc.shape[0]
    S = enc[0, 0].numel() if N and enc.shape[1] else 0
    if enc.shape[1] != C or N < 1 or S < 1:
        raise ValueError(f"enc must be [N >= 1, {C}, S >= 1], got {tuple(enc.shape)}")
    if K % 4 or C % 4 or K < 4 or K > 64 or K * C > MAX_KC:
        raise ValueError(f"NetVLAD training needs K % 4 == 0, C % 4 == 0, 4 <= K <= 64 and K * C <= {MAX_KC} (got K {K}, C {C})")
    if not (enc.device == weight.device == centroids.device):
        raise ValueError("enc, weight and centroids must live on one device")
    return enc.contiguous().view(N, C, S), weight.detach().contiguous().view(K, C), N, S, C, K


def _scratch(lib, N, S, C, K, dev):
    nbytes = int(lib.kp2d_vlad_train_scratch_bytes(N, S, C, K))
    if nbytes == 0:
        raise ValueError(f"NetVLAD training does not support N {N}, S {S}, C {C}, K {K}")
    return _dev.scratch(nbytes, dev)


def netvlad_forward(enc, weight, centroids, scratch=None):
    """enc [N, C, Hc, Wc] (``model.only_encoder``'s map), weight [K, C, 1, 1], centroids [K, C] ->
    (vlad [N, K C], saved [N, K C + 2 K + 4]): the model's own ``vlad`` output in fp32 arithmetic, and per frame the
    intra-normalised V, the row norms n, the assignment sums r and the global norm g that ``netvlad_backward`` reads."""
    x, w, N, S, C, K = _check_layer(enc, weight, centroids)
    cent = centroids.detach().contiguous()
    lib = _lib.load()
    scratch = _scratch(lib, N, S, C, K, x.device) if scratch is None else scratch
    vlad = torch.empty(N, K * C, dtype=torch.float32, device=x.device)
    saved = torch.empty(N, K * C + 2 * K + 4, dtype=torch.float32, device=x.device)
    _lib.check(lib.kp2d_vlad_forward_train(_ptr(x), _ptr(w), _ptr(cent), N, S, C, K, _ptr(vlad), _ptr(saved), _ptr(scratch),
                                           scratch.numel(), _stream(x.device)))
    return vlad, saved


def _neg_offsets(neg_counts, B, dev):
    """-> (offsets [B + 1] int32 on ``dev``, the sum when it is known on the host else None).  Built with torch."""
    if isinstance(neg_counts, torch.Tensor):
        if neg_counts.dim() != 1 or neg_counts.numel() != B or neg_counts.is_floating_point():
            raise ValueError(f"neg_counts must hold {B} integers")
        total = None                  # a device tensor is not read back: it is trusted
        if neg_counts.device.type == "cpu":
            if B and int(neg_counts.min()) < 0:
                raise ValueError(f"neg_counts must hold {B} non-negative integers")
            total = int(neg_counts.sum())
        cnt = neg_counts.to(dev, torch.int32)
    else:
        host = [int(c) for c in neg_counts]
        if len(host) != B or any(c < 0 for c in host):
            raise ValueError(f"neg_counts must hold {B} non-negative integers")
        total = sum(host)
        cnt = torch.tensor(host, dtype=torch.int32).to(dev, non_blocking=True)
    off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    off[1:] = torch.cumsum(cnt, 0)
    return off, total


def triplet_margin_loss(vlad, B, neg_counts, margin=0.1, scratch=None):
    """vlad [2 B + n_neg, dim] with rows (queries, positives, negatives in query order), ``neg_counts`` the negatives per
    query (a host sequence or a tensor; a device tensor is trusted to sum to the rows there are) ->
    (loss [] , dvlad like vlad, n_active [] int32).  ``margin`` is the reference's squared margin: the hinge uses
    margin ** 0.5; distances are torch's pairwise_distance (eps 1e-6 added to the difference); the sum is divided by the
    number of negatives.  No negatives at all: loss 0 and zero gradients."""
    _dev.require_device("triplet_margin_loss: vlad", vlad)
    B = int(B)
    if vlad.dim() != 2 or vlad.dtype != torch.float32 or B < 1 or vlad.shape[0] < 2 * B or vlad.shape[1] < 1:
        raise ValueError(f"vlad must be float32 [2 B + n_neg, dim] with B = {B}, got {vlad.dtype} {tuple(vlad.shape)}")
    if not margin >= 0:
        raise ValueError(f"margin must be >= 0, got {margin}")
    vlad = vlad.detach().contiguous()
    n_neg = vlad.shape[0] - 2 * B
    off, total = _neg_offsets(neg_counts, B, vlad.device)
    if total is not None and total != n_neg:
        raise ValueError(f"neg_counts sum to {total} but vlad has {n_neg} negative rows")
    lib = _lib.load()
    dev = vlad.device
    scratch = _dev.scratch(4 * (B + n_neg), dev) if scratch is None else scratch
    loss = torch.empty((), dtype=torch.float32, device=dev)
    n_active = torch.empty((), dtype=torch.int32, device=dev)
    dvlad = torch.empty_like(vlad)
    _lib.check(lib.kp2d_triplet_loss(_ptr(vlad), B, _ptr(off), n_neg, vlad.shape[1], float(margin), _ptr(loss), _ptr(dvlad),
                                     _ptr(n_active), _ptr(scratch), scratch.numel(), _stream(dev)))
    return loss, dvlad, n_active


def netvlad_backward(enc, weight, centroids, saved, dvlad, scratch=None):
    """The gradients of a scalar with respect to weight and centroids given its gradient ``dvlad`` [N, K C] with respect to
    ``netvlad_forward``'s output, whose ``saved`` this takes -> (dW [K, C, 1, 1], dcent [K, C]).  Bit-reproducible: sums
    over pixels in tile order, then over frames in frame order."""
    x, w, N, S, C, K = _check_layer(enc, weight, centroids)
    for name, t, shape in (("saved", saved, (N, K * C + 2 * K + 4)), ("dvlad", dvlad, (N, K * C))):
        _dev.require_device(f"netvlad_backward: {name}", t)
        if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != x.device:
            raise ValueError(f"{name} must be float32 {shape} on {x.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    cent = centroids.detach().contiguous()
    lib = _lib.load()
    scratch = _scratch(lib, N, S, C, K, x.device) if scratch is None else scratch
    dW = torch.empty(K, C, 1, 1, dtype=torch.float32, device=x.device)
    dcent = torch.empty(K, C, dtype=torch.float32, device=x.device)
    _lib.check(lib.kp2d_vlad_backward(_ptr(x), _ptr(w), _ptr(cent), _ptr(saved.contiguous()), _ptr(dvlad.contiguous()), N, S, C, K,
                                      _ptr(dW), _ptr(dcent), _ptr(scratch), scratch.numel(), _stream(x.device)))
    return dW, dcent


class NetVLADTrainer(AdamTrainer):
    """Adam on the NetVLAD layer of ``model`` under the reference's triplet loss.

        trainer = NetVLADTrainer(model, lr=1e-4, margin=0.1)
        loss = trainer.step(query, positives, negatives, neg_counts)      # frames [., 3, H, W]; loss: a device scalar

    ``step`` runs ``model.only_encoder`` on the concatenated frames (frozen, inference semantics), then forward, loss,
    backward and Adam on the device, and updates the two ``nn.Parameter`` s in place; the trainer's own calls make no host
    synchronisation and the loss stays on the device.  The model's next forward uses the new weights: the parameters'
    version counters are bumped, so the engine re-packs its weights on its next call — its ordinary upload path, which goes
    through the host.  ``only_encoder`` is such a call, so a loop over ``step`` pays that upload once per step; the encoder
    being frozen, a loop over ``step_encoded`` on encoder maps computed once does not.
    ``step_views(frames, frames_aug)`` is the multitask run's step on a batch of view pairs (``augment.view_pair``): the
    batch-hard triplet loss on (plain views, augmented views) with ``view_labels``; ``ht_stats`` holds its ``stats``.
    GeM / ConvAP poolers and ``remove_netvlad`` models raise ValueError."""

    _WHO = "NetVLADTrainer"

    def __init__(self, model, lr=1e-4, margin=0.1, betas=(0.9, 0.999), eps=1e-8):
        if getattr(model, "global_descriptor_method", None) != "netvlad":
            raise ValueError(f"NetVLADTrainer needs a NetVLAD pooler, the model has {getattr(model, 'global_descriptor_method', None)!r}")
        if getattr(model, "remove_netvlad", False) or not hasattr(model.vlad_head, "netvlad"):
            raise ValueError("NetVLADTrainer: the model was built with remove_netvlad")
        self._init_adam(lr, betas, eps, margin)
        self.model = model
        self.n_active = None          # device int32 scalar of the last step
        self.ht_stats = None          # device int64 [4] of the last view step

    @property
    def layer(self):
        return self.model.vlad_head.netvlad

    def step(self, query, positives, negatives, neg_counts):
        """Frames [B, 3, H, W], [B, 3, H, W], [n_neg, 3, H, W] and the negatives per query -> the loss before the update."""
        for name, t in (("query", query), ("positives", positives), ("negatives", negatives)):
            _dev.require_device(f"NetVLADTrainer.step: {name}", t)
        if query.dim() != 4 or positives.shape != query.shape or negatives.dim() != 4 or negatives.shape[1:] != query.shape[1:]:
            raise ValueError("query and positives must be [B, 3, H, W], negatives [n_neg, 3, H, W]")
        with torch.no_grad():
            enc = self.model.only_encoder(torch.cat([query, positives, negatives]))
        return self.step_encoded(enc, query.shape[0], neg_counts)

    def step_encoded(self, enc, B, neg_counts):
        """``enc`` = ``model.only_encoder`` of (queries, positives, negatives) -> the loss before the update."""
        def loss_fn(vlad, scratch):
            loss, dvlad, self.n_active = triplet_margin_loss(vlad, B, neg_counts, self.margin, scratch)
            return loss, dvlad
        return self._step_layer(enc, loss_fn)

    def _step_layer(self, enc, loss_fn):
        """The layer's forward on ``enc``, ``loss_fn(vlad, scratch) -> (loss, dvlad)``, backward and one Adam step."""
        weight, cent = self.layer.conv.weight, self.layer.centroids
        x, w, N, S, C, K = _check_layer(enc, weight, cent)
        self._check_contiguous((weight, cent), "the layer's")
        lib = _lib.load()
        scratch = _scratch(lib, N, S, C, K, x.device)
        vlad, saved = netvlad_forward(x, w, cent, scratch)
        loss, dvlad = loss_fn(vlad, scratch)
        dW, dcent = netvlad_backward(x, w, cent, saved, dvlad, scratch)
        self._apply((weight, cent), (dW, dcent))
        return loss

    def step_views(self, frames, frames_aug, margin=0.1, weight=1.0):
        """A batch of view pairs, frames and frames_aug [N, 3, H, W] -> the loss before the update:
        ``weight * hard_triplet_loss(cat(vlad, vlad_aug), view_labels(N), margin, hardest=True)``."""
        for name, t in (("frames", frames), ("frames_aug", frames_aug)):
            _dev.require_device(f"NetVLADTrainer.step_views: {name}", t)
        if frames.dim() != 4 or frames_aug.shape != frames.shape:
            raise ValueError("frames and frames_aug must both be [N, 3, H, W]")
        with torch.no_grad():
            enc = self.model.only_encoder(torch.cat([frames, frames_aug]))
        N = frames.shape[0]
        return self.step_views_encoded(enc[:N], enc[N:], margin, weight)

    def step_views_encoded(self, enc, enc_aug, margin=0.1, weight=1.0):
        """``enc``, ``enc_aug`` = ``model.only_encoder`` of the plain and of the augmented views -> the loss before the update."""
        for name, t in (("enc", enc), ("enc_aug", enc_aug)):
            _dev.require_device(f"NetVLADTrainer.step_views_encoded: {name}", t)
        if enc.dim() != 4 or enc_aug.shape != enc.shape or enc.dtype != torch.float32 or enc_aug.dtype != torch.float32:
            raise ValueError("enc and enc_aug must both be float32 [N, C, Hc, Wc]")
        return self._step_layer(torch.cat([enc, enc_aug]), _views_loss(self, enc.shape[0], margin, weight))
