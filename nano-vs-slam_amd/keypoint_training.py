"""Fine-tuning the keypoint heads on the device: what the reference's ``train_multitask.py`` moves in ``score_head``,
``loc_head`` (``SimpleTaskHead``) and ``desc_head`` (``UpscaleHead``, modules/decoders/heads.py) under the keypoint block of
``KeypointNetwithIOLoss.forward`` (KeypointNetwithIOLoss.py:423-541 with ``build_descriptor_loss``, :25-154), on the HIP
kernels of csrc/keypoint_train.hip, csrc/seg_train.hip and csrc/vpr_head_train.hip (include/kp2d.h).

* ``keypoint_loss`` — the self-supervised loss over a frame (the TARGET view, the reference's ``out``) and its
  homography-warped view (the SOURCE view, ``out_aug``): location, descriptor triplet, USP and score consistency, with its
  gradient with respect to the six maps.
* ``KeypointHeadTrainer`` — forward, loss, backward and Adam for any subset of the three heads, 5 + 5 + 10 tensors in the
  reference's registration order; the layers are ``train_ops``'s ``cbr_forward`` / ``cbr_backward``, ``conv_bias_forward`` /
  ``conv_bias_backward``, ``shuffle_cat_forward`` / ``shuffle_cat_backward`` and ``adam_step``, as they are.
* ``normalized_homography`` — a pixel homography as the loss takes it.

The homography maps SOURCE points to TARGET points in normalised coordinates, as the reference's ``_warp_homography_batch``
uses ``data["homography"]``.  ``synthetic.homography_pairs`` returns ``(frames, hom, warped)`` with ``hom`` mapping the pixels
of ``frames`` to those of ``warped``: with ``frames`` as the target and ``warped`` as the source (the augmented view), the loss
takes ``normalized_homography(hom, H, W, invert=True)``.

Conventions kept from the reference: the weights (loc 1, descriptor 2 with the loss's own factor 2, score 1, keypoint 1),
``relax_field`` 4, ``cross_ratio`` 2, the 4-pixel validity radius, the triplet margin 0.2, the skip of frames with fewer than
20 interior cells, ``torch.optim.Adam``'s update, the parameters' registration order, exact fp32 arithmetic.  Frozen: the
backbone and every other head.  Deviations: the IO-net term is not built (the trainer corresponds to ``with_io = False``);
the heads run as ``.eval()`` under autograd (BatchNorm on its running statistics, which do not move, no ``Dropout2d``; the
reference trains under ``model.train()``); every argmin takes the lowest index among equal values; an anchor without an
admissible negative takes its overall nearest; a batch without a valid cell gives loc = usp = 0 (torch: NaN).

There is no CPU path: CPU tensors raise ValueError.
"""
from __future__ import annotations

import torch

from . import _dev, _lib, train_ops as _ops
from ._dev import ptr as _ptr, stream as _stream
from .train_ops import (LEAKY_SLOPE, MAX_CH, MIN_CH, AdamTrainer, adam_step, bn_vectors, cbr_backward, cbr_forward,  # noqa: F401
                        cbr_layer_backward, cbr_layer_forward, conv_bias_backward, conv_bias_forward, shuffle_cat_backward,
                        shuffle_cat_forward)

HEADS = ("score", "loc", "desc")
MAX_CELLS, MIN_FEAT, MAX_FEAT = 65536, 16, 256


def normalized_homography(hom, H, W, invert=False):
    """A homography [B, 3, 3] between PIXEL coordinates (x along the width) -> float32 [B, 3, 3] between coordinates normalised
    to [-1, 1] over [0, W - 1] x [0, H - 1]; ``invert``: of the inverse map.  Formed in float64 with torch."""
    hom = hom.to(torch.float64)
    if invert:
        hom = torch.linalg.inv(hom)
    sx, sy = (W - 1) / 2.0, (H - 1) / 2.0
    to_pix = torch.tensor([[sx, 0.0, sx], [0.0, sy, sy], [0.0, 0.0, 1.0]], dtype=torch.float64, device=hom.device)
    out = torch.linalg.inv(to_pix) @ hom @ to_pix
    return (out / out[:, 2:3, 2:3]).to(torch.float32).contiguous()


def _check_views(where, out, out_aug, homography):
    maps = []
    for view, d in (("out", out), ("out_aug", out_aug)):
        for key in ("score", "coord", "feat"):
            if not isinstance(d, dict) or key not in d or not isinstance(d[key], torch.Tensor):
                raise ValueError(f"{where}: {view} must be a dict with the tensors 'score', 'coord' and 'feat' (the model's training forward)")
            maps.append((f"{view}['{key}']", d[key]))
    _ops._f32_maps(where, tuple(maps))
    score, shift, feat = out["score"], out["coord"], out["feat"]
    B, _, Hc, Wc = score.shape
    C, Hf, Wf = feat.shape[1:]
    for view, d in (("out", out), ("out_aug", out_aug)):
        if tuple(d["score"].shape) != (B, 1, Hc, Wc) or tuple(d["coord"].shape) != (B, 2, Hc, Wc) or tuple(d["feat"].shape) != (B, C, Hf, Wf):
            raise ValueError(f"{where}: {view} must hold score [B, 1, Hc, Wc], coord [B, 2, Hc, Wc] and feat [B, C, Hf, Wf] with the "
                             f"other view's sizes, got {tuple(d['score'].shape)}, {tuple(d['coord'].shape)}, {tuple(d['feat'].shape)}")
    _check_homography(where, homography, B, score.device)
    return B, Hc, Wc, C, Hf, Wf


def _check_homography(where, homography, B, device):
    if not isinstance(homography, torch.Tensor) or not _ops._is_device(homography):
        raise ValueError(f"{where}: homography must be a device tensor (there is no CPU path)")
    if homography.dtype != torch.float32 or tuple(homography.shape) != (B, 3, 3):
        raise ValueError(f"{where}: homography must be float32 [{B}, 3, 3] in normalised coordinates, source to target "
                         f"(normalized_homography), got {homography.dtype} {tuple(homography.shape)}")
    if homography.device != device:
        raise ValueError(f"{where}: homography and the maps must live on one device")


def keypoint_loss(out, out_aug, homography, size, cell, loc_weight=1.0, descriptor_weight=2.0, score_weight=1.0, keypoint_weight=1.0,
                  relax_field=4, cross_ratio=2.0, scratch=None, return_parts=False):
    """``out`` (the target view: the plain frame) and ``out_aug`` (the source view: the augmented frame), each the dict of the
    model's training forward (``score`` [B,1,Hc,Wc] after the sigmoid, ``coord`` [B,2,Hc,Wc]: the shift after the tanh,
    ``feat`` [B,C,Hf,Wf] raw), ``homography`` float32 [B,3,3] in normalised coordinates, source to target, ``size`` = (H, W)
    of the frames -> (loss, grads, stats): the device scalar
    ``keypoint_weight (loc_weight loc + descriptor_weight 2 metric + score_weight usp + score_weight con)`` (formulas:
    include/kp2d.h), ``grads = {"out": {...}, "out_aug": {...}}`` with the gradient of every map under its key, and
    ``stats = {"valid": M, "anchors": n, "hits": ..., "recall": ...}`` (int64 device scalars; recall a float32 device
    scalar; anchors is 0 when the descriptor term was skipped: fewer than 20 interior cells).  ``return_parts=True`` adds
    ``stats["parts"]``, the float32 device tensor [loc, metric, usp, con], unweighted.  No host synchronisation."""
    where = "keypoint_loss"
    B, Hc, Wc, C, Hf, Wf = _check_views(where, out, out_aug, homography)
    H, W = (int(v) for v in size)
    cell = int(cell)
    weights = tuple(float(v) for v in (cross_ratio, relax_field, loc_weight, descriptor_weight, score_weight, keypoint_weight))
    if not all(0.0 <= v < float("inf") for v in weights):
        raise ValueError(f"{where}: cross_ratio, relax_field and the weights must be finite and >= 0, got {weights}")
    if H < 2 or W < 2 or cell < 1:
        raise ValueError(f"{where}: needs size (H, W) >= 2 and cell >= 1, got {(H, W)}, cell {cell}")
    if not (1 <= B <= 65535 and Hc * Wc <= MAX_CELLS and C % 16 == 0 and MIN_FEAT <= C <= MAX_FEAT):
        raise ValueError(f"{where}: needs 1 <= B <= 65535, Hc * Wc <= {MAX_CELLS} and feat channels a multiple of 16 in "
                         f"[{MIN_FEAT}, {MAX_FEAT}], got B {B}, cells {Hc} x {Wc}, C {C}")
    lib = _lib.load()
    dev = out["score"].device
    if scratch is None:
        nbytes = int(lib.kp2d_keypoint_loss_scratch_bytes(B, Hc, Wc, C, Hf, Wf))
        if nbytes == 0:
            raise ValueError(f"{where}: maps of {Hc} x {Wc} cells with feat {tuple(out['feat'].shape)} are not supported")
        scratch = _dev.scratch(nbytes, dev)
    t = [out[k].contiguous() for k in ("score", "coord", "feat")]
    s = [out_aug[k].contiguous() for k in ("score", "coord", "feat")]
    hom = homography.contiguous()
    res = torch.empty(5, dtype=torch.float32, device=dev)          # loss, loc, metric, usp, con
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    gt, gs = [torch.empty_like(v) for v in t], [torch.empty_like(v) for v in s]
    _lib.check(lib.kp2d_keypoint_loss(_ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _ptr(s[0]), _ptr(s[1]), _ptr(s[2]), _ptr(hom), B, Hc, Wc, C, Hf, Wf,
                                      H, W, cell, *weights, _ptr(res[0:1]), _ptr(res[1:5]), _ptr(gt[0]), _ptr(gt[1]), _ptr(gt[2]),
                                      _ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), _ptr(counts), _ptr(scratch), scratch.numel(), _stream(dev)))
    n = max(Hc - 2, 0) * max(Wc - 2, 0)
    stats = {"valid": counts[0], "anchors": counts[1], "hits": counts[2], "recall": counts[2].to(torch.float32) / float(max(B * n, 1))}
    if return_parts:
        stats["parts"] = res[1:5]
    grads = {"out": dict(zip(("score", "coord", "feat"), gt)), "out_aug": dict(zip(("score", "coord", "feat"), gs))}
    return res[0], grads, stats


def _check_model(model, train):
    """The refusals that need no device -> the chosen heads in HEADS order."""
    who = "KeypointHeadTrainer"
    train = (train,) if isinstance(train, str) else tuple(train)
    if not train or any(h not in HEADS for h in train) or len(set(train)) != len(train):
        raise ValueError(f"{who}: train must be a non-empty subset of {HEADS}, got {train!r}")
    if getattr(model, "_version_id", 2) != 2 or not all(hasattr(model, a) for a in ("score_head", "loc_head", "desc_head")):
        raise ValueError(f"{who}: V3 models are not supported: score and location share the merged score_loc_head and the "
                         "descriptor is a branch of the segmentation trunk")
    if getattr(model, "upscale_method", "pixelshuffle") != "pixelshuffle" or hasattr(model.desc_head, "upsample"):
        raise ValueError(f"{who}: upscale_method='convtranspose' (to_mcu) is not supported: only pixel shuffle has a backward")

    def channels(name, layers):
        for label, conv, last in layers:
            co, ci = conv.weight.shape[:2]
            if ci % 16 or not MIN_CH <= ci <= MAX_CH or not 1 <= co <= MAX_CH or (not last and co % 16):
                raise ValueError(f"{who}: {name}.{label} has channel counts {ci} -> {co}, which the conv kernels do not take "
                                 f"(Cin % 16 == 0, {MIN_CH} <= Cin <= {MAX_CH}; Cout % 16 == 0 before a BatchNorm); "
                                 f"leave {name.split('_')[0]!r} out of train")

    if "score" in train:
        channels("score_head", (("convDa", model.score_head.convDa.conv, False), ("convDb", model.score_head.convDb, True)))
    if "loc" in train:
        channels("loc_head", (("convDa", model.loc_head.convDa.conv, False), ("convDb", model.loc_head.convDb, True)))
    if "desc" in train:
        d = model.desc_head
        channels("desc_head", (("convA", d.convA.conv, False), ("convB", d.convB, True), ("confAa", d.confAa.conv, False), ("confBb", d.confBb, True)))
        nfeat = d.confBb.weight.shape[0]
        if d.convB.weight.shape[0] % 4 or nfeat % 16 or not MIN_FEAT <= nfeat <= MAX_FEAT:
            raise ValueError(f"{who}: desc_head's channel counts (convB {d.convB.weight.shape[0]}, nfeatures {nfeat}) are not supported: "
                             f"the shuffle needs a multiple of 4, the loss a multiple of 16 in [{MIN_FEAT}, {MAX_FEAT}]")
    return tuple(h for h in HEADS if h in train)


class KeypointHeadTrainer(AdamTrainer):
    """Adam on ``model.score_head``, ``model.loc_head`` and ``model.desc_head`` under the reference's keypoint loss, on a
    frozen backbone.

        trainer = KeypointHeadTrainer(model, lr=1e-4, train=("score", "loc", "desc"))
        loss = trainer.step(frames, frames_aug, homography)      # frames [B, 3, H, W]; homography float32 [B, 3, 3], normalised
        loss = trainer.step_features(model.backbone_maps(frames), model.backbone_maps(frames_aug), homography, (H, W))
        outs = trainer.forward_features(x, skip)                 # {"score", "coord", "feat"} as the model's training forward

    ``frames`` are the target view, ``frames_aug`` the source view; ``homography`` maps source to target (see the module's
    docstring for ``synthetic.homography_pairs``).  Both views go through the heads as one batch of 2 B.  ``train``: any subset
    of the three heads; their parameters in the reference's registration order (``parameters()``): ``convDa.conv.weight``,
    ``convDa.bn.weight``, ``convDa.bn.bias``, ``convDb.weight``, ``convDb.bias`` per SimpleTaskHead, ``convA.*``, ``convB.*``,
    ``confAa.*``, ``confBb.*`` of the UpscaleHead.  A head outside ``train`` still runs forward (the loss needs its map) and
    keeps every bit.  BatchNorm runs on its running statistics, which stay as they are, and there is no dropout.  After a
    step ``parts`` (float32 [loc, metric, usp, con], unweighted), ``recall`` and ``valid`` describe it, and every updated
    parameter's version counter is bumped, so the engine re-packs its weights on its next call.  V3 models, ``to_mcu``
    models, a chosen head whose channel counts the conv kernels do not take (config N's 72-channel concatenation: "desc"),
    CPU tensors, non-contiguous parameters and a homography that is not float32 [B, 3, 3] raise ValueError."""

    _WHO = "KeypointHeadTrainer"

    def __init__(self, model, lr=1e-4, train=HEADS, loc_weight=1.0, descriptor_weight=2.0, score_weight=1.0, keypoint_weight=1.0,
                 relax_field=4, betas=(0.9, 0.999), eps=1e-8):
        self.train = _check_model(model, train)
        self._init_adam(lr, betas, eps)
        self.weights = tuple(float(v) for v in (loc_weight, descriptor_weight, score_weight, keypoint_weight))
        if not all(0 <= v < float("inf") for v in self.weights + (float(relax_field),)):
            raise ValueError(f"KeypointHeadTrainer: the weights {self.weights} and relax_field {relax_field} must be finite and >= 0")
        self.model, self.relax_field = model, relax_field
        self.slope = LEAKY_SLOPE if getattr(model, "leaky_relu", True) else 0.0
        self.parts = self.recall = self.valid = None

    @staticmethod
    def _simple(head):
        return [head.convDa.conv.weight, head.convDa.bn.weight, head.convDa.bn.bias, head.convDb.weight, head.convDb.bias]

    def parameters(self):
        """The trained parameters in the reference's registration order: 5 per SimpleTaskHead, 10 of the UpscaleHead."""
        m, out = self.model, []
        if "score" in self.train:
            out += self._simple(m.score_head)
        if "loc" in self.train:
            out += self._simple(m.loc_head)
        if "desc" in self.train:
            d = m.desc_head
            out += [d.convA.conv.weight, d.convA.bn.weight, d.convA.bn.bias, d.convB.weight, d.convB.bias,
                    d.confAa.conv.weight, d.confAa.bn.weight, d.confAa.bn.bias, d.confBb.weight, d.confBb.bias]
        return out

    def _check_maps(self, x, skip):
        who = "KeypointHeadTrainer"
        _ops._f32_maps(who, (("x", x), ("skip", skip)))
        c4 = self.model.score_head.convDa.conv.weight.shape[1]
        c_skip = self.model.desc_head.confAa.conv.weight.shape[1] - self.model.desc_head.convB.weight.shape[0] // 4
        N, _, H, W = x.shape
        if x.shape[1] != c4 or tuple(skip.shape) != (N, c_skip, 2 * H, 2 * W):
            raise ValueError(f"{who}: needs x [N, {c4}, Hc, Wc] and skip [N, {c_skip}, 2 Hc, 2 Wc] (model.backbone_maps), got "
                             f"{tuple(x.shape)}, {tuple(skip.shape)}")

    def _forward(self, x, skip):
        m = self.model
        x, skip = x.contiguous(), skip.contiguous()
        a = {"score": cbr_layer_forward(m.score_head.convDa, x, self.slope), "loc": cbr_layer_forward(m.loc_head.convDa, x, self.slope),
             "descA": cbr_layer_forward(m.desc_head.convA, x, self.slope)}
        score = torch.sigmoid(conv_bias_forward(a["score"][1], m.score_head.convDb.weight, m.score_head.convDb.bias))
        shift = torch.tanh(conv_bias_forward(a["loc"][1], m.loc_head.convDb.weight, m.loc_head.convDb.bias))
        up = conv_bias_forward(a["descA"][1], m.desc_head.convB.weight, m.desc_head.convB.bias)
        a["descAa"] = cbr_layer_forward(m.desc_head.confAa, shuffle_cat_forward(up, skip), self.slope)
        feat = conv_bias_forward(a["descAa"][1], m.desc_head.confBb.weight, m.desc_head.confBb.bias)
        return {"score": score, "coord": shift, "feat": feat}, a

    def forward_features(self, x, skip):
        """The three heads' training forward on the backbone's two maps -> {"score", "coord", "feat"}: the score after the
        sigmoid, the shift after the tanh, the raw descriptor map."""
        self._check_maps(x, skip)
        return self._forward(x, skip)[0]

    def gradients(self, maps, maps_aug, homography, size):
        """One forward, loss and backward without an update -> (loss, outs of the 2 B frames (target view first), the gradients
        in ``parameters()`` order)."""
        who = "KeypointHeadTrainer"
        for pair in (maps, maps_aug):
            if not isinstance(pair, (tuple, list)) or len(pair) != 2:
                raise ValueError(f"{who}: pass each view's (x, skip) as model.backbone_maps returns them")
        self._check_maps(*maps)
        self._check_maps(*maps_aug)
        if tuple(maps[0].shape) != tuple(maps_aug[0].shape) or maps[0].device != maps_aug[0].device:
            raise ValueError(f"{who}: both views must have one size and one device, got {tuple(maps[0].shape)}, {tuple(maps_aug[0].shape)}")
        B = maps[0].shape[0]
        _check_homography(who, homography, B, maps[0].device)
        self._check_contiguous(self.parameters(), "the heads'")
        m = self.model
        outs, a = self._forward(torch.cat([maps[0], maps_aug[0]]), torch.cat([maps[1], maps_aug[1]]))
        loss, g, stats = keypoint_loss({k: v[:B] for k, v in outs.items()}, {k: v[B:] for k, v in outs.items()}, homography, size, m.cell,
                                       *self.weights, relax_field=self.relax_field, cross_ratio=m.cross_ratio, return_parts=True)
        self.parts, self.recall, self.valid = stats["parts"], stats["recall"], stats["valid"]
        grads = []

        def simple(head, saved, dz):
            dw, db, dy = conv_bias_backward(saved[1], head.convDb.weight, dz)
            return list(cbr_layer_backward(head.convDa, saved, dy, self.slope, need_dx=False)[:3]) + [dw, db]

        if "score" in self.train:       # the sigmoid's and the tanh's derivative: torch element-wise operations
            dz = torch.cat([g["out"]["score"], g["out_aug"]["score"]]) * outs["score"] * (1.0 - outs["score"])
            grads += simple(m.score_head, a["score"], dz)
        if "loc" in self.train:
            dz = torch.cat([g["out"]["coord"], g["out_aug"]["coord"]]) * (1.0 - outs["coord"] * outs["coord"])
            grads += simple(m.loc_head, a["loc"], dz)
        if "desc" in self.train:
            d = m.desc_head
            dw2, db2, dy = conv_bias_backward(a["descAa"][1], d.confBb.weight, torch.cat([g["out"]["feat"], g["out_aug"]["feat"]]))
            ga = cbr_layer_backward(d.confAa, a["descAa"], dy, self.slope)
            dup = shuffle_cat_backward(ga[3], d.convB.weight.shape[0] // 4)
            dw1, db1, dy = conv_bias_backward(a["descA"][1], d.convB.weight, dup)
            grads += list(cbr_layer_backward(d.convA, a["descA"], dy, self.slope, need_dx=False)[:3]) + [dw1, db1] + list(ga[:3]) + [dw2, db2]
        return loss, outs, grads

    def step_features(self, maps, maps_aug, homography, size):
        """``model.backbone_maps`` of the target frames and of the source frames, the homography and the frames' (H, W) -> the
        loss before the update, a device scalar."""
        loss, _, grads = self.gradients(maps, maps_aug, homography, size)
        self._apply(self.parameters(), grads)
        return loss

    def step(self, frames, frames_aug, homography):
        """Target frames and source frames [B, 3, H, W] and the homography -> the loss before the update.  Runs the frozen
        backbone through ``model.backbone_maps`` for each view."""
        for name, t in (("frames", frames), ("frames_aug", frames_aug)):
            if not isinstance(t, torch.Tensor) or not _ops._is_device(t):
                raise ValueError(f"KeypointHeadTrainer.step: {name} must be a device tensor (there is no CPU path)")
        if tuple(frames.shape) != tuple(frames_aug.shape):
            raise ValueError(f"KeypointHeadTrainer.step: both views must have one size, got {tuple(frames.shape)}, {tuple(frames_aug.shape)}")
        with torch.no_grad():
            maps, maps_aug = self.model.backbone_maps(frames), self.model.backbone_maps(frames_aug)
        return self.step_features(maps, maps_aug, homography, (frames.shape[2], frames.shape[3]))
