"""Fine-tuning the V2 attention segmentation and depth heads on the device: what the reference's ``train_multitask.py
--freeze_backbone`` moves in a ``SegmentationHeadATT`` (modules/decoders/segmentation.py:350-475), on the HIP kernels of
csrc/attention_train.hip beside those of the non-attention trainers (include/kp2d.h).

* ``AttentionSegHeadTrainer`` — ``seg_training.SegHeadTrainer`` on ``model.seg_head`` of a ``use_attention`` model.
* ``AttentionDepthHeadTrainer`` — ``depth_training.DepthHeadTrainer`` on ``model.depth_head`` of one, the pair step included.

``train="head"`` moves all 47 tensors of the head in the reference's registration order: ``convs.0`` (conv.weight, bn.weight,
bn.bias), the 15 tensors of each ``SegFormerAttentionModule`` ``convs.1`` and ``convs.2`` (``att.fn.to_q.weight``,
``att.fn.to_kv.weight``, ``att.fn.to_out.weight``, ``att.norm.g``, ``att.norm.b``, ``mff.fn.net.0.weight``, ``.bias``,
``mff.fn.net.1.net.0.weight``, ``.bias``, ``mff.fn.net.1.net.1.weight``, ``.bias``, ``mff.fn.net.3.weight``, ``.bias``,
``mff.norm.g``, ``mff.norm.b``), ``convs.3`` ... ``convs.6`` and ``convs.7.weight``, ``.bias``.  ``train="last"`` is the last layer
alone, as in the other trainers.  The walk is ``seg_training._DenseHeadTrainer``'s attention branch: convs[0], module, pool,
module, convs[3], shuffle + cat with x, convs[4], convs[5], shuffle + cat with skip, convs[6], convs[7]; the modules run through
``train_ops.attention_module_forward`` / ``attention_module_backward``.

Loss, Adam, the version-counter bump and ``valid`` / ``stray`` / ``parts`` are the other trainers'.  Deviation, as there: the
head runs as ``.eval()`` under autograd (BatchNorm on its running statistics, no ``Dropout2d``).  Refused with ValueError:
non-attention models (``SegHeadTrainer`` / ``DepthHeadTrainer`` take those), V3 models, ``to_mcu`` models, odd backbone maps,
backbone maps under 4 x 4 (the pooled map needs one 2 x 2 key patch), channel counts the conv kernels do not take (config N_A:
its 72-channel concatenation), CPU tensors and non-contiguous parameters.

There is no CPU path: CPU tensors raise ValueError.
"""
from __future__ import annotations

from .depth_training import DepthHeadTrainer
from .seg_training import SegHeadTrainer


class AttentionSegHeadTrainer(SegHeadTrainer):
    """Adam on the attention ``model.seg_head`` under the reference's segmentation loss, on a frozen backbone.

        trainer = AttentionSegHeadTrainer(model, lr=1e-4, train="head", ce_weight=0.5, dice_weight=1.5, ignore_index=255)
        loss = trainer.step(frames, labels)
        loss = trainer.step_features(x, skip, labels)
        logits = trainer.forward_features(x, skip)
    """

    _WHO, _ATTENTION = "AttentionSegHeadTrainer", True


class AttentionDepthHeadTrainer(DepthHeadTrainer):
    """Adam on the attention ``model.depth_head`` under the reference's depth loss; ``step``, ``step_features``, ``step_pair``,
    ``step_pair_features`` and ``pair_gradients`` as on ``DepthHeadTrainer``."""

    _WHO, _ATTENTION = "AttentionDepthHeadTrainer", True
