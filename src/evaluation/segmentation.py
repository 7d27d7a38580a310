"""Alias so the reference's import line keeps working (eval_multitask.py:18, ./src on sys.path):

    from evaluation.segmentation import evaluate_segmentation

It resolves to the device implementation in ``nano-vs-slam_amd/dense_metrics.py`` (kp2d_seg_stats in place of
segmentation_models_pytorch; this module imports neither smp nor tqdm nor cv2).
"""
import os as _os
import sys as _sys

_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.insert(0, _root)

from nano_vs_slam_amd.dense_metrics import (accuracy, confusion_matrix, evaluate_segmentation, f1_score, get_stats,  # noqa: E402,F401
                                            iou_score)
