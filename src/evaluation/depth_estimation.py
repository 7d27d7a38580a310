"""Alias so the reference's import line keeps working (eval_multitask.py:19, ./src on sys.path):

    from evaluation.depth_estimation import evaluate_depth_estimation

It resolves to the device implementation in ``nano-vs-slam_amd/dense_metrics.py`` (kp2d_depth_sums; this module imports
neither tqdm nor cv2).
"""
import os as _os
import sys as _sys

_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.insert(0, _root)

from nano_vs_slam_amd.dense_metrics import compute_errors_torch, depth_sums, evaluate_depth_estimation  # noqa: E402,F401
