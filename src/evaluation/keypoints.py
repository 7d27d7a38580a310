"""Alias so the reference's import line keeps working (eval_multitask.py:18, ./src on sys.path):

    from evaluation.keypoints import evaluate_keypoint_net

It resolves to the device implementation in ``nano-vs-slam_amd/keypoint_metrics.py`` (score, coordinate and descriptor maps
stay on the device; this module imports neither cv2 nor tqdm).  The correctness and AUC values, which rest on the RANSAC
homography fit, come back as nan.
"""
import os as _os
import sys as _sys

_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.insert(0, _root)

from nano_vs_slam_amd.keypoint_metrics import (compute_homography, compute_matching_score, compute_repeatability,  # noqa: E402,F401
                                               evaluate_keypoint_net)
