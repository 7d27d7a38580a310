"""Alias so the reference's import line keeps working (src/evaluation/keypoints.py:8, ./src on sys.path):

    from evaluation.detector import compute_repeatability

It resolves to the device implementation in ``nano-vs-slam_amd/keypoint_metrics.py`` (kp2d_kp_repeatability in place of the
numpy code; this module does not import cv2).
"""
import os as _os
import sys as _sys

_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.insert(0, _root)

from nano_vs_slam_amd.keypoint_metrics import compute_repeatability  # noqa: E402,F401
