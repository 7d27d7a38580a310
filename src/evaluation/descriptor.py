"""Alias so the reference's import line keeps working (src/evaluation/keypoints.py:7, ./src on sys.path):

    from evaluation.descriptor import compute_homography, compute_matching_score

It resolves to the device implementation in ``nano-vs-slam_amd/keypoint_metrics.py`` (kp2d_kp_matching_score in place of
cv2.BFMatcher and numpy; this module does not import cv2).  ``compute_homography``, the RANSAC homography fit, is outside
this build's scope and raises.
"""
import os as _os
import sys as _sys

_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.insert(0, _root)

from nano_vs_slam_amd.keypoint_metrics import compute_homography, compute_matching_score  # noqa: E402,F401

MAX_VAL = 1000
