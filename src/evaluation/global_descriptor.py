"""Alias so the reference's import line keeps working (eval_multitask.py:20, train_visloc.py:16, ./src on sys.path):

    from evaluation.global_descriptor import evaluate_global_descriptor

It resolves to the device implementation in ``nano-vs-slam_amd/vpr.py`` (a FlatL2Index in place of faiss, which this
module does not import).
"""
import os as _os
import sys as _sys

_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.insert(0, _root)

from nano_vs_slam_amd.vpr import FlatL2Index, evaluate_global_descriptor, recall_at_n  # noqa: E402,F401
