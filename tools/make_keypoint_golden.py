"""Generate tests/golden/keypoints/rep_*.npz by running the REFERENCE's compute_repeatability
(src/evaluation/detector.py, imported read-only from /root/reference) on the cases of tests/keypoint_ref.make_case.

    python3 tools/make_keypoint_golden.py

Runs only where the reference exists; no test, smoke() or bench.py reads it, they read the committed fixtures.  detector.py
needs numpy and utils/keypoints.py alone; the latter's `import cv2` line (used by its drawing helper only) is satisfied by an
empty stand-in module, OpenCV not being installed.  compute_matching_score calls cv2.BFMatcher and therefore cannot be
pinned this way: it stays restated in tests/keypoint_ref.py.  Each fixture holds arrays only: the case's inputs, keep_k,
distance_thresh and the reference's four outputs (N1, N2, repeatability, loc_err).
"""
import importlib.util
import os
import sys
import types

import numpy as np

REFERENCE = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a folder of its own: the suite takes every tests/golden/*.npz for a model fixture
GOLDEN = os.path.join(ROOT, "tests", "golden", "keypoints")

# (name, seed, k0, k1, image_shape, keep_k, distance_thresh): the sizes of tests/test_gpu_keypoint_metrics.py
CASES = [
    ("37x53_k300", 11, 37, 53, (240, 320), 300, 3),
    ("37x53_k10_odd_box", 12, 37, 53, (37, 53), 10, 3),
    ("300x257_k100", 13, 300, 257, (240, 320), 100, 3),
    ("300x257_k300", 13, 300, 257, (240, 320), 300, 3),
    ("1000x1000_k300", 14, 1000, 1000, (240, 320), 300, 3),
    ("1000x1000_k2000_t1", 14, 1000, 1000, (240, 320), 2000, 1),
    ("0x40_k300", 15, 0, 40, (240, 320), 300, 3),
    ("40x0_k300", 16, 40, 0, (240, 320), 300, 3),
    ("1x1_k300", 17, 1, 1, (240, 320), 300, 3),
]


def reference_compute_repeatability():
    """The reference's function, and nothing else: refuses to run against anything outside /root/reference."""
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))              # empty stand-in: only the import line needs it
    sys.path[:] = [REFERENCE] + [p for p in sys.path if os.path.realpath(p or ".") != os.path.realpath(ROOT)]
    path = os.path.join(REFERENCE, "src", "evaluation", "detector.py")
    spec = importlib.util.spec_from_file_location("reference_detector", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for m in (mod, sys.modules["utils.keypoints"]):
        where = os.path.realpath(m.__file__)
        if not where.startswith(REFERENCE + os.sep):
            raise RuntimeError(f"{m.__name__} resolved to {where}: fixtures must come from the reference under {REFERENCE}")
    return mod.compute_repeatability


def main():
    compute_repeatability = reference_compute_repeatability()
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import keypoint_ref as kr
    os.makedirs(GOLDEN, exist_ok=True)
    for name, seed, k0, k1, shape, keep_k, thresh in CASES:
        case = kr.make_case(seed, k0, k1, 32, shape, (keep_k,), distance_thresh=thresh)
        data = {"image_shape": shape, "homography": case["homography"], "prob": case["prob"], "warped_prob": case["warped_prob"]}
        n1, n2, rep, loc = compute_repeatability(data, keep_k_points=keep_k, distance_thresh=thresh)
        path = os.path.join(GOLDEN, f"rep_{name}.npz")
        np.savez_compressed(path, prob=case["prob"], warped_prob=case["warped_prob"], homography=case["homography"],
                            image_shape=np.asarray(shape, np.int64), keep_k=np.int64(keep_k), distance_thresh=np.float64(thresh),
                            N1=np.int64(n1), N2=np.int64(n2), repeatability=np.float64(rep), loc_err=np.float64(loc))
        print(f"{os.path.basename(path)}: {os.path.getsize(path)} B  N1 {n1} N2 {n2} repeatability {rep!r} loc_err {loc!r}")


if __name__ == "__main__":
    main()
