"""Time the keypoint scores (csrc/keypoint_metrics.hip) against the reference-style host path.

    python3 tools/bench_keypoint_metrics.py [--dry-run] [--out profiles/keypoint_metrics.json] [--window 0.5]

Shape: one batch of 16 pairs, 1000 rows per image, 32-wide descriptors, bounds (240, 320): the rows of tests/keypoint_ref's
case generator, resident on the device as the model would leave them.  Steps, each in a fresh child process under its own
time limit (--step-timeout seconds; a step that exceeds it or fails is recorded as such and nothing more is started on the
device):
  repeatability   keypoint_metrics.repeatability_stats, keep_k = 300, distance_thresh = 3
  matching_score  keypoint_metrics.matching_score_stats, keep_k = 1000
Per step three figures: ``ms`` the HIP-event time of a window of >= --window seconds of back-to-back calls (the device work
alone), ``ms_with_read`` the wall-clock time of a call plus the one host read of its counts (what a caller waits for), and
``host_ms`` the wall-clock time of the reference's way: copy every row of the batch to the host, then the float64 numpy code
of tests/keypoint_ref.py pair by pair (the reference's own code for repeatability; for the matching score a numpy
brute-force matcher stands where the reference has cv2.BFMatcher, which is not installed, so that figure is no OpenCV
timing).  No speed-up is promised: what is measured is written.  --dry-run (no device): shapes only.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

B, K, C, SHAPE = 16, 1000, 32, (240, 320)
STEPS = {"repeatability": 300, "matching_score": 1000}       # keep_k


def event_ms(fn, window):
    import torch
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); fn(); e.record(); torch.cuda.synchronize()
    reps = max(1, int(window * 1000 / max(s.elapsed_time(e), 1e-3)))
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def wall_ms(fn, window):
    import torch
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter(); fn(); one = time.perf_counter() - t
    reps = max(1, int(window / max(one, 1e-6)))
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) / reps * 1e3


def run_step(step, window, rounds):
    import numpy as np
    import torch
    import keypoint_ref as kr
    from nano_vs_slam_amd import keypoint_metrics as km
    keep_k = STEPS[step]
    cases = [kr.make_case(900 + b, K, K, C, SHAPE, (keep_k,)) for b in range(B)]
    dev = lambda key, dt: torch.from_numpy(np.stack([c[key] for c in cases]).astype(dt)).cuda()
    p0, p1, d0, d1 = dev("prob", np.float32), dev("warped_prob", np.float32), dev("desc", np.float32), dev("warped_desc", np.float32)
    hom = dev("homography", np.float64)
    cnt = torch.full((B,), K, dtype=torch.int32, device="cuda")
    if step == "repeatability":
        def ours():
            return km.repeatability_stats(p0, cnt, p1, cnt, hom, SHAPE, keep_k, 3)

        def read():
            counts, le = ours()
            return counts.cpu(), le.cpu()

        def host():
            a, b, h = p0.cpu().numpy(), p1.cpu().numpy(), hom.cpu().numpy()
            return [kr.repeatability_stats(a[i], b[i], h[i], SHAPE, keep_k, 3) for i in range(B)]
    else:
        def ours():
            return km.matching_score_stats(p0, cnt, d0, p1, cnt, d1, hom, SHAPE, keep_k)

        def read():
            return ours().cpu()

        def host():
            a, b, h, x, y = p0.cpu().numpy(), p1.cpu().numpy(), hom.cpu().numpy(), d0.cpu().numpy(), d1.cpu().numpy()
            return [kr.matching_score_stats(a[i], b[i], x[i], y[i], h[i], SHAPE, keep_k) for i in range(B)]
    ms = min(event_ms(ours, window) for _ in range(rounds))
    ms_read = min(wall_ms(read, window) for _ in range(rounds))
    host_ms = min(wall_ms(host, window) for _ in range(rounds))
    return {"step": step, "pairs": B, "rows": K, "desc_width": C, "keep_k": keep_k, "ms": round(ms, 4), "ms_with_read": round(ms_read, 4),
            "host_ms": round(host_ms, 3), "host_over_device_with_read": round(host_ms / ms_read, 1), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoint_metrics.json"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--step-timeout", type=float, default=120.0)
    ap.add_argument("--child", default="", help="internal: run ONE step in this process and print its JSON line")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(run_step(args.child, args.window, args.rounds)), flush=True)
        return 0
    steps = [s for s in args.steps.split(",") if s]
    if args.dry_run:
        for s in steps:
            print(json.dumps({"step": s, "pairs": B, "rows": K, "desc_width": C, "keep_k": STEPS[s]}))
        return 0
    rows, device, worst = [], None, 0
    for s in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", s, "--window", str(args.window), "--rounds", str(args.rounds)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            rows.append({"step": s, "error": f"no result within {args.step_timeout:g} s"})
            print(json.dumps(rows[-1]), flush=True)
            worst = 124
            break                                        # a step that hangs: nothing more is started on the device
        if p.returncode != 0:
            rows.append({"step": s, "error": f"exit code {p.returncode}", "stderr": p.stderr[-2000:]})
            print(json.dumps(rows[-1]), flush=True)
            worst = p.returncode
            break                                        # nor after one that failed
        r = json.loads(p.stdout.strip().splitlines()[-1])
        device = r.pop("device")
        print(json.dumps(r), flush=True)
        rows.append(r)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": device, "note": "one batch of 16 pairs resident on the device; host_ms includes the copy of every row "
                                             "to the host, ms_with_read the read of the counts", "results": rows}, fh, indent=1)
        fh.write("\n")
    return worst


if __name__ == "__main__":
    sys.exit(main())
