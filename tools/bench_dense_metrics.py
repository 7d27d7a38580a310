"""Time the dense-head scores (csrc/dense_metrics.hip) against their plain torch formulations.

    python3 tools/bench_dense_metrics.py [--dry-run] [--out profiles/dense_metrics.json] [--window 0.5]

Shape: 64 images of 240 x 320, 28 classes (a batch of the flagship workload's dense maps).  Steps, each in a fresh child
process under its own time limit (--step-timeout seconds; a step that exceeds it or fails is recorded as such and
nothing more is started on the device):
  seg        dense_metrics.seg_stats, uint8 labels with ~5 % ignored, no confusion matrix
  seg_conf   the same with the [B, C, C] confusion matrix (the LDS-tile form at 28 classes)
  depth      dense_metrics.depth_sums, no mask
Baselines: segmentation, ONE torch.bincount on target * C + pred for the whole batch (an offset per image, ignored pixels
sent to a spare bin) -> [B, C, C], from which tp / fp / fn / tn follow; depth, the reference's nine float32 expressions
(compute_errors_torch, src/evaluation/depth_estimation.py:58-83) without the .item() reads.  Per step: HIP-event time of a window of >= --window
seconds of back-to-back calls after a warm-up, kernel and baseline alternated over --rounds rounds, the best window of each
kept.  GB/s counts the bytes a call has to read (pred 8 B + label 1 B, or two floats, per pixel) against 6.3 TB/s of
achievable HBM bandwidth; the maps of one batch (44 MB / 39 MB) stay in the 256 MB Infinity Cache between back-to-back
calls, so the figure is no HBM rate, only a distance from that bound.  --dry-run (no device): shapes and bytes only.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W, C = 64, 240, 320, 28
STEPS = {"seg": 9, "seg_conf": 9, "depth": 8}        # bytes read per pixel
HBM_GBS = 6300.0


def timed(fn, window):
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


def run_step(step, window, rounds):
    import torch
    from nano_vs_slam_amd import dense_metrics as dm
    g = torch.Generator(device="cuda").manual_seed(0)
    if step == "depth":
        gt = torch.rand(B, H, W, device="cuda", generator=g) * 79.5 + 0.5
        pred = gt * torch.exp(0.3 * torch.randn(B, H, W, device="cuda", generator=g))

        def ours():
            return dm.depth_sums(gt, pred)

        def baseline():
            thresh = torch.max(gt / pred, pred / gt)
            err = torch.log(pred) - torch.log(gt)
            return ((thresh < 1.25).float().mean(), (thresh < 1.25 ** 2).float().mean(), (thresh < 1.25 ** 3).float().mean(),
                    torch.mean(torch.abs(gt - pred) / gt), torch.mean((gt - pred) ** 2 / gt), torch.sqrt(((gt - pred) ** 2).mean()),
                    torch.sqrt(((torch.log(gt) - torch.log(pred)) ** 2).mean()),
                    torch.sqrt(torch.mean(err ** 2) - torch.mean(err) ** 2) * 100,
                    (torch.abs(torch.log10(gt) - torch.log10(pred))).mean())
    else:
        target = torch.randint(0, C, (B, H, W), device="cuda", generator=g)
        pred = torch.where(torch.rand(B, H, W, device="cuda", generator=g) < 0.7, target,
                           torch.randint(0, C, (B, H, W), device="cuda", generator=g))
        target = torch.where(torch.rand(B, H, W, device="cuda", generator=g) < 0.05, torch.full_like(target, 255), target)
        target = target.to(torch.uint8)

        def ours():
            return dm.seg_stats(pred, target, C, 255, confusion=step == "seg_conf")

        offset = (torch.arange(B, device="cuda") * (C * C + 1))[:, None]

        def baseline():
            t, p = target.reshape(B, -1).to(torch.int64), pred.reshape(B, -1)
            key = torch.where(t == 255, torch.full_like(t, C * C), t * C + p) + offset      # ignored pixels: one spare bin
            conf = torch.bincount(key.reshape(-1), minlength=B * (C * C + 1)).reshape(B, C * C + 1)[:, :C * C].reshape(B, C, C)
            tp = conf.diagonal(dim1=1, dim2=2)
            fp, fn = conf.sum(1) - tp, conf.sum(2) - tp
            return tp, fp, fn, conf.sum((1, 2))[:, None] - tp - fp - fn
    t_ours, t_base = [], []
    for _ in range(rounds):
        t_ours.append(timed(ours, window))
        t_base.append(timed(baseline, window))
    ms, bms = min(t_ours), min(t_base)
    nbytes = B * H * W * STEPS[step]
    return {"step": step, "B": B, "H": H, "W": W, "classes": C, "ms": round(ms, 4), "gbs": round(nbytes / ms / 1e6, 1),
            "bound_gbs": HBM_GBS, "frac_of_hbm": round(nbytes / ms / 1e6 / HBM_GBS, 4), "baseline_torch_ms": round(bms, 4),
            "speedup_vs_baseline": round(bms / ms, 2), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_metrics.json"))
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
            print(json.dumps({"step": s, "B": B, "H": H, "W": W, "classes": C, "bytes": B * H * W * STEPS[s]}))
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
        json.dump({"device": device, "note": "back-to-back calls on the same maps: the inputs stay in the Infinity Cache",
                   "results": rows}, fh, indent=1)
        fh.write("\n")
    return worst


if __name__ == "__main__":
    sys.exit(main())
