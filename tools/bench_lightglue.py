#!/usr/bin/env python3
"""BASELINE config 5: KP2DTiny-S keypoints + LightGlue on 480x640 image pairs (synthetic frames, seeded weights).

    python3 tools/bench_lightglue.py [--pairs 8] [--steps 20] [--kpts 1024] [--sweep 8,16,32]

Prints one JSON line per pairs-per-step value: image pairs/s for extractor (both images) + K3 top-k + matcher, the matcher
alone, and the `roofline` object of the step's dominant kernel family (HIP events around every launch of the extractor's
forward on the 2 x pairs frames, as bench.py does; the matcher's ~25 launches are timed as a whole beside it).

    python3 tools/bench_lightglue.py --width-confidence 0.6 [--parent-tree DIR] [--pairs 8] [--kpts 1024]

Point pruning A/B of the matcher alone on seeded random keypoint sets: pairs/s with pruning off and on (three repeats each,
same process, same box), the mean survivors per layer and set, and — with --parent-tree, a BUILT checkout of the parent
commit — the parent's pairs/s with pruning off, three repeats in a fresh child process on the same inputs.  Written to
profiles/lightglue_pruning.json.  Seeded random weights: the pruned share says nothing about trained weights.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --tree DIR: import the package from another (built) checkout, e.g. the parent commit, for an A/B on one box
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else ROOT
sys.path.insert(0, TREE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kpts", type=int, default=1024)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--sweep", default="", help="comma-separated pairs-per-step values (one line each) instead of --pairs")
    ap.add_argument("--filter-threshold", type=float, default=0.0,
                    help="LightGlue filter_threshold (seeded random weights give matching scores near 0: with the reference configs' "
                         "0.1 the filter and the compaction would see no match at all)")
    ap.add_argument("--width-confidence", type=float, default=-1.0,
                    help="> 0: the point-pruning A/B of the matcher alone -> profiles/lightglue_pruning.json")
    ap.add_argument("--parent-tree", default="", help="built checkout of the parent commit: its pruning-off figure beside ours")
    ap.add_argument("--tree", default="", help="import the package from this checkout instead of the tool's own")
    ap.add_argument("--matcher-off-only", action="store_true", help="print the pruning-off repeats as one JSON line (child mode)")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.matcher_off_only:
        print(json.dumps({"off_pairs_per_s": matcher_rates(a, -1.0)[0]}), flush=True)
        return
    if a.width_confidence > 0:
        pruning_ab(a)
        return
    for pairs in ([int(v) for v in a.sweep.split(",")] if a.sweep else [a.pairs]):
        a.pairs = pairs
        run(a)


def matcher_rates(a, wc):
    """([pairs/s] * repeats of the matcher alone, last prediction) on seeded random unit descriptors / keypoints."""
    from lightglue.lightglue import LightGlue
    from lightglue.lightglue_configs import get_light_glue_config
    from nano_vs_slam_amd.synthetic import seeded_linear_state_dict
    dev = torch.device("cuda:0")
    conf = dict(get_light_glue_config("S"), filter_threshold=a.filter_threshold, width_confidence=wc)
    lg = LightGlue(conf)
    shapes = {k: tuple(v.shape) for k, v in lg.state_dict().items()}
    lg.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_linear_state_dict(shapes).items()})
    lg = lg.to(dev).eval()
    g = torch.Generator().manual_seed(0)
    size = torch.tensor([[float(a.width), float(a.height)]]).expand(a.pairs, 2).contiguous().to(dev)
    kp = lambda: (torch.rand(a.pairs, a.kpts, 2, generator=g) * torch.tensor([float(a.width), float(a.height)])).to(dev)
    ds = lambda: torch.nn.functional.normalize(torch.randn(a.pairs, a.kpts, 32, generator=g), dim=-1).to(dev)
    data = {"keypoints0": kp(), "keypoints1": kp(), "descriptors0": ds(), "descriptors1": ds(),
            "view0": {"image_size": size}, "view1": {"image_size": size}}
    rates, pred = [], None
    with torch.no_grad():
        for _ in range(a.repeats):
            for _ in range(a.warmup):
                pred = lg(data)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                pred = lg(data)
            torch.cuda.synchronize()
            rates.append(round(a.pairs * a.steps / (time.perf_counter() - t0), 1))
    return rates, pred


def pruning_ab(a):
    import subprocess
    off, _ = matcher_rates(a, -1.0)
    on, pred = matcher_rates(a, a.width_confidence)
    n_layers = 4
    # a point dropped after layer i holds i + 1, a survivor n_layers: survivors after layer i = #(prune > i + 1)
    surv = {f"set{s}": [round(float((pred[f"prune{s}"] > i + 1).sum(1).float().mean()), 1) for i in range(n_layers - 1)]
            for s in (0, 1)}
    out = {"metric": "LightGlue S matcher alone, image pairs/s, point pruning off / on", "unit": "pairs/s",
           "pairs_per_step": a.pairs, "keypoints": a.kpts, "steps": a.steps, "width_confidence": a.width_confidence,
           "filter_threshold": a.filter_threshold, "off_pairs_per_s": off, "on_pairs_per_s": on,
           "mean_survivors_after_layer": surv, "parent_off_pairs_per_s": None,
           "data": "seeded random keypoints / unit descriptors, seeded random weights (the pruned share says nothing about "
                   "trained weights)"}
    if a.parent_tree:
        # a fresh child process (its own HIP context and library), same inputs, pruning off
        a.parent_tree = os.path.abspath(a.parent_tree)
        cmd = [sys.executable, os.path.abspath(__file__), "--tree", a.parent_tree, "--matcher-off-only", "--pairs", str(a.pairs),
               "--steps", str(a.steps), "--warmup", str(a.warmup), "--kpts", str(a.kpts), "--repeats", str(a.repeats),
               "--filter-threshold", str(a.filter_threshold), "--height", str(a.height), "--width", str(a.width)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=a.parent_tree, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"parent tree run failed ({r.returncode}): {r.stderr[-2000:]}")
        out["parent_off_pairs_per_s"] = json.loads(r.stdout.strip().splitlines()[-1])["off_pairs_per_s"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "lightglue_pruning.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


def run(a):
    from lightglue.lightglue import LightGlue
    from lightglue.lightglue_configs import get_light_glue_config
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    from nano_vs_slam_amd.pipeline import two_view_match
    from nano_vs_slam_amd.synthetic import seeded_linear_state_dict
    from nano_vs_slam_amd.synthetic import spread_state_dict
    dev = torch.device("cuda:0")
    net = tiny_factory("S", 28)
    sd = spread_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()})
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    net = net.to(dev).eval()
    net.training = False
    conf = dict(get_light_glue_config("S"), filter_threshold=a.filter_threshold)
    lg = LightGlue(conf)
    shapes = {k: tuple(v.shape) for k, v in lg.state_dict().items()}
    lg.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_linear_state_dict(shapes).items()})
    lg = lg.to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    im0 = torch.rand(a.pairs, 3, a.height, a.width, device=dev, generator=g)
    im1 = torch.rand(a.pairs, 3, a.height, a.width, device=dev, generator=g)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3

    with torch.no_grad():
        p0, p1, m = two_view_match(net, lg, im0, im1, a.kpts)
        data = {"keypoints0": p0["keypoints"], "keypoints1": p1["keypoints"], "descriptors0": p0["descriptors"],
                "descriptors1": p1["descriptors"], "view0": {"image_size": p0["image_size"]},
                "view1": {"image_size": p1["image_size"]}}
        t_all = timed(lambda: two_view_match(net, lg, im0, im1, a.kpts))
        t_lg = timed(lambda: lg(data))
        # roofline of the dominant kernel family: the extractor's forward on the 2 x pairs frames, one lane, HIP events per launch
        import bench
        H, W = a.height - a.height % 8, a.width - a.width % 8
        x = ((torch.cat([im0[:, :, :H, :W], im1[:, :, :H, :W]], 0) - 0.5) * 2.0).contiguous()
        agg = bench.kernel_profile(net, x, H, W, 3)
    dom = max(agg, key=lambda k: agg[k]["ms"])
    d = agg[dom]
    split = "f16x3" in dom
    peak = bench.PEAK_F16_MFMA_TFLOPS / 3.0 if split else bench.PEAK_F32_MFMA_TFLOPS
    achieved = d["flops"] / (d["ms"] * 1e-3) / 1e12
    roof = {"bound": "mfma", "kernel": dom, "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4), "traffic": None,
            "avg_launch_ms": round(d["ms"] / d["launches"], 4), "launches_per_step": d["launches"] // 3,
            "share_of_extractor_kernel_time": round(d["ms"] / sum(v["ms"] for v in agg.values()), 4),
            "extractor_kernel_ms_sum": round(sum(v["ms"] for v in agg.values()) / 3, 3),
            "note": "extractor forward of the step's 2 x pairs frames, single lane; the matcher (fp32, ~25 small launches) is matcher_ms_per_step"}
    print(json.dumps({
        "metric": "image pairs/sec KP2DTiny-S + LightGlue 480x640", "value": round(a.pairs / t_all * 1e3, 1),
        "unit": "pairs/s", "pairs_per_step": a.pairs, "keypoints": a.kpts, "ms_per_step": round(t_all, 3),
        "matcher_ms_per_step": round(t_lg, 3), "matcher_pairs_per_s": round(a.pairs / t_lg * 1e3, 1),
        "matched_fraction": round(float((m["matches0"] >= 0).float().mean()), 4), "data": "synthetic",
        "filter_threshold": a.filter_threshold, "roofline": roof,
        "dtype": "f16x3 extractor, fp32 matcher"}), flush=True)


if __name__ == "__main__":
    main()
