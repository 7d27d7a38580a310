"""Time kp2d_kmeans_train (csrc/kmeans.hip) against a torch Lloyd on the same GPU, in the same process.

    python3 tools/bench_kmeans.py [--dry-run] [--out profiles/kmeans_train.json] [--window 1.0]

Shapes: (a) the reference's NetVLAD fit, n 16384 (50 000 descriptors subsampled by max_points_per_centroid) x d 64,
k 64, 100 iterations; (b) d 48, k 32 (the N configs); (c) a vocabulary: n 1 048 576 x d 128, k 4096, 10 iterations.
Per shape and precision: HIP-event time of a window of >= --window seconds of back-to-back trainings after a warm-up,
the kernels and the baseline alternated (ours, baseline, ours, baseline) and the best window of each kept.
Baseline: torch Lloyd in fp32 (argmin of |c|^2 - 2 x c^T, chunked over rows to bound its memory, index_add_, division).
For (a) also sklearn.cluster.KMeans (lloyd, one init, tol 0) on the host, wall clock.
One step is also run under torch.profiler to split its time by kernel into phases (pack + search / index build / sum /
update), to count its launches and to give the sum pass's GB/s (the rows and their index read once) against 6.3 TB/s.
--dry-run (no device): shapes, FLOPs of the assignment and bytes of the sum pass only.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"a": (16384, 64, 64, 100), "b": (16384, 48, 32, 100), "c": (1 << 20, 128, 4096, 10)}
PRECS = ("f16x3", "fp32")
HBM_GBS = 6300.0
PHASES = (("vpr_", "pack_search"), ("km_hist", "index_build"), ("km_colscan", "index_build"), ("km_scan", "index_build"),
          ("km_scatter", "index_build"), ("km_sum", "sum"), ("km_update", "update"), ("km_split", "update"),
          ("km_normalize", "update"))


def work(n, d, k):
    return 2.0 * n * k * d, n * d * 4 + n * 4


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


def torch_lloyd(x, c, niter):
    import torch
    n, k = x.shape[0], c.shape[0]
    chunk = max(1, (1 << 28) // k)
    for _ in range(niter):
        cn = (c * c).sum(1)
        a = torch.cat([(cn[None, :] - 2.0 * x[i:i + chunk] @ c.T).argmin(1) for i in range(0, n, chunk)])
        sums = torch.zeros_like(c).index_add_(0, a, x)
        c = sums / torch.bincount(a, minlength=k).clamp(min=1)[:, None].float()
    return c


def profile_step(x, c, flags):
    """-> (phase -> us, launches, us of km_sum_kernel) of one step, or (None, None, None) with the reason printed."""
    import torch
    from nano_vs_slam_amd.clustering import kmeans_step
    try:
        from torch.profiler import ProfilerActivity, profile
        kmeans_step(x, c, flags)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            kmeans_step(x, c, flags)
            torch.cuda.synchronize()
        phases, launches, t_sum = {}, 0, 0.0
        for ev in prof.events():
            if str(ev.device_type).endswith("CUDA"):
                name = ev.name
                us = float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0))
                hit = next((p for pre, p in PHASES if pre in name), None)
                if hit is None:
                    hit = "index_build" if "emset" in name or "fill" in name.lower() else None
                if hit is None:
                    continue
                launches += 1
                phases[hit] = phases.get(hit, 0.0) + us
                if "km_sum" in name:
                    t_sum += us
        if not launches:
            raise RuntimeError("the profiler recorded no device activity")
        return {p: round(v, 2) for p, v in phases.items()}, launches, t_sum
    except Exception as exc:                             # the record says so instead of guessing
        print(f"per-kernel profile unavailable: {exc!r}", flush=True)
        return None, None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_train.json"))
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    if args.dry_run:
        for name in args.shapes:
            n, d, k, niter = SHAPES[name]
            f, b = work(n, d, k)
            print(json.dumps({"shape": name, "n": n, "dim": d, "k": k, "niter": niter, "assign_gflop_per_iter": f / 1e9,
                              "sum_pass_bytes_per_iter": b}))
        return
    import torch
    from nano_vs_slam_amd.clustering import kmeans_train
    from nano_vs_slam_amd.vpr import PRECISIONS
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for name in args.shapes:
        n, d, k, niter = SHAPES[name]
        centre = torch.nn.functional.normalize(torch.randn(k, d, device="cuda", generator=g), dim=1)
        x = centre[torch.arange(n, device="cuda") % k] + 0.6 * torch.randn(n, d, device="cuda", generator=g) / d ** 0.5
        x = torch.nn.functional.normalize(x, dim=1).contiguous()
        init = x[:k].clone()
        baseline = lambda: torch_lloyd(x, init, niter)
        t_sk = None
        if name == "a":
            from sklearn.cluster import KMeans
            xh, ih = x.cpu().numpy().astype("float32"), init.cpu().numpy().astype("float32")
            t0 = time.perf_counter()
            KMeans(n_clusters=k, init=ih, n_init=1, algorithm="lloyd", tol=0, max_iter=niter).fit(xh)
            t_sk = (time.perf_counter() - t0) * 1e3
        for prec in PRECS:
            flags = PRECISIONS[prec]
            ours = lambda: kmeans_train(x, init, niter, flags)
            t_ours, t_base = [], []
            for _ in range(args.rounds):
                t_ours.append(timed(ours, args.window))
                t_base.append(timed(baseline, args.window))
            ms, bms = min(t_ours), min(t_base)
            phases, launches, t_sum = profile_step(x, init, flags)
            f, b = work(n, d, k)
            r = {"shape": name, "n": n, "dim": d, "k": k, "niter": niter, "precision": prec, "ms": round(ms, 4),
                 "ms_per_iter": round(ms / niter, 4), "baseline_torch_fp32_ms": round(bms, 4),
                 "speedup_vs_baseline": round(bms / ms, 2), "assign_tflops": round(f * niter / ms / 1e9, 2),
                 "step_phase_us": phases, "step_launches": launches}
            if t_sum:
                r.update({"sum_pass_us": round(t_sum, 2), "sum_pass_gbs": round(b / t_sum / 1e3, 1), "bound_gbs": HBM_GBS,
                          "sum_pass_frac_of_hbm": round(b / t_sum / 1e3 / HBM_GBS, 4)})
            if t_sk is not None:
                r["sklearn_host_ms"] = round(t_sk, 1)
            print(json.dumps(r), flush=True)
            rows.append(r)
        del x, init, centre
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "results": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
