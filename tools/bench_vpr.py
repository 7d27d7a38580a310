"""Time FlatL2Index.search (csrc/vpr.hip) against a torch fp32 baseline in the same process.

    python3 tools/bench_vpr.py [--dry-run] [--out profiles/vpr_search.json] [--window 1.0]

Shapes: (a) Pittsburgh-30k-like Q 6816 x N 10000, dim 4096; (b) Pittsburgh-250k-like Q 8192 x N 81920; (c) one query
against N 81920 (loop closure); (d) dim 1536 (the N configs), Q 8192 x N 81920.  k = 20.  Per shape and precision:
HIP-event time of a window of >= --window seconds of back-to-back searches after a warm-up, the kernel and the baseline
alternated (kernel, baseline, kernel, baseline) and the best window of each kept.  TFLOP/s = 2 Q N dim / t against the
bound of the arithmetic (split fp16: 2516.6 / 3 = 838.9 TFLOP/s of dense fp16 MFMA; fp32 MFMA: 157.3); GB/s for (c)
against 6.3 TB/s achievable HBM bandwidth (bytes: the packed rows the split form reads, or the fp32 rows).
Baseline: (|d|^2 - 2 q @ db^T).topk(k, largest=False) in fp32, chunked over queries to bound its memory.
--dry-run (no device): shapes, FLOPs and bytes only.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"a": (6816, 10000, 4096), "b": (8192, 81920, 4096), "c": (1, 81920, 4096), "d": (8192, 81920, 1536)}
K = 20
BOUND_TF = {"f16x3": 2516.6 / 3, "fp32": 157.3}
HBM_GBS = 6300.0


def work(Q, N, D, prec):
    flops = 2.0 * Q * N * D
    row = 4 * D + 16 if prec == "f16x3" else 4 * D
    return flops, N * row + Q * D * 4


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vpr_search.json"))
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--shapes", default="abcd")
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    if args.dry_run:
        for name in args.shapes:
            Q, N, D = SHAPES[name]
            for prec in BOUND_TF:
                f, b = work(Q, N, D, prec)
                print(json.dumps({"shape": name, "Q": Q, "N": N, "dim": D, "k": K, "precision": prec, "gflop": f / 1e9,
                                  "bytes": b}))
        return
    import torch
    from nano_vs_slam_amd.vpr import FlatL2Index
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for name in args.shapes:
        Q, N, D = SHAPES[name]
        db = torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=g), dim=1)
        q = torch.nn.functional.normalize(torch.randn(Q, D, device="cuda", generator=g), dim=1)
        dn = (db * db).sum(1)
        chunk = max(1, (1 << 30) // (N * 4))

        def baseline():
            for i in range(0, Q, chunk):
                (dn[None, :] - 2.0 * q[i:i + chunk] @ db.T).topk(K, dim=1, largest=False)
        for prec in BOUND_TF:
            ix = FlatL2Index(D, precision=prec)
            ix.add(db)
            ours = lambda: ix.search(q, K)
            t_ours, t_base = [], []
            for _ in range(args.rounds):
                t_ours.append(timed(ours, args.window))
                t_base.append(timed(baseline, args.window))
            f, b = work(Q, N, D, prec)
            ms, bms = min(t_ours), min(t_base)
            r = {"shape": name, "Q": Q, "N": N, "dim": D, "k": K, "precision": prec, "ms": round(ms, 4),
                 "tflops": round(f / ms / 1e9, 2), "bound_tflops": round(BOUND_TF[prec], 1),
                 "frac_of_bound": round(f / ms / 1e9 / BOUND_TF[prec], 4),
                 "baseline_torch_fp32_ms": round(bms, 4), "speedup_vs_baseline": round(bms / ms, 2)}
            if name == "c":
                r.update({"gbs": round(b / ms / 1e6, 1), "bound_gbs": HBM_GBS, "frac_of_hbm": round(b / ms / 1e6 / HBM_GBS, 4)})
            print(json.dumps(r), flush=True)
            rows.append(r)
            del ix
        del db, q, dn
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "k": K, "results": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
