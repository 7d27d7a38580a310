"""Time one NetVLAD training step (NetVLADTrainer.step_encoded) against the plain torch formulation on the same device.

    python3 tools/bench_vlad_training.py [--B 4] [--negs 10] [--H 120] [--W 160] [--config S]
                                         [--out profiles/vlad_training.json] [--commit NAME]

Inputs: the reference's training defaults (train_visloc.py: batch of 4 queries, 10 negatives each, 120 x 160 frames, margin
0.1, lr 1e-4) on synthetic frames; the encoder map comes from model.only_encoder once and is not part of the timing
(both sides start from it: the encoder is frozen here).
Device path: forward, triplet loss, backward and two Adam updates of csrc/vlad_train.hip through step_encoded.
Baseline: a restated NetVLAD module (normalise, 1x1 conv as a matmul, softmax, aggregation as one einsum minus the
assignment sums times the centroids, both normalisations) + torch autograd + torch.nn.TripletMarginLoss(margin ** 0.5,
p=2, reduction="sum") / nNeg + torch.optim.Adam, on the same device.  Two forms of the loss: `loop`, the reference's per
query, per negative calls (train_visloc.py:270-276), and `batched`, one call on gathered rows.
HIP-event time per step over a window of back-to-back steps after a warm-up, three repeats; all three are recorded.
Nothing is gated on the result; the file is where the numbers go.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, repeats=3):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(repeats):
        s.record()
        for _ in range(steps):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--negs", type=int, default=10)
    ap.add_argument("--H", type=int, default=120)
    ap.add_argument("--W", type=int, default=160)
    ap.add_argument("--config", default="S")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--commit", default="", help="recorded when the tree is not a git checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vlad_training.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from nano_vs_slam_amd import vlad_training as vt
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    from oracle.weights import spread_state_dict, synthetic_frames

    dev = "cuda:0"
    model = tiny_factory(args.config, 28)
    sd = spread_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(dev).eval()
    model.training = False
    B, counts = args.B, [args.negs] * args.B
    n_neg = sum(counts)
    N = 2 * B + n_neg
    frames = torch.from_numpy(synthetic_frames(N, args.H, args.W, seed=5)).to(dev)
    with torch.no_grad():
        enc = model.only_encoder(frames)
    layer = model.vlad_head.netvlad
    K, C = layer.centroids.shape
    W0, c0 = layer.conv.weight.detach().clone(), layer.centroids.detach().clone()
    res = {"device": torch.cuda.get_device_name(0), "config": args.config, "B": B, "negatives_per_query": args.negs, "frames": N,
           "H": args.H, "W": args.W, "S": int(enc[0, 0].numel()), "K": int(K), "C": int(C), "margin": 0.1, "lr": 1e-4,
           "steps_per_window": args.steps,
           "commit": subprocess.run(["git", "describe", "--always", "--dirty"], cwd=ROOT, capture_output=True,
                                    text=True).stdout.strip() or args.commit or "unknown"}

    # the device path
    trainer = vt.NetVLADTrainer(model, lr=1e-4, margin=0.1)
    cnt_dev = torch.tensor(counts, dtype=torch.int32, device=dev)
    first = float(trainer.step_encoded(enc, B, cnt_dev))
    ms = timed(lambda: trainer.step_encoded(enc, B, cnt_dev), args.steps)
    res.update(step_encoded_ms=ms, step_encoded_ms_best=min(ms), first_loss=first)

    # the plain torch formulation
    w = torch.nn.Parameter(W0.clone().view(K, C))
    cent = torch.nn.Parameter(c0.clone())
    opt = torch.optim.Adam([w, cent], lr=1e-4)
    criterion = torch.nn.TripletMarginLoss(margin=0.1 ** 0.5, p=2, reduction="sum")
    owner = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(counts, device=dev))
    x = enc.view(N, C, -1)

    def netvlad(x):
        xh = F.normalize(x, p=2.0, dim=1)                                  # [N, C, S]
        a = F.softmax(torch.einsum("kc,ncs->nks", w, xh), dim=1)
        vlad = torch.einsum("nks,ncs->nkc", a, xh) - a.sum(-1).unsqueeze(2) * cent.unsqueeze(0)
        vlad = F.normalize(vlad, p=2.0, dim=2).reshape(N, -1)
        return F.normalize(vlad, p=2.0, dim=1)

    def torch_step(loop):
        opt.zero_grad()
        vq, vp, vn = torch.split(netvlad(x), [B, B, n_neg])
        if loop:
            loss, j = 0, 0
            for i, c in enumerate(counts):
                for _ in range(c):
                    loss = loss + criterion(vq[i:i + 1], vp[i:i + 1], vn[j:j + 1])
                    j += 1
        else:
            loss = criterion(vq[owner], vp[owner], vn)
        loss = loss / n_neg
        loss.backward()
        opt.step()
        return loss.detach()

    torch_first = float(torch_step(False))
    for name, loop in (("batched", False), ("loop", True)):
        ms = timed(lambda: torch_step(loop), args.steps)
        res[f"torch_{name}_ms"] = ms
        res[f"torch_{name}_ms_best"] = min(ms)
    res["torch_first_loss"] = torch_first
    assert abs(first - torch_first) < 1e-5, (first, torch_first)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
