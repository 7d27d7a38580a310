"""Time one head training step (VPRHeadTrainer.step_features) against the plain torch formulation on the same device.

    python3 tools/bench_vpr_head_training.py [--B 4] [--negs 10] [--H 120] [--W 160] [--config S]
                                             [--out profiles/vpr_head_training.json] [--commit NAME] [--baseline-only]
                                             [--bn batch] [--dropout 0.2]

Inputs: the reference's training defaults (train_visloc.py: batch of 4 queries, 10 negatives each, 120 x 160 frames, margin
0.1, lr 1e-4) on synthetic frames; the backbone map comes from model.backbone_features once (model.forward_with_tap where
the model has no such method) and is not part of the timing: both sides start from it, the backbone is frozen.
Device path: three CBR forwards, NetVLAD forward, triplet loss, NetVLAD backward and input gradient, three CBR backwards and
eleven Adam updates through step_features; `split_ms` times each call of one step on its own (HIP events around the call,
the mean of 20), which adds up to more than the step where the calls overlap the host's launch work.
Baseline: a restated head (F.conv2d, F.batch_norm on the running statistics, F.leaky_relu, NetVLAD as normalise, matmul,
softmax, one einsum, both normalisations) + torch autograd + torch.nn.TripletMarginLoss(margin ** 0.5, p=2,
reduction="sum") / nNeg on gathered rows + torch.optim.Adam over the eleven parameters, on the same device.  The baseline
needs nothing of this package's training modules (--baseline-only), so it runs on earlier commits too.
HIP-event time per step over a window of back-to-back steps after a warm-up, three repeats; all three are recorded.
--bn batch [--dropout P] times the reference's own mode, the head under model.train(): VPRHeadTrainer(bn="batch", dropout=P)
against the restated head with F.batch_norm(training=True) on the batch's statistics, its running-statistics update, and
F.dropout2d(P) behind convlad1; the two sides draw different masks, so their first losses are compared only at P = 0.  The
default --out is then profiles/vpr_head_training_batchnorm.json.  --merge-into FILE writes the result under --label in an
existing JSON file instead of a file of its own (several modes and commits side by side in one file).
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
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--bn", choices=("running", "batch"), default="running")
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-into", default=None, help="an existing JSON file: the result goes under --label there")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    batch = args.bn == "batch"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "vpr_head_training_batchnorm.json" if batch or args.dropout else "vpr_head_training.json")
    import numpy as np
    import torch
    import torch.nn.functional as F
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    from oracle.weights import spread_state_dict, synthetic_frames

    dev = "cuda:0"
    model = tiny_factory(args.config, 28)
    sd = spread_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(dev).eval()
    model.training = False
    model.set_precision("fp32")
    B, counts = args.B, [args.negs] * args.B
    n_neg = sum(counts)
    N = 2 * B + n_neg
    frames = torch.from_numpy(synthetic_frames(N, args.H, args.W, seed=5)).to(dev)
    c4, cell = int(model.channel_dims[3]), int(model.cell)
    with torch.no_grad():
        if hasattr(model, "backbone_features"):
            feat = model.backbone_features(frames)
        else:
            feat = model.forward_with_tap(frames, "backbone.conv4b", (c4, args.H // cell, args.W // cell))[1]
    head = model.vlad_head
    layers = (head.convlad1, head.convlad2, head.convlad3)
    K, C = head.netvlad.centroids.shape
    slope = 0.01 if model.leaky_relu else 0.0
    res = {"device": torch.cuda.get_device_name(0), "config": args.config, "B": B, "negatives_per_query": args.negs, "frames": N,
           "H": args.H, "W": args.W, "map": [int(feat.shape[2]), int(feat.shape[3])], "Cin": c4, "K": int(K), "C": int(C), "margin": 0.1,
           "lr": 1e-4, "steps_per_window": args.steps, "bn": args.bn, "dropout": args.dropout,
           "commit": subprocess.run(["git", "describe", "--always", "--dirty"], cwd=ROOT, capture_output=True,
                                    text=True).stdout.strip() or args.commit or "unknown"}

    # the plain torch formulation, on copies of the parameters (before the device path moves the model's own)
    convs = [torch.nn.Parameter(l.conv.weight.detach().clone()) for l in layers]
    gammas = [torch.nn.Parameter(l.bn.weight.detach().clone()) for l in layers]
    betas = [torch.nn.Parameter(l.bn.bias.detach().clone()) for l in layers]
    stats = [(l.bn.running_mean.detach().clone(), l.bn.running_var.detach().clone(), l.bn.eps, l.bn.momentum) for l in layers]
    w = torch.nn.Parameter(head.netvlad.conv.weight.detach().clone().view(K, C))
    cent = torch.nn.Parameter(head.netvlad.centroids.detach().clone())
    opt = torch.optim.Adam([t for trio in zip(convs, gammas, betas) for t in trio] + [w, cent], lr=1e-4)
    criterion = torch.nn.TripletMarginLoss(margin=0.1 ** 0.5, p=2, reduction="sum")
    owner = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(counts, device=dev))

    def torch_head(x):
        for i, (cw, g, b, (mean, var, eps, mom)) in enumerate(zip(convs, gammas, betas, stats)):
            x = F.batch_norm(F.conv2d(x, cw, padding=1), mean, var, g, b, training=batch, momentum=mom, eps=eps)
            x = F.leaky_relu(x, slope) if slope else F.relu(x)
            if i == 0 and args.dropout:
                x = F.dropout2d(x, args.dropout, training=True)
        xh = F.normalize(x.view(N, C, -1), p=2.0, dim=1)
        a = F.softmax(torch.einsum("kc,ncs->nks", w, xh), dim=1)
        vlad = torch.einsum("nks,ncs->nkc", a, xh) - a.sum(-1).unsqueeze(2) * cent.unsqueeze(0)
        vlad = F.normalize(vlad, p=2.0, dim=2).reshape(N, -1)
        return F.normalize(vlad, p=2.0, dim=1)

    def torch_step():
        opt.zero_grad()
        vq, vp, vn = torch.split(torch_head(feat), [B, B, n_neg])
        loss = criterion(vq[owner], vp[owner], vn) / n_neg
        loss.backward()
        opt.step()
        return loss.detach()

    res["torch_first_loss"] = float(torch_step())
    ms = timed(torch_step, args.steps)
    res.update(torch_ms=ms, torch_ms_best=min(ms))

    if not args.baseline_only:
        from nano_vs_slam_amd import vlad_training as vt, vpr_head_training as ht
        kw = {"bn": args.bn, "dropout": args.dropout} if batch or args.dropout else {}      # (earlier commits: no such arguments)
        trainer = ht.VPRHeadTrainer(model, lr=1e-4, margin=0.1, **kw)
        cnt_dev = torch.tensor(counts, dtype=torch.int32, device=dev)
        first = float(trainer.step_features(feat, B, cnt_dev))
        ms = timed(lambda: trainer.step_features(feat, B, cnt_dev), args.steps)
        res.update(step_features_ms=ms, step_features_ms_best=min(ms), first_loss=first)
        if not args.dropout:
            assert abs(first - res["torch_first_loss"]) < 1e-5, (first, res["torch_first_loss"])

        # one step's calls, each on its own
        split = {}

        def one(name, fn, reps=20):
            out = fn()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            split[name] = s.elapsed_time(e) / reps
            return out

        drop = None
        if args.dropout:
            drop = one("dropout2d_scale", lambda: ht.dropout2d_scale(N, int(C), args.dropout, 0, 1, 1, dev))
        acts, x = [], feat
        for i, layer in enumerate(layers):
            d = drop if i == 0 else None
            if batch:
                bn = layer.bn
                y, c, mean, invstd = one(f"convlad{i + 1}_forward", lambda: ht.cbr_forward_batch(
                    x, layer.conv.weight, bn.weight, bn.bias, bn.eps, slope, d, (bn.running_mean, bn.running_var), bn.momentum))
                acts.append((x, y, c, (None, None, mean, invstd)))
                x = y
            else:
                vec = ht.bn_vectors(layer.bn)
                y, c = one(f"convlad{i + 1}_forward", lambda: ht.cbr_forward(x, layer.conv.weight, vec[0], vec[1], slope))
                acts.append((x, y, c, vec))
                x = y if d is None else y * d[:, :, None, None]
        nw, nc = head.netvlad.conv.weight, head.netvlad.centroids
        vlad, saved = one("netvlad_forward", lambda: vt.netvlad_forward(x, nw, nc))
        loss, dvlad, _ = one("triplet_loss", lambda: vt.triplet_margin_loss(vlad, B, cnt_dev, 0.1))
        one("netvlad_backward", lambda: vt.netvlad_backward(x, nw, nc, saved, dvlad))
        dy = one("netvlad_backward_input", lambda: ht.netvlad_backward_input(x, nw, nc, saved, dvlad))
        for i in (2, 1, 0):
            lx, ly, lc, (scale, _, mean, invstd) = acts[i]
            g = dy
            d = drop if i == 0 else None
            name = f"convlad{i + 1}_backward" + ("" if i else "_no_dx")
            if batch:
                out = one(name, lambda: ht.cbr_backward_batch(lx, layers[i].conv.weight, layers[i].bn.weight, mean, invstd, ly, lc, g,
                                                              slope, d, need_dx=i > 0))
            else:
                if d is not None:
                    g = g * d[:, :, None, None]
                out = one(name, lambda: ht.cbr_backward(lx, layers[i].conv.weight, scale, mean, invstd, ly, lc, g, slope, need_dx=i > 0))
            dy = out[3]
        p = torch.zeros_like(out[0]).view(-1)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        one("adam_conv_weight", lambda: vt.adam_step(p, out[0].view(-1), m, v, 1))
        res["split_ms"] = split

    if args.merge_into:
        args.out = args.merge_into
        whole = json.load(open(args.out)) if os.path.exists(args.out) else {}
        whole[args.label or f"{args.bn}_dropout_{args.dropout}_{res['commit']}"] = res
        res = whole
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
