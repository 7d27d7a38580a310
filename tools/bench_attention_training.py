"""Time one attention-head training step (AttentionSegHeadTrainer.step_features) against the plain torch formulation on the
same device.

    python3 tools/bench_attention_training.py [--N 8] [--H 240] [--W 320] [--config S_A] [--classes 28] [--steps 50]
                                              [--out profiles/attention_training.json] [--label NAME] [--commit NAME]

Inputs: config S_A on 8 synthetic frames of 240 x 320 (x 60 x 80, skip 120 x 160; 28 classes, about one label in ten ignored);
--H 120 --W 160 gives x 30 x 40 and skip 60 x 80.  The two backbone maps come from model.backbone_maps once and are not part
of the timing.  A result goes under --label (default "HxW") into the JSON file, beside what the file already holds.
Device path, train="head": five CBR forwards, two attention modules (ten stage calls each), pooling, two shuffle +
concatenations, the last layer, the loss, all of that backwards, 47 Adam updates.  `split_ms` times calls of one step on their
own (HIP events around the call, the mean of 20): each module's forward and backward as a whole, and its attention forward and
attention backward apart.
Baseline: the head restated in plain torch (F.conv2d, F.batch_norm on the running statistics, the reference's LayerNorm
expression, softmax attention by matmul, F.gelu) + autograd + F.cross_entropy and the Dice loss written out + torch.optim.Adam
over the 47 parameters, on the same device.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_seg_training import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--H", type=int, default=240)
    ap.add_argument("--W", type=int, default=320)
    ap.add_argument("--config", default="S_A")
    ap.add_argument("--classes", type=int, default=28)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--commit", default="", help="recorded when the tree is not a git checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_training.json"))
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from nano_vs_slam_amd import attention_training as at, seg_training as st, train_ops as ops
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    from oracle.weights import spread_state_dict, synthetic_frames

    dev = "cuda:0"
    model = tiny_factory(args.config, args.classes)
    sd = spread_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(dev).eval()
    model.training = False
    model.set_precision("fp32")
    N, Cn = args.N, args.classes
    frames = torch.from_numpy(synthetic_frames(N, args.H, args.W, seed=5)).to(dev)
    with torch.no_grad():
        x, skip = model.backbone_maps(frames)
    rng = np.random.default_rng(5)
    lab = rng.integers(0, Cn, (N, skip.shape[2], skip.shape[3])).astype(np.uint8)
    lab[rng.random(lab.shape) < 0.1] = 255
    labels = torch.from_numpy(lab).to(dev)
    labels64 = labels.long()
    convs = list(model.seg_head.convs)
    slope = 0.01 if model.leaky_relu else 0.0
    res = {"device": torch.cuda.get_device_name(0), "config": args.config, "frames": N, "H": args.H, "W": args.W, "classes": Cn,
           "x": list(x.shape), "skip": list(skip.shape), "lr": 1e-4, "ce_weight": 0.5, "dice_weight": 1.5, "steps_per_window": args.steps,
           "commit": subprocess.run(["git", "describe", "--always", "--dirty"], cwd=ROOT, capture_output=True,
                                    text=True).stdout.strip() or args.commit or "unknown"}

    # ---- the plain torch formulation, on copies of the parameters -------------------------------------------------------------
    tp = [torch.nn.Parameter(p.detach().clone()) for p in model.seg_head.parameters()]
    stats = {i: (convs[i].bn.running_mean.detach().clone(), convs[i].bn.running_var.detach().clone(), convs[i].bn.eps) for i in (0, 3, 4, 5, 6)}
    slot = {0: 0, 3: 33, 4: 36, 5: 39, 6: 42}

    def cbr(i, v):
        w, g, b = tp[slot[i]:slot[i] + 3]
        v = F.batch_norm(F.conv2d(v, w, padding=1), stats[i][0], stats[i][1], g, b, training=False, eps=stats[i][2])
        return F.leaky_relu(v, slope) if slope else F.relu(v)

    def ln(v, g, b):
        return (v - v.mean(dim=1, keepdim=True)) / (torch.var(v, dim=1, unbiased=False, keepdim=True).sqrt() + 1e-5) * g + b

    def module(v, p):
        n, c, h, w = v.shape
        t = ln(v, p[3], p[4])
        q, kv = F.conv2d(t, p[0]), F.conv2d(t, p[1], stride=2)
        heads = lambda m: m.reshape(n, 4, c // 4, -1).transpose(2, 3)
        sim = heads(q) @ heads(kv[:, :c]).transpose(2, 3) * (c // 4) ** -0.5
        o = (sim.softmax(dim=-1) @ heads(kv[:, c:])).transpose(2, 3).reshape(n, c, h, w)
        t = ln(F.conv2d(o, p[2]), p[13], p[14])
        t = F.conv2d(F.conv2d(F.conv2d(t, p[5], p[6]), p[7], p[8], padding=1, groups=2 * c), p[9], p[10])
        return F.conv2d(F.gelu(t), p[11], p[12])

    def torch_logits():
        s = module(cbr(0, x), tp[3:18])
        s = cbr(3, module(F.max_pool2d(s, 2, 2), tp[18:33]))
        s = cbr(5, cbr(4, torch.cat([F.pixel_shuffle(s, 2), x], dim=1)))
        s = cbr(6, torch.cat([F.pixel_shuffle(s, 2), skip], dim=1))
        return F.conv2d(s, tp[45], tp[46], padding=1)

    def torch_loss(z):
        ce = F.cross_entropy(z, labels64, ignore_index=255)
        mask = labels64 != 255
        p = torch.softmax(z, dim=1) * mask[:, None]
        t = F.one_hot(torch.where(mask, labels64, 0), Cn).permute(0, 3, 1, 2).to(z.dtype) * mask[:, None]
        inter, card = (p * t).sum(dim=(0, 2, 3)), (p + t).sum(dim=(0, 2, 3))
        dice = ((1 - 2 * inter / card.clamp_min(1e-7)) * (t.sum(dim=(0, 2, 3)) > 0)).sum() / Cn
        return 0.5 * ce + 1.5 * dice

    opt = torch.optim.Adam(tp, lr=1e-4)

    def torch_step():
        opt.zero_grad()
        loss = torch_loss(torch_logits())
        loss.backward()
        opt.step()
        return loss.detach()

    res["torch_head_first_loss"] = float(torch_step())
    ms = timed(torch_step, args.steps)
    res.update(torch_head_ms=ms, torch_head_ms_best=min(ms))

    # ---- the device path ------------------------------------------------------------------------------------------------------
    keep = [p.detach().clone() for p in model.seg_head.parameters()]
    head = at.AttentionSegHeadTrainer(model, lr=1e-4, train="head")
    first = float(head.step_features(x, skip, labels))
    ms = timed(lambda: head.step_features(x, skip, labels), args.steps)
    res.update(head_step_features_ms=ms, head_step_features_ms_best=min(ms), head_first_loss=first)
    assert abs(first - res["torch_head_first_loss"]) < 1e-4, (first, res["torch_head_first_loss"])
    with torch.no_grad():
        for p, k in zip(model.seg_head.parameters(), keep):
            p.copy_(k)

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

    vec = ops.bn_vectors(convs[0].bn)
    y0 = ops.cbr_forward(x, convs[0].conv.weight, vec[0], vec[1], slope)[0]
    v = y0
    for i in (1, 2):
        y, saved = one(f"module{i}_forward", lambda: ops.attention_module_forward(convs[i], v))
        one(f"module{i}_attention_forward", lambda: ops.attention_forward(saved["q"], saved["kv"]))
        dy = torch.randn_like(y)
        one(f"module{i}_backward", lambda: ops.attention_module_backward(convs[i], saved, dy))
        one(f"module{i}_attention_backward", lambda: ops.attention_backward(saved["q"], saved["kv"], saved["o"], saved["lse"], dy))
        res[f"module{i}_map"] = list(v.shape)
        v = st.maxpool2_forward(y)
    res["split_ms"] = split

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    whole = json.load(open(args.out)) if os.path.exists(args.out) else {}
    whole[args.label or f"{args.H}x{args.W}"] = res
    with open(args.out, "w") as f:
        json.dump(whole, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
