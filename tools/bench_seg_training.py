"""Time one segmentation-head training step (SegHeadTrainer.step_features) against the plain torch formulation on the same
device.

    python3 tools/bench_seg_training.py [--N 8] [--H 240] [--W 320] [--config S] [--classes 28] [--steps 50]
                                        [--out profiles/seg_training.json] [--label NAME] [--commit NAME]

Inputs: config S on 8 synthetic frames of 240 x 320 (config S halves twice: x 60 x 80, skip 120 x 160; 28 classes, about one
label in ten ignored); --H 120 --W 160 gives x 30 x 40 and skip 60 x 80.  The two backbone maps come from
model.backbone_maps once and are not part of the timing: both sides start from them, the backbone is frozen.  A result goes
under --label (default "HxW") into the JSON file, beside what the file already holds.
Device path, train="head": eight CBR forwards, pooling, two shuffle + concatenations, the last layer, the loss, and all of
that backwards, 26 Adam updates; train="last": the last layer forward, the loss, its backward without dx and two Adam updates,
on the last layer's input taken from the "head" forward.  `split_ms` times each call of one "head" step on its own (HIP events
around the call, the mean of 20), which adds up to more than the step where the calls overlap the host's launch work.
Baseline: a restated head (F.conv2d, F.batch_norm on the running statistics, F.leaky_relu, F.max_pool2d, F.pixel_shuffle,
torch.cat) + torch autograd + F.cross_entropy(ignore_index=255) and the Dice loss written out + torch.optim.Adam over the 26
(or 2) parameters, on the same device.
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
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--H", type=int, default=240)
    ap.add_argument("--W", type=int, default=320)
    ap.add_argument("--config", default="S")
    ap.add_argument("--classes", type=int, default=28)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--commit", default="", help="recorded when the tree is not a git checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_training.json"))
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from nano_vs_slam_amd import seg_training as st, vlad_training as vt, vpr_head_training as ht
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

    # the plain torch formulation, on copies of the parameters (before the device path moves the model's own)
    cw = [torch.nn.Parameter(l.conv.weight.detach().clone()) for l in convs[:8]]
    gam = [torch.nn.Parameter(l.bn.weight.detach().clone()) for l in convs[:8]]
    bet = [torch.nn.Parameter(l.bn.bias.detach().clone()) for l in convs[:8]]
    stats = [(l.bn.running_mean.detach().clone(), l.bn.running_var.detach().clone(), l.bn.eps) for l in convs[:8]]
    w8, b8 = torch.nn.Parameter(convs[8].weight.detach().clone()), torch.nn.Parameter(convs[8].bias.detach().clone())

    def cbr(i, v):
        v = F.batch_norm(F.conv2d(v, cw[i], padding=1), stats[i][0], stats[i][1], gam[i], bet[i], training=False, eps=stats[i][2])
        return F.leaky_relu(v, slope) if slope else F.relu(v)

    def torch_trunk():
        s = F.max_pool2d(cbr(1, cbr(0, x)), 2, 2)
        s = torch.cat([F.pixel_shuffle(cbr(4, cbr(3, cbr(2, s))), 2), x], dim=1)
        s = torch.cat([F.pixel_shuffle(cbr(6, cbr(5, s)), 2), skip], dim=1)
        return cbr(7, s)

    def torch_loss(z):
        ce = F.cross_entropy(z, labels64, ignore_index=255)
        mask = labels64 != 255
        p = torch.softmax(z, dim=1) * mask[:, None]
        t = F.one_hot(torch.where(mask, labels64, 0), Cn).permute(0, 3, 1, 2).to(z.dtype) * mask[:, None]
        inter, card = (p * t).sum(dim=(0, 2, 3)), (p + t).sum(dim=(0, 2, 3))
        dice = ((1 - 2 * inter / card.clamp_min(1e-7)) * (t.sum(dim=(0, 2, 3)) > 0)).sum() / Cn
        return 0.5 * ce + 1.5 * dice

    opt_head = torch.optim.Adam([t for trio in zip(cw, gam, bet) for t in trio] + [w8, b8], lr=1e-4)

    def torch_step_head():
        opt_head.zero_grad()
        loss = torch_loss(F.conv2d(torch_trunk(), w8, b8, padding=1))
        loss.backward()
        opt_head.step()
        return loss.detach()

    with torch.no_grad():
        feat_t = torch_trunk().clone()      # the last layer's input of the untrained head: what "last" mode starts from
    w8l, b8l = torch.nn.Parameter(w8.detach().clone()), torch.nn.Parameter(b8.detach().clone())
    opt_last = torch.optim.Adam([w8l, b8l], lr=1e-4)

    def torch_step_last():
        opt_last.zero_grad()
        loss = torch_loss(F.conv2d(feat_t, w8l, b8l, padding=1))
        loss.backward()
        opt_last.step()
        return loss.detach()

    res["torch_last_first_loss"] = float(torch_step_last())
    ms = timed(torch_step_last, args.steps)
    res.update(torch_last_ms=ms, torch_last_ms_best=min(ms))
    res["torch_head_first_loss"] = float(torch_step_head())
    ms = timed(torch_step_head, args.steps)
    res.update(torch_head_ms=ms, torch_head_ms_best=min(ms))

    # the device path; "last" first, on the untrained head's last-layer input, then "head" on the same starting weights but
    # for the last layer's few steps
    keep = [p.detach().clone() for p in model.seg_head.parameters()]
    head = st.SegHeadTrainer(model, lr=1e-4, train="head")
    feat = head._forward(x, skip)[1]["feat"].clone()
    last = st.SegHeadTrainer(model, lr=1e-4, train="last")
    first = float(last.step_features(feat, None, labels))
    ms = timed(lambda: last.step_features(feat, None, labels), args.steps)
    res.update(last_step_features_ms=ms, last_step_features_ms_best=min(ms), last_first_loss=first)
    assert abs(first - res["torch_last_first_loss"]) < 1e-4, (first, res["torch_last_first_loss"])
    with torch.no_grad():
        for p, k in zip(model.seg_head.parameters(), keep):
            p.copy_(k)
    first = float(head.step_features(x, skip, labels))
    ms = timed(lambda: head.step_features(x, skip, labels), args.steps)
    res.update(head_step_features_ms=ms, head_step_features_ms_best=min(ms), head_first_loss=first)
    assert abs(first - res["torch_head_first_loss"]) < 1e-4, (first, res["torch_head_first_loss"])

    # one "head" step's calls, each on its own
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

    acts = {}

    def fwd(i, v):
        vec = ht.bn_vectors(convs[i].bn)
        y, c = one(f"convs{i}_forward", lambda: ht.cbr_forward(v, convs[i].conv.weight, vec[0], vec[1], slope))
        acts[i] = (v, y, c, vec)
        return y

    y1 = fwd(1, fwd(0, x))
    pooled = one("maxpool2_forward", lambda: st.maxpool2_forward(y1))
    y4 = fwd(4, fwd(3, fwd(2, pooled)))
    cat1 = one("shuffle_cat1_forward", lambda: st.shuffle_cat_forward(y4, x))
    y6 = fwd(6, fwd(5, cat1))
    cat2 = one("shuffle_cat2_forward", lambda: st.shuffle_cat_forward(y6, skip))
    y7 = fwd(7, cat2)
    logits = one("conv_bias_forward", lambda: st.conv_bias_forward(y7, convs[8].weight, convs[8].bias))
    _, dz, _, _ = one("segmentation_loss", lambda: st.segmentation_loss(logits, labels))
    one("conv_bias_backward_no_dx", lambda: st.conv_bias_backward(y7, convs[8].weight, dz, need_dx=False))
    dw8, _, dy = one("conv_bias_backward", lambda: st.conv_bias_backward(y7, convs[8].weight, dz))

    def back(i, g, need_dx=True):
        lx, ly, lc, (scale, _, mean, invstd) = acts[i]
        return one(f"convs{i}_backward" + ("" if need_dx else "_no_dx"),
                   lambda: ht.cbr_backward(lx, convs[i].conv.weight, scale, mean, invstd, ly, lc, g, slope, need_dx=need_dx))[3]

    C4 = convs[6].conv.weight.shape[0] // 4
    dy = back(7, dy)
    dy = back(6, one("shuffle_cat2_backward", lambda: st.shuffle_cat_backward(dy, C4)))
    dy = back(5, dy)
    dy = back(4, one("shuffle_cat1_backward", lambda: st.shuffle_cat_backward(dy, C4)))
    dy = back(2, back(3, dy))
    dy = back(1, one("maxpool2_backward", lambda: st.maxpool2_backward(y1, dy)))
    back(0, dy, need_dx=False)
    p = torch.zeros_like(dw8).view(-1)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    one("adam_last_weight", lambda: vt.adam_step(p, dw8.view(-1), m, v, 1))
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
