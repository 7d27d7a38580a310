"""Time the keypoint loss (keypoint_loss) and one keypoint-head training step (KeypointHeadTrainer.step_features) against the
plain torch formulation on the same device.

    python3 tools/bench_keypoint_training.py [--B 8] [--H 240] [--W 320] [--config S] [--steps 50]
                                             [--out profiles/keypoint_training.json] [--label NAME] [--commit NAME]

Inputs: config S on 8 synthetic pairs of 240 x 320 from synthetic.homography_pairs (60 x 80 cells, n = 4524 interior cells,
32 descriptor channels at 120 x 160).  The backbone maps of both views come from model.backbone_maps once and are not part
of the timing: both sides start from them, the backbone is frozen.  A result goes under --label (default "HxW") into the
JSON file, beside what the file already holds.
Device path: the three heads' forward on the 2 B frames, the loss, all of that backwards, 20 Adam updates.  `split_ms` times
each call of one step on its own (HIP events around the call, the mean of 20), which adds up to more than the step where the
calls overlap the host's launch work.
Baseline: the loss restated with dense torch operations (torch.cdist and min for the nearest target, one n x n matrix product
per pair, F.grid_sample, F.triplet_margin_loss) under autograd, and for the step the heads restated with F.conv2d,
F.batch_norm on the running statistics, F.leaky_relu, F.pixel_shuffle and torch.cat, with torch.optim.Adam over the 20
parameters, on the same device.
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


def torch_keypoint_loss(out, aug, hom, H, W, cell, weights=(1.0, 2.0, 1.0, 1.0), relax=4.0, cross_ratio=2.0):
    """The loss of include/kp2d.h with dense torch operations -> (loss, recall)"""
    import torch
    import torch.nn.functional as F
    lw, dw, sw, kw = weights
    B, _, Hc, Wc = out["score"].shape
    dev = out["score"].device
    mask = torch.zeros(Hc, Wc, dtype=torch.bool, device=dev)
    mask[1:-1, 1:-1] = True
    flat = mask.flatten()
    step = (cell - 1) / 2.0
    ys, xs = torch.meshgrid(torch.arange(Hc, device=dev, dtype=torch.float32), torch.arange(Wc, device=dev, dtype=torch.float32), indexing="ij")
    base = torch.stack([xs, ys]) * cell + step

    def decode(shift):
        u = base + shift * (cross_ratio * step)
        return torch.stack([u[:, 0].clamp(0, W - 1), u[:, 1].clamp(0, H - 1)], -1).reshape(B, -1, 2)

    def norm(c):
        return torch.stack([c[..., 0] / ((W - 1) / 2.0) - 1.0, c[..., 1] / ((H - 1) / 2.0) - 1.0], -1)

    ct, cs = decode(out["coord"]), decode(aug["coord"])
    st, ss = out["score"] * mask, aug["score"] * mask
    sn = norm(cs)
    p = sn @ hom[:, :, :2].transpose(1, 2) + hom[:, None, :, 2]
    wn = p[..., :2] / p[..., 2:]
    w = torch.stack([(wn[..., 0] + 1.0) * ((W - 1) / 2.0), (wn[..., 1] + 1.0) * ((H - 1) / 2.0)], -1)
    d, a = torch.cdist(w, ct).min(dim=2)
    valid = (d < 4.0) & flat
    dv = d[valid]
    S = (st.flatten(1).gather(1, a) + ss.flatten(1))[valid]
    loc = dv.mean()
    usp = (S * (dv - dv.mean())).mean()
    res = F.grid_sample(st, wn.detach().reshape(B, Hc, Wc, 2), mode="bilinear", align_corners=True)
    con = 2.0 * F.mse_loss(res[:, :, mask], ss[:, :, mask])
    metric, hits = 0.0, 0
    n = int(flat.sum())
    for b in range(B if n >= 20 else 0):
        ref = F.grid_sample(aug["feat"][b:b + 1], sn[b].detach().reshape(1, Hc, Wc, 2), align_corners=True)[0][:, mask]
        tar = F.grid_sample(out["feat"][b:b + 1], wn[b].detach().reshape(1, Hc, Wc, 2), align_corners=True)[0][:, mask]
        ref = ref / (torch.norm(ref + 1e-8, dim=0) + 1e-8)
        tar = tar / (torch.norm(tar + 1e-8, dim=0) + 1e-8)
        dm = torch.sqrt(2.0 - 2.0 * torch.clamp(ref.t() @ tar, -1.0, 1.0) + 1e-8).detach()
        wk = w[b][flat].detach()
        within = ((wk[None, :, 0] - wk[:, None, 0]).abs() <= relax) & ((wk[None, :, 1] - wk[:, None, 1]).abs() <= relax)
        best = dm.argmin(dim=1)
        neg = torch.where(within.all(dim=1), best, dm.masked_fill(within, float("inf")).argmin(dim=1))
        hits = hits + (wk[best] == wk).all(dim=1).sum()
        metric = metric + F.triplet_margin_loss(ref.t(), tar.t(), tar[:, neg].t(), margin=0.2) / B
    loss = kw * (lw * loc + dw * 2.0 * metric + sw * usp + sw * con)
    return loss, hits / float(max(B * n, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=240)
    ap.add_argument("--W", type=int, default=320)
    ap.add_argument("--config", default="S")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--commit", default="", help="recorded when the tree is not a git checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoint_training.json"))
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from nano_vs_slam_amd import keypoint_training as kt, seg_training as st, vlad_training as vt, vpr_head_training as ht
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    from nano_vs_slam_amd.synthetic import homography_pairs
    from oracle.weights import spread_state_dict

    dev = "cuda:0"
    model = tiny_factory(args.config, 28)
    sd = spread_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(dev).eval()
    model.training = False
    model.set_precision("fp32")
    B, H, W = args.B, args.H, args.W
    frames, hom, warped = homography_pairs(B, H, W, seed=5, device=dev)
    hn = kt.normalized_homography(hom, H, W, invert=True)
    with torch.no_grad():
        maps, maps_aug = model.backbone_maps(frames), model.backbone_maps(warped)
    x2, skip2 = torch.cat([maps[0], maps_aug[0]]), torch.cat([maps[1], maps_aug[1]])
    slope = 0.01 if model.leaky_relu else 0.0
    res = {"device": torch.cuda.get_device_name(0), "config": args.config, "pairs": B, "H": H, "W": W, "x": list(maps[0].shape),
           "skip": list(maps[1].shape), "lr": 1e-4, "steps_per_window": args.steps,
           "commit": subprocess.run(["git", "describe", "--always", "--dirty"], cwd=ROOT, capture_output=True,
                                    text=True).stdout.strip() or args.commit or "unknown"}

    # ---- the plain torch formulation, on copies of the parameters (before the device path moves the model's own)
    trainer = kt.KeypointHeadTrainer(model, lr=1e-4)
    names = [n for n, p in model.named_parameters() if any(p is q for q in trainer.parameters())]
    tp = {n: torch.nn.Parameter(p.detach().clone()) for n, p in zip(names, trainer.parameters())}

    def cbr(prefix, bn, v):
        v = F.batch_norm(F.conv2d(v, tp[prefix + ".conv.weight"], padding=1), bn.running_mean, bn.running_var, tp[prefix + ".bn.weight"],
                         tp[prefix + ".bn.bias"], training=False, eps=bn.eps)
        return F.leaky_relu(v, slope) if slope else F.relu(v)

    def torch_heads(x, skip):
        m = model
        score = torch.sigmoid(F.conv2d(cbr("score_head.convDa", m.score_head.convDa.bn, x), tp["score_head.convDb.weight"], tp["score_head.convDb.bias"], padding=1))
        shift = torch.tanh(F.conv2d(cbr("loc_head.convDa", m.loc_head.convDa.bn, x), tp["loc_head.convDb.weight"], tp["loc_head.convDb.bias"], padding=1))
        up = F.conv2d(cbr("desc_head.convA", m.desc_head.convA.bn, x), tp["desc_head.convB.weight"], tp["desc_head.convB.bias"], padding=1)
        cat = torch.cat([F.pixel_shuffle(up, 2), skip], dim=1)
        feat = F.conv2d(cbr("desc_head.confAa", m.desc_head.confAa.bn, cat), tp["desc_head.confBb.weight"], tp["desc_head.confBb.bias"], padding=1)
        return {"score": score, "coord": shift, "feat": feat}

    opt = torch.optim.Adam(list(tp.values()), lr=1e-4)

    def torch_step():
        opt.zero_grad()
        o = torch_heads(x2, skip2)
        loss, _ = torch_keypoint_loss({k: v[:B] for k, v in o.items()}, {k: v[B:] for k, v in o.items()}, hn, H, W, model.cell)
        loss.backward()
        opt.step()
        return loss.detach()

    with torch.no_grad():
        outs = {k: v.clone() for k, v in trainer.forward_features(x2, skip2).items()}
    out, aug = {k: v[:B] for k, v in outs.items()}, {k: v[B:] for k, v in outs.items()}

    def torch_loss_only():
        o = {k: v.detach().requires_grad_(True) for k, v in out.items()}
        a = {k: v.detach().requires_grad_(True) for k, v in aug.items()}
        loss, recall = torch_keypoint_loss(o, a, hn, H, W, model.cell)
        loss.backward()
        return loss.detach(), recall

    l0, r0 = torch_loss_only()
    res.update(torch_loss_value=float(l0), torch_recall=float(r0))
    ms = timed(torch_loss_only, args.steps)
    res.update(torch_loss_ms=ms, torch_loss_ms_best=min(ms))
    res["torch_step_first_loss"] = float(torch_step())
    ms = timed(torch_step, args.steps)
    res.update(torch_step_ms=ms, torch_step_ms_best=min(ms))

    # ---- the device path
    size = (H, W)
    loss, _, stats = kt.keypoint_loss(out, aug, hn, size, model.cell)
    res.update(loss_value=float(loss), recall=float(stats["recall"]), valid=int(stats["valid"]), anchors=int(stats["anchors"]))
    assert abs(res["loss_value"] - res["torch_loss_value"]) < 1e-3 * abs(res["torch_loss_value"]), (res["loss_value"], res["torch_loss_value"])
    ms = timed(lambda: kt.keypoint_loss(out, aug, hn, size, model.cell), args.steps)
    res.update(keypoint_loss_ms=ms, keypoint_loss_ms_best=min(ms))
    first = float(trainer.step_features(maps, maps_aug, hn, size))
    ms = timed(lambda: trainer.step_features(maps, maps_aug, hn, size), args.steps)
    res.update(step_features_ms=ms, step_features_ms_best=min(ms), step_first_loss=first)
    assert abs(first - res["torch_step_first_loss"]) < 1e-3 * abs(first), (first, res["torch_step_first_loss"])

    # ---- one step's calls, each on its own
    split = {}

    def one(name, fn, reps=20):
        val = fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        split[name] = s.elapsed_time(e) / reps
        return val

    m = model
    acts = {}

    def fwd(name, layer, v):
        vec = ht.bn_vectors(layer.bn)
        y, c = one(name + "_forward", lambda: ht.cbr_forward(v, layer.conv.weight, vec[0], vec[1], slope))
        acts[name] = (v, y, c, vec)
        return y

    def back(name, layer, dy, need_dx):
        lx, ly, lc, (scale, _, mean, invstd) = acts[name]
        return one(name + "_backward", lambda: ht.cbr_backward(lx, layer.conv.weight, scale, mean, invstd, ly, lc, dy, slope, need_dx=need_dx))

    ys = fwd("score_convDa", m.score_head.convDa, x2)
    zs = one("score_convDb_forward", lambda: st.conv_bias_forward(ys, m.score_head.convDb.weight, m.score_head.convDb.bias))
    yl = fwd("loc_convDa", m.loc_head.convDa, x2)
    zl = one("loc_convDb_forward", lambda: st.conv_bias_forward(yl, m.loc_head.convDb.weight, m.loc_head.convDb.bias))
    ya = fwd("desc_convA", m.desc_head.convA, x2)
    up = one("desc_convB_forward", lambda: st.conv_bias_forward(ya, m.desc_head.convB.weight, m.desc_head.convB.bias))
    cat = one("shuffle_cat_forward", lambda: st.shuffle_cat_forward(up, skip2))
    yb = fwd("desc_confAa", m.desc_head.confAa, cat)
    feat = one("desc_confBb_forward", lambda: st.conv_bias_forward(yb, m.desc_head.confBb.weight, m.desc_head.confBb.bias))
    o = {"score": torch.sigmoid(zs), "coord": torch.tanh(zl), "feat": feat}
    _, g, _ = one("keypoint_loss", lambda: kt.keypoint_loss({k: v[:B] for k, v in o.items()}, {k: v[B:] for k, v in o.items()}, hn, size, m.cell))
    gz = {k: torch.cat([g["out"][k], g["out_aug"][k]]) for k in ("score", "coord", "feat")}
    _, _, dy = one("score_convDb_backward", lambda: st.conv_bias_backward(ys, m.score_head.convDb.weight, gz["score"] * o["score"] * (1 - o["score"])))
    back("score_convDa", m.score_head.convDa, dy, False)
    _, _, dy = one("loc_convDb_backward", lambda: st.conv_bias_backward(yl, m.loc_head.convDb.weight, gz["coord"] * (1 - o["coord"] ** 2)))
    back("loc_convDa", m.loc_head.convDa, dy, False)
    _, _, dy = one("desc_confBb_backward", lambda: st.conv_bias_backward(yb, m.desc_head.confBb.weight, gz["feat"]))
    dcat = back("desc_confAa", m.desc_head.confAa, dy, True)[3]
    dup = one("shuffle_cat_backward", lambda: st.shuffle_cat_backward(dcat, m.desc_head.convB.weight.shape[0] // 4))
    dwb, _, dy = one("desc_convB_backward", lambda: st.conv_bias_backward(ya, m.desc_head.convB.weight, dup))
    back("desc_convA", m.desc_head.convA, dy, False)
    p0 = m.desc_head.convB.weight
    mom, var = torch.zeros_like(p0.data), torch.zeros_like(p0.data)
    one("adam_step_convB", lambda: vt.adam_step(p0.data, dwb, mom, var, 1, 0.0))
    res["split_ms"] = split
    res["split_sum_ms"] = sum(split.values())

    label = args.label or f"{H}x{W}"
    data = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            data = json.load(f)
    data[label] = res
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
