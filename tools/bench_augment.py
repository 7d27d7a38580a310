"""Time the on-device view pairs (nano_vs_slam_amd.augment) against the plain torch formulation on the same device.

    python3 tools/bench_augment.py [--N 64] [--H 240] [--W 320] [--d_f 4] [--steps 50] [--out profiles/augment.json]
                                   [--label NAME] [--commit NAME]

view_pair: N frames of H x W with uint8 labels and float32 depth at the frames' size -> image, image_aug, seg, seg_aug, depth,
depth_aug (targets at 1 / d_f) from given homographies (the sampler is timed on its own).  Baseline: the same batch by torch on the same device from the
same float32 homographies: the normalised grid (linspace, one batched 3 x 3 product, the division), grid_sample(nearest,
zeros, align_corners=True) three times (the labels through float32, as the reference does), `* 2 - 1`, and the nearest
resizes as strided slices.  The baseline forms its grid in float32, so a few of its nearest decisions differ from the device's
double arithmetic; the share of differing pixels is recorded, not gated.
cross_view_mse: forward and both gradients at [N, H / 2, W / 2] against torch autograd through grid_sample(nearest) and
F.mse_loss.  step_pair_features: a config-S depth model on 8 pairs of H x W frames, beside two step_features calls (the two
views without the cross term); there is no torch counterpart of that step in this tool.
HIP-event time per call over a window of back-to-back calls after a warm-up, three repeats; all three are recorded.  Nothing
is gated on the result; the file is where the numbers go.
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
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--H", type=int, default=240)
    ap.add_argument("--W", type=int, default=320)
    ap.add_argument("--d_f", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=8, help="pairs of the step_pair_features timing")
    ap.add_argument("--commit", default="", help="recorded when the tree is not a git checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment.json"))
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from nano_vs_slam_amd import augment as ag, depth_training as dt
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import KP2DTinyV2, get_config
    from oracle.weights import spread_state_dict, synthetic_frames

    dev = "cuda:0"
    N, H, W, d_f = args.N, args.H, args.W, args.d_f
    rng = np.random.default_rng(5)
    frames = torch.from_numpy(rng.random((N, 3, H, W)).astype(np.float32)).to(dev)
    labels = torch.from_numpy(rng.integers(0, 28, (N, H, W)).astype(np.uint8)).to(dev)
    depth = torch.from_numpy((0.05 + rng.random((N, H, W))).astype(np.float32)).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "frames": N, "H": H, "W": W, "d_f": d_f, "steps_per_window": args.steps,
           "commit": subprocess.run(["git", "describe", "--always", "--dirty"], cwd=ROOT, capture_output=True,
                                    text=True).stdout.strip() or args.commit or "unknown"}

    # ---- view_pair ----
    hom = ag.sample_homographies(N, (H, W), seed=0, step=0, device=dev)
    ms = timed(lambda: ag.sample_homographies(N, (H, W), seed=0, step=0, device=dev), args.steps)
    res.update(sample_homographies_ms=ms, sample_homographies_ms_best=min(ms))

    def grid_of(hom, h, w):
        ys, xs = torch.meshgrid(torch.linspace(-1, 1, h, device=dev), torch.linspace(-1, 1, w, device=dev), indexing="ij")
        pts = torch.stack([xs, ys, torch.ones_like(xs)], -1).reshape(1, h * w, 3)
        q = pts @ hom.transpose(1, 2)
        return (q[..., :2] / q[..., 2:]).reshape(-1, h, w, 2)

    def torch_pair():
        g = grid_of(hom, H, W)
        ws = lambda t: F.grid_sample(t, g, mode="nearest", padding_mode="zeros", align_corners=True)
        lab, dep = labels[:, None].float(), depth[:, None]
        return {"image": frames * 2.0 - 1.0, "image_aug": ws(frames) * 2.0 - 1.0, "seg": lab[:, 0, ::d_f, ::d_f].contiguous(),
                "seg_aug": ws(lab)[:, 0, ::d_f, ::d_f].contiguous(), "depth": dep[:, 0, ::d_f, ::d_f].contiguous(),
                "depth_aug": ws(dep)[:, 0, ::d_f, ::d_f].contiguous(), "homography": hom}

    ours = ag.view_pair(frames, seg=labels, depth=depth, d_f=d_f, homography=hom)
    theirs = torch_pair()
    res["pixels_differing_from_float32_grid"] = {k: float((ours[k].float() != theirs[k].float()).float().mean())
                                                 for k in ("image_aug", "seg_aug", "depth_aug")}
    assert torch.equal(ours["image"], theirs["image"]) and torch.equal(ours["seg"].float(), theirs["seg"])
    ms = timed(lambda: ag.view_pair(frames, seg=labels, depth=depth, d_f=d_f, homography=hom), args.steps)      # the sampler: timed above
    res.update(view_pair_ms=ms, view_pair_ms_best=min(ms))
    ms = timed(torch_pair, args.steps)
    res.update(torch_view_pair_ms=ms, torch_view_pair_ms_best=min(ms))

    # ---- cross_view_mse ----
    h2, w2 = H // 2, W // 2
    p = torch.from_numpy(rng.random((N, h2, w2)).astype(np.float32)).to(dev)
    pa = torch.from_numpy(rng.random((N, h2, w2)).astype(np.float32)).to(dev)
    first = float(ag.cross_view_mse(p, pa, hom)[0])
    ms = timed(lambda: ag.cross_view_mse(p, pa, hom), args.steps)
    res.update(cross_view_mse_ms=ms, cross_view_mse_ms_best=min(ms), cross_view_loss=first, cross_view_shape=[N, h2, w2])
    ms = timed(lambda: ag.warp_backward(pa, hom, (h2, w2)), args.steps)
    res.update(warp_backward_ms=ms, warp_backward_ms_best=min(ms))

    def torch_cross():
        a, b = p.detach().requires_grad_(True), pa.detach().requires_grad_(True)
        warped = F.grid_sample(a[:, None], grid_of(hom, h2, w2), mode="nearest", padding_mode="zeros", align_corners=True)[:, 0]
        loss = 0.5 * F.mse_loss(b, warped)
        loss.backward()
        return loss.detach()

    res["torch_cross_view_loss"] = float(torch_cross())
    ms = timed(torch_cross, args.steps)
    res.update(torch_cross_view_ms=ms, torch_cross_view_ms_best=min(ms))

    # ---- step_pair_features ----
    model = KP2DTinyV2(**get_config("S", to_mcu=False, v3=False), nClasses=28, depth=True)
    sd = spread_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(dev).eval()
    model.training = False
    model.set_precision("fp32")
    B = args.pairs
    f8 = (torch.from_numpy(synthetic_frames(B, H, W, seed=5)).to(dev) + 1.0) * 0.5
    batch = ag.view_pair(f8, depth=depth[:B], d_f=2, seed=0, step=0)
    with torch.no_grad():
        maps, maps_aug = model.backbone_maps(batch["image"]), model.backbone_maps(batch["image_aug"])
    trainer = dt.DepthHeadTrainer(model, lr=1e-4)
    step = lambda: trainer.step_pair_features(maps, maps_aug, batch["depth"], batch["depth_aug"], batch["homography"])
    res["step_pair_first_loss"] = float(step())
    ms = timed(step, args.steps)
    res.update(step_pair_features_ms=ms, step_pair_features_ms_best=min(ms), pairs=B)

    def two_steps():
        trainer.step_features(maps[0], maps[1], batch["depth"])
        return trainer.step_features(maps_aug[0], maps_aug[1], batch["depth_aug"])

    ms = timed(two_steps, args.steps)
    res.update(two_step_features_ms=ms, two_step_features_ms_best=min(ms))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    whole = json.load(open(args.out)) if os.path.exists(args.out) else {}
    whole[args.label or f"{H}x{W}"] = res
    with open(args.out, "w") as f:
        json.dump(whole, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
