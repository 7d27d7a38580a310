"""Generate tests/golden/depth_pair/ by running the REFERENCE's SegmentationHead with one class in .eval() followed by
.sigmoid() on both views of a pair as one batch, its SILogLoss with torch.nn.HuberLoss() per view as
KeypointNetwithIOLoss._compute_depth_loss combines them, and the cross-view term of KeypointNetwithIOLoss.py:587-603,
MSE(depth_aug, warper(depth, homography)) * 0.5, in float64 under torch autograd with torch.optim.Adam; and the same in
float32, the yardstick of the GPU test's bounds.  The modules are loaded read-only from a checkout of the reference exactly as
tools/make_depth_training_golden.py loads them.

    python3 tools/make_depth_pair_golden.py --reference PATH        (or KP2D_REFERENCE=PATH)

The warper is RESTATED, not run: torchgeometry is not a dependency, so tgm.HomographyWarper(h, w, mode="nearest")(x, H) is
written out as what it calls, grid_sample(x, H · meshgrid(-1..1), mode="nearest", padding_mode="zeros", align_corners=True),
the grid formed in the run's own precision.  A seed is kept only when every nearest decision is further than
depth_pair_ref.NEAREST_SAFE (1e-3 pixel) from a tie, so the float32 run makes the decisions of the float64 run (asserted), and
when the loss conditions of make_depth_training_golden hold for both views; refused seeds are printed.

Written: pair.npz (the loss, the five parts, every stored entry of the 26 gradients, five Adam steps' losses and parameters,
err32_* of each, settings) and seed.json.  No test, smoke() or bench.py reads the reference.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_depth_training_golden import build, reference_loss, reference_silog  # noqa: E402
from make_seg_training_golden import reference_seg_head  # noqa: E402


def warper(x, hom):
    """x [N, 1, h, w], hom [N, 3, 3] of x's dtype -> (warped, the grid)"""
    n, _, h, w = x.shape
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, h, dtype=x.dtype), torch.linspace(-1, 1, w, dtype=x.dtype), indexing="ij")
    pts = torch.stack([xs, ys, torch.ones_like(xs)], -1).reshape(1, h * w, 3).expand(n, -1, -1)
    q = pts @ hom.transpose(1, 2)
    grid = (q[..., :2] / q[..., 2:]).reshape(n, h, w, 2)
    return torch.nn.functional.grid_sample(x, grid, mode="nearest", padding_mode="zeros", align_corners=True), grid


def pair_step(head, SILog, inp, dtype, cross_weight):
    """Both views as one batch through the head -> dict(loss, parts [5], decisions); the parameters' .grad are set."""
    t = lambda k: torch.from_numpy(inp[k]).to(dtype)
    n = inp["N"]
    logits = head(torch.cat([t("x"), t("x_aug")]), torch.cat([t("skip"), t("skip_aug")]))
    plain, silog, huber, d = reference_loss(SILog, logits[:n], t("gt")[:, None], inp["weights"])
    aug, silog_aug, huber_aug, d_aug = reference_loss(SILog, logits[n:], t("gt_aug")[:, None], inp["weights"])
    parts = [silog, huber, silog_aug, huber_aug]
    pred = logits.sigmoid()
    warped, grid = warper(pred[:n], t("homography"))
    cross = torch.nn.functional.mse_loss(pred[n:], warped)
    loss = plain + aug + cross_weight * cross
    loss.backward()
    size = torch.tensor([grid.shape[2] - 1, grid.shape[1] - 1], dtype=dtype)
    return {"loss": loss.detach(), "parts": torch.stack(parts + [cross]).detach(), "decisions": torch.round((grid.detach() + 1) / 2 * size),
            "logits": logits.detach(), "d": torch.cat([d, d_aug])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("KP2D_REFERENCE"), help="a checkout of the reference project")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        raise SystemExit("needs --reference PATH (or KP2D_REFERENCE): a checkout of the reference project")
    Head, SILog = reference_seg_head(args.reference), reference_silog(args.reference)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import augment_ref as ar
    import depth_pair_ref as pr
    os.makedirs(pr.GOLDEN, exist_ok=True)

    def run(inp):
        out = {}
        for dtype in (torch.float64, torch.float32):
            head, params = build(Head, inp, dtype)
            r = pair_step(head, SILog, inp, dtype, pr.CROSS_WEIGHT)
            r["grads"] = [p.grad.clone() for p in params]
            out[dtype] = r
        return out[torch.float64], out[torch.float32]

    seed = pr.BASE_SEED
    while True:
        inp = pr.make_inputs(seed)
        margin = pr.nearest_margin(inp["homography"], 2 * pr.H8, 2 * pr.W8)
        why = None if margin > pr.NEAREST_SAFE else f"a nearest decision is {margin:.2e} pixel from a tie"
        if why is None:
            r64, r32 = run(inp)
            if not torch.equal(r64["decisions"], r32["decisions"].double()):
                why = "the float32 run rounds a coordinate the other way"
            elif float(r64["logits"].abs().max()) > 8.0:
                why = f"|logit| {float(r64['logits'].abs().max()):.3f} above 8"
            else:
                ok = np.concatenate([inp["gt"], inp["gt_aug"]]) > 0
                d64, d32 = r64["d"][:, 0].numpy()[ok], r32["d"][:, 0].numpy()[ok].astype(np.float64)
                gap, derr = float(np.abs(np.abs(d64) - 1.0).min()), float(np.abs(d32 - d64).max())
                if not gap > 100.0 * derr:
                    why = f"smallest ||d| - 1| {gap:.3e} within 100 x the float32 error of d {derr:.3e}"
        if why is None:
            break
        print(f"seed {seed} refused: {why}")
        seed += 1000
    # the oracle's decisions are the float64 run's
    near = np.stack([np.stack(np.divmod(ar.nearest(h, 2 * pr.H8, 2 * pr.W8)[1], 2 * pr.W8)[::-1], -1) for h in inp["homography"].astype(np.float64)])
    inside = np.stack([ar.nearest(h, 2 * pr.H8, 2 * pr.W8)[0] for h in inp["homography"].astype(np.float64)])
    assert np.array_equal(r64["decisions"].numpy()[inside], near[inside].astype(np.float64)), "the oracle's nearest pixels differ from grid_sample's"
    ref = ar.cross_view_mse(r64["logits"][:pr.N, 0].sigmoid().numpy(), r64["logits"][pr.N:, 0].sigmoid().numpy(), inp["homography"].astype(np.float64), 1.0)
    assert abs(ref["loss"] - float(r64["parts"][4])) <= 1e-12, "the oracle's cross-view term differs from the restated warper's"

    data = {"loss": np.float64(r64["loss"]), "parts": r64["parts"].numpy(), "seed": np.int64(seed), "cross_weight": np.float64(pr.CROSS_WEIGHT),
            "nearest_margin": np.float64(margin), "inside": np.int64(inside.sum()), "lr": np.float64(pr.LR),
            "err32_loss": np.float64(abs(float(r32["loss"]) - float(r64["loss"])) / abs(float(r64["loss"])))}
    for j, name in enumerate(pr.PARTS):
        data["err32_" + name] = np.float64(abs(float(r32["parts"][j]) - float(r64["parts"][j])) / abs(float(r64["parts"][j])))
    for i in range(26):
        data[f"g{i}"] = pr.stored(r64["grads"][i].numpy())
        data[f"err32_g{i}"] = np.float64(pr.rel_err(r32["grads"][i].numpy(), r64["grads"][i].numpy()))
    print(f"seed {seed}: loss {float(r64['loss'])!r}, parts {r64['parts'].tolist()}, inside {int(inside.sum())} of {inside.size}, "
          f"nearest margin {margin:.2e}; fp32 error: loss {float(data['err32_loss']):.1e}, gradients {max(float(data[f'err32_g{i}']) for i in range(26)):.1e}")

    runs = {}
    for dtype in (torch.float64, torch.float32):
        head, params = build(Head, inp, dtype)
        opt = torch.optim.Adam(params, lr=pr.LR)
        losses, after = [], []
        for _ in range(pr.STEPS):
            opt.zero_grad()
            losses.append(float(pair_step(head, SILog, inp, dtype, pr.CROSS_WEIGHT)["loss"]))
            opt.step()
            after.append([p.detach().numpy().copy() for p in params])
        runs[dtype] = (np.asarray(losses, np.float64), after)
    (l64, a64), (l32, a32) = runs[torch.float64], runs[torch.float32]
    data["losses_traj"] = l64
    data["err32_loss_traj"] = np.float64((np.abs(l32 - l64) / np.abs(l64)).max())
    for i in range(26):
        data[f"p{i}_traj"] = np.stack([pr.stored(a[i], pr.TRAJ_STORED) for a in a64])
        data[f"err32_p{i}_traj"] = np.float64(max(pr.rel_err(b[i], a[i]) for a, b in zip(a64, a32)))
    print("trajectory: losses", " ".join(f"{v:.6f}" for v in l64), f" fp32-vs-fp64 {float(data['err32_loss_traj']):.1e}")
    path = os.path.join(pr.GOLDEN, "pair.npz")
    np.savez_compressed(path, **data)
    with open(os.path.join(pr.GOLDEN, "seed.json"), "w") as f:
        json.dump({"pair": seed}, f)
        f.write("\n")
    print(f"pair.npz: {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
