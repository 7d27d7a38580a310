"""Generate tests/golden/depth_training/ by running the REFERENCE's SegmentationHead with one class
(modules/decoders/segmentation.py with modules/base.py and modules/segformer.py) in .eval() followed by .sigmoid(), and its
SILogLoss (utils/losses.py) with torch.nn.HuberLoss() as KeypointNetwithIOLoss._compute_depth_loss combines them, loaded
read-only from a checkout of the reference, in float64 under torch autograd with torch.optim.Adam, on the cases of
tests/depth_training_ref; and the same in float32, the yardstick of the GPU tests' bounds.

    python3 tools/make_depth_training_golden.py --reference PATH        (or KP2D_REFERENCE=PATH)

Runs only where the reference exists (its losses.py imports matplotlib); no test, smoke() or bench.py reads it, they read the
committed fixtures: case_*.npz (outputs and settings only; of an array of more than MAX_STORED entries every
stride_of(size)-th entry of the flattened array), trajectory.npz (ten Adam steps of case C over all 26 parameters and three
over the last layer's two: the loss of and the trained parameters after every step) and seeds.json (the seed each case's
inputs are regenerated from).  err32_*: the error of the SAME modules run in float32 on the CPU against their float64 run,
E = max|G - G64| / max|G64| per quantity (a scalar: relative).

Asserted per case on the float64 run, re-seeding (seed + 1000, ...) until the reference alone meets them, and printed:
|logit| <= 8 (case L4, whose logits are near -20 by definition: <= 20.01); between 10 % and 40 % of the pixels have gt <= 0
(case L3: apart from its two deliberately emptied frames); both Huber branches hold at least 10 % of the valid pixels each
(not L4: its gt is near 0.9, every pixel is on the quadratic branch); Dg >= 1e-3; the smallest ||d| - 1| exceeds 100 x the
float32 run's error of d, and for the whole step the |pre-activation| of a BatchNorm layer exceeds 100 x the float32
run's error of that same element and both runs pick the same pooling argmax, so no branch flips between float32 and float64.
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_seg_training_golden import reference_seg_head  # noqa: E402  (the loading mechanism, and its refusal of foreign files)


def reference_silog(reference):
    """The reference's SILogLoss from its own utils/losses.py."""
    reference = os.path.realpath(reference)
    path = os.path.join(reference, "src", "kp2dtiny", "utils", "losses.py")
    spec = importlib.util.spec_from_file_location("kp2d_reference_losses", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.realpath(mod.__file__).startswith(reference + os.sep):
        raise RuntimeError(f"{mod.__file__}: fixtures must come from the reference under {reference}")
    return mod.SILogLoss


def reference_loss(SILog, z, gt, weights):
    """_compute_depth_loss on pred = z.sigmoid(), z [N, 1, H, W] -> (loss, silog, huber, d = pred - gt)"""
    pred = z.sigmoid()
    mask = gt.gt(0.0)
    silog = SILog()(pred, gt, mask=mask)
    huber = torch.nn.HuberLoss()(pred[mask], gt[mask])
    return weights[0] * silog + weights[1] * huber, silog, huber, (pred - gt).detach()


def build(Head, inp, dtype):
    c_exp = inp["d1"] // 4 + inp["c_skip"]
    head = Head(inp["c_in"], inp["c_hidden"], c_exp, 1, inp["d1"], with_drop=True, leaky_relu=True).to(dtype).eval()
    p = [torch.from_numpy(a).to(dtype) for a in inp["params"]]
    params = []
    with torch.no_grad():
        for i in range(8):
            layer = head.convs[i]
            layer.conv.weight.copy_(p[3 * i])
            layer.bn.weight.copy_(p[3 * i + 1])
            layer.bn.bias.copy_(p[3 * i + 2])
            layer.bn.running_mean.copy_(torch.from_numpy(inp["stats"][i][0]).to(dtype))
            layer.bn.running_var.copy_(torch.from_numpy(inp["stats"][i][1]).to(dtype))
            params += [layer.conv.weight, layer.bn.weight, layer.bn.bias]
        head.convs[8].weight.copy_(p[24])
        head.convs[8].bias.copy_(p[25])
    named = [q for _, q in head.named_parameters()]
    params += [head.convs[8].weight, head.convs[8].bias]
    assert len(named) == 26 and all(a is b for a, b in zip(named, params)), "not the reference's registration order"
    return head, params


def step(head, SILog, inp, dtype):
    """One batch through the reference's head and the loss -> dict of detached tensors by seg_training_ref's names; the
    parameters' .grad are set.  The layers are called one by one, as SegmentationHead.forward does in eval mode."""
    x = torch.from_numpy(inp["x"]).to(dtype)
    skip = torch.from_numpy(inp["skip"]).to(dtype)
    gt = torch.from_numpy(inp["gt"]).to(dtype)[:, None]
    c = head.convs
    t = {}
    t["y0"] = c[0](x)
    t["y1"] = c[1](t["y0"])
    t["pooled"], at = torch.nn.functional.max_pool2d(t["y1"], 2, 2, return_indices=True)
    t["y2"] = c[2](t["pooled"])
    t["y3"] = c[3](t["y2"])
    t["y4"] = c[4](t["y3"])
    t["cat1"] = torch.cat([head.upsample(head.dropout(t["y4"])), x], dim=1)
    t["y5"] = c[5](t["cat1"])
    t["y6"] = c[6](head.dropout(t["y5"]))
    t["cat2"] = torch.cat([head.upsample2(t["y6"]), skip], dim=1)
    t["y7"] = c[7](t["cat2"])
    t["logits"] = c[8](t["y7"])
    for v in t.values():
        v.retain_grad()
    with torch.no_grad():
        assert torch.equal(head(x, skip), t["logits"]), "SegmentationHead.forward is not the layer sequence restated here"
    loss, silog, huber, d = reference_loss(SILog, t["logits"], gt, inp["weights"])
    loss.backward()
    out = {k: v.detach() for k, v in t.items()}
    out.update({"d_" + k if k != "logits" else "dlogits": v.grad.detach() for k, v in t.items()})
    out.update(loss=loss.detach(), silog=silog.detach(), huber=huber.detach(), argmax=at, d=d[:, 0])
    return out


def loss_conditions(name, z, gt, d64, d32, Dg, emptied=()):
    """-> (None or the reason the seed is refused, the smallest ||d| - 1|, the float32 run's error of d)"""
    ok = gt > 0
    gap = float(np.abs(np.abs(d64[ok]) - 1.0).min())
    derr = float(np.abs(d32[ok].astype(np.float64) - d64[ok]).max())
    zmax = 20.01 if name == "L4" else 8.0
    if np.abs(z).max() > zmax:
        return f"|logit| {np.abs(z).max():.3f} above {zmax}", gap, derr
    frames = [n for n in range(gt.shape[0]) if n not in emptied]
    none = float((gt[frames] <= 0).mean())
    if not 0.1 <= none <= 0.4:
        return f"{none:.3f} of the pixels have gt <= 0", gap, derr
    linear = float((np.abs(d64[ok]) >= 1.0).mean())
    if name != "L4" and not 0.1 <= linear <= 0.9:
        return f"{linear:.3f} of the valid pixels are on Huber's linear branch", gap, derr
    if Dg < 1e-3:
        return f"Dg {Dg:.3e} below 1e-3", gap, derr
    if not gap > 100.0 * derr:
        return f"smallest ||d| - 1| {gap:.3e} within 100 x the float32 error of d {derr:.3e}", gap, derr
    return None, gap, derr


def _pre(r):
    return [torch.where(r[f"y{i}"] > 0, r[f"y{i}"], r[f"y{i}"] / 0.01) for i in range(8)]


def step_conditions(r64, r32):
    """-> (None or the reason, the smallest |pre-activation|, the float32 run's error of that element); the condition holds
    element by element: every |pre-activation| exceeds 100 x the float32 run's error of that same element."""
    pre64 = torch.cat([p.flatten() for p in _pre(r64)])
    err = (torch.cat([p.flatten() for p in _pre(r32)]).double() - pre64).abs()
    at = int(pre64.abs().argmin())
    pre, perr = float(pre64[at].abs()), float(err[at])
    if not torch.equal(r64["argmax"], r32["argmax"]):
        return "the float32 pass picks another pooling argmax", pre, perr
    bad = pre64.abs() <= 100.0 * err
    if bad.any():
        k = int(bad.float().argmax())
        return f"a |pre-activation| {float(pre64[k].abs()):.3e} within 100 x its float32 error {float(err[k]):.3e}", pre, perr
    return None, pre, perr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("KP2D_REFERENCE"), help="a checkout of the reference project")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        raise SystemExit("needs --reference PATH (or KP2D_REFERENCE): a checkout of the reference project")
    Head = reference_seg_head(args.reference)
    SILog = reference_silog(args.reference)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import depth_training_ref as dr
    os.makedirs(dr.GOLDEN, exist_ok=True)
    seeds = {}

    # ---- the loss alone ----
    def run_loss(z, gt):
        out = {}
        for dtype in (torch.float64, torch.float32):
            zt = torch.from_numpy(z).to(dtype)[:, None].requires_grad_(True)
            loss, silog, huber, d = reference_loss(SILog, zt, torch.from_numpy(gt).to(dtype)[:, None], dr.WEIGHTS)
            loss.backward()
            out[dtype] = {"loss": float(loss), "silog": float(silog), "huber": float(huber), "dlogits": zt.grad[:, 0].numpy(), "d": d[:, 0].numpy()}
        return out[torch.float64], out[torch.float32]

    def scalar_err(a, b):
        return np.float64(abs(a - b) / abs(b))

    for name in dr.LOSS_CASES:
        seed = dr.BASE_SEED[name]
        while True:
            z, gt = dr.make_loss_inputs(name, seed)
            r64, r32 = run_loss(z, gt)
            ours = dr.depth_loss(z, gt)
            why, gap, derr = loss_conditions(name, z, gt, r64["d"], r32["d"], ours["Dg"], emptied=(1, 3) if name == "L3" else ())
            if why is None:
                break
            print(f"case {name}: seed {seed} refused: {why}")
            seed += 1000
        seeds[name] = seed
        data = {"dlogits": dr.stored(r64["dlogits"]), "loss": np.float64(r64["loss"]), "silog": np.float64(r64["silog"]),
                "huber": np.float64(r64["huber"]), "valid": np.int64(ours["valid"]), "Dg": np.float64(ours["Dg"]),
                "max_stored": np.int64(dr.MAX_STORED), "seed": np.int64(seed), "weights": np.asarray(dr.WEIGHTS, np.float64),
                "huber_gap": np.float64(gap), "err32_d": np.float64(derr),
                "err32_dlogits": np.float64(dr.rel_err(r32["dlogits"], r64["dlogits"]))}
        for k in ("loss", "silog", "huber"):
            data["err32_" + k] = scalar_err(r32[k], r64[k])
        worst = max(dr.rel_err(ours["dz"], r64["dlogits"]), abs(ours["loss"] - r64["loss"]))
        path = os.path.join(dr.GOLDEN, f"case_{name}.npz")
        np.savez_compressed(path, **data)
        print(f"case_{name}.npz: {os.path.getsize(path)} B  seed {seed}  loss {r64['loss']!r} (SILog {r64['silog']:.6f}, Huber {r64['huber']:.6f})  "
              f"valid {ours['valid']}  Dg {ours['Dg']:.3e}  oracle-vs-reference {worst:.1e}")
        print("  fp32 error: loss %.1e, SILog %.1e, Huber %.1e, dlogits %.1e; smallest ||d| - 1| %.3e against d's error %.1e" % (
            data["err32_loss"], data["err32_silog"], data["err32_huber"], data["err32_dlogits"], gap, derr))

    # ---- the whole step ----
    def run(inp):
        out = {}
        for dtype in (torch.float64, torch.float32):
            head, params = build(Head, inp, dtype)
            r = step(head, SILog, inp, dtype)
            r["grads"] = [p.grad.clone() for p in params]
            out[dtype] = r
        return out[torch.float64], out[torch.float32]

    keys = dr.MAPS + dr.DMAPS
    for name in dr.STEP_CASES:
        seed = dr.BASE_SEED[name]
        while True:
            inp = dr.make_inputs(name, seed)
            r64, r32 = run(inp)
            ours = dr.step_gradients(inp)
            why, gap, derr = loss_conditions(name, r64["logits"][:, 0].numpy(), inp["gt"], r64["d"].numpy(), r32["d"].numpy(), ours["Dg"])
            if why is None:
                why, pre, perr = step_conditions(r64, r32)
            if why is None:
                break
            print(f"case {name}: seed {seed} refused: {why}")
            seed += 1000
        seeds[name] = seed
        data = {k: dr.stored(r64[k].numpy()) for k in keys}
        data.update({f"g{i}": dr.stored(g.numpy()) for i, g in enumerate(r64["grads"])})
        data.update(loss=np.float64(r64["loss"]), silog=np.float64(r64["silog"]), huber=np.float64(r64["huber"]),
                    valid=np.int64(ours["valid"]), Dg=np.float64(ours["Dg"]), max_stored=np.int64(dr.MAX_STORED), seed=np.int64(seed),
                    weights=np.asarray(inp["weights"], np.float64), huber_gap=np.float64(gap), err32_d=np.float64(derr),
                    pre_gap=np.float64(pre), err32_pre=np.float64(perr))
        for k in ("loss", "silog", "huber"):
            data["err32_" + k] = scalar_err(float(r32[k]), float(r64[k]))
        for k in keys:
            data["err32_" + k] = np.float64(dr.rel_err(r32[k].numpy(), r64[k].numpy()))
        for i in range(26):
            data[f"err32_g{i}"] = np.float64(dr.rel_err(r32["grads"][i].numpy(), r64["grads"][i].numpy()))
        worst = max(dr.rel_err(np.asarray(a).reshape(b.shape), b.numpy()) for a, b in zip(ours["grads"], r64["grads"]))
        path = os.path.join(dr.GOLDEN, f"case_{name}.npz")
        np.savez_compressed(path, **data)
        print(f"case_{name}.npz: {os.path.getsize(path)} B  seed {seed}  loss {float(r64['loss'])!r} (SILog {float(r64['silog']):.6f}, "
              f"Huber {float(r64['huber']):.6f})  valid {ours['valid']}  |logit| <= {float(r64['logits'].abs().max()):.3f}  "
              f"oracle-vs-reference gradients {worst:.1e}")
        print("  fp32 error: loss %.1e; largest of the maps %.1e, of the gradients %.1e; smallest ||d| - 1| %.3e (error %.1e), "
              "smallest |pre-activation| %.3e (error %.1e)" % (data["err32_loss"], max(float(data["err32_" + k]) for k in keys),
                                                              max(float(data[f"err32_g{i}"]) for i in range(26)), gap, derr, pre, perr))

    with open(os.path.join(dr.GOLDEN, "seeds.json"), "w") as f:
        json.dump(seeds, f, indent=1, sort_keys=True)
        f.write("\n")

    # ---- the trajectory: Adam on case C, all 26 parameters and the last layer's two ----
    inp = dr.make_inputs(dr.TRAJECTORY_CASE, seeds[dr.TRAJECTORY_CASE])
    data = {"lr": np.float64(dr.LR)}
    for mode, steps in (("head", dr.HEAD_STEPS), ("last", dr.LAST_STEPS)):
        runs = {}
        for dtype in (torch.float64, torch.float32):
            head, params = build(Head, inp, dtype)
            trained = params if mode == "head" else params[24:]
            opt = torch.optim.Adam(trained, lr=dr.LR)
            losses, after = [], []
            for _ in range(steps):
                opt.zero_grad()
                for p in params:
                    p.grad = None
                losses.append(float(step(head, SILog, inp, dtype)["loss"]))
                opt.step()
                after.append([p.detach().numpy().copy() for p in trained])
            runs[dtype] = (np.asarray(losses, np.float64), after)
        l64, a64 = runs[torch.float64]
        l32, a32 = runs[torch.float32]
        data[f"losses_{mode}"] = l64
        data[f"err32_loss_{mode}"] = np.float64((np.abs(l32 - l64) / np.abs(l64)).max())
        for j in range(len(a64[0])):
            i = j if mode == "head" else 24 + j
            data[f"p{i}_{mode}"] = np.stack([dr.stored(a[j], dr.TRAJ_STORED) for a in a64])
            data[f"err32_p{i}_{mode}"] = np.float64(max(dr.rel_err(b[j], a[j]) for a, b in zip(a64, a32)))
        print(f"trajectory {mode}: losses", " ".join(f"{v:.6f}" for v in l64), f" fp32-vs-fp64 {float(data[f'err32_loss_{mode}']):.1e}; "
              f"parameters {max(float(data[k]) for k in data if k.startswith('err32_p') and k.endswith(mode)):.1e}")
    path = os.path.join(dr.GOLDEN, "trajectory.npz")
    np.savez_compressed(path, **data)
    print(f"trajectory.npz: {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
