"""Generate tests/golden/seg_training/ by running the REFERENCE's SegmentationHead (modules/decoders/segmentation.py with
modules/base.py and modules/segformer.py, loaded read-only from a checkout of the reference) in .eval() in float64 under
torch autograd, with torch.nn.CrossEntropyLoss(ignore_index=255), the Dice loss restated below and torch.optim.Adam, on the
cases of tests/seg_training_ref.make_inputs; and the same in float32, the yardstick of the GPU tests' bounds.

    python3 tools/make_seg_training_golden.py --reference PATH        (or KP2D_REFERENCE=PATH)

Runs only where the reference exists; no test, smoke() or bench.py reads it, they read the committed fixtures: case_*.npz
(outputs and settings only; of an array of more than MAX_STORED entries every stride_of(size)-th entry of the flattened
array), trajectory.npz (ten Adam steps of case A over all 26 parameters and three over the last layer's two: the loss of
and the trained parameters after every step) and seeds.json (the seed each case's inputs are regenerated from).  err32_*:
the error of the SAME module run in float32 on the CPU against its float64 run, E = max|G - G64| / max|G64| per quantity
(the loss: relative).

The Dice loss is smp.losses.DiceLoss(mode="multiclass", ignore_index=255) with smooth = 0 and eps = 1e-7 RESTATED
(segmentation_models_pytorch is not installed): see ``dice_loss``.

Asserted per case, re-seeding (seed + 1000, ...) until they hold, and printed: the float32 and the float64 pass pick the same
argmax in every pooling window and put every BatchNorm output on the same side of zero; every class that occurs has
S_c > 1e-3; apart from case B's deliberately ignored frame at least half the pixels are valid.
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "kp2d_reference_seg_modules"


def reference_seg_head(reference):
    """The reference's SegmentationHead from its own module files under a synthetic package; refuses anything that resolves
    outside ``reference``."""
    reference = os.path.realpath(reference)
    base = os.path.join(reference, "src", "kp2dtiny", "modules")
    for name in (PKG, PKG + ".decoders"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []       # a package without a search path: only what is loaded below exists in it
        sys.modules[name] = pkg
    mods = {}
    for name, rel in ((".base", "base.py"), (".segformer", "segformer.py"), (".decoders.segmentation", "decoders/segmentation.py")):
        path = os.path.join(base, rel)
        spec = importlib.util.spec_from_file_location(PKG + name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[PKG + name] = mod
        spec.loader.exec_module(mod)
        where = os.path.realpath(mod.__file__)
        if not where.startswith(reference + os.sep):
            raise RuntimeError(f"{mod.__name__} resolved to {where}: fixtures must come from the reference under {reference}")
        mods[name] = mod
    return mods[".decoders.segmentation"].SegmentationHead


def dice_loss(logits, labels, ignore, eps=1e-7):
    """smp's multiclass DiceLoss, from_logits, smooth 0, restated: p and the one-hot t zeroed at ignored pixels, per-class
    sums over the whole batch, score = 2 I / max(S, eps), mean over ALL classes of [class occurs] (1 - score)."""
    N, C = logits.shape[:2]
    p = logits.log_softmax(dim=1).exp().view(N, C, -1)
    y = labels.view(N, -1)
    mask = y != ignore
    p = p * mask.unsqueeze(1)
    t = torch.nn.functional.one_hot((y * mask).long(), C).permute(0, 2, 1) * mask.unsqueeze(1)
    t = t.to(p.dtype)
    inter = (p * t).sum(dim=(0, 2))
    card = (p + t).sum(dim=(0, 2))
    score = 2.0 * inter / card.clamp_min(eps)
    return ((1.0 - score) * (t.sum(dim=(0, 2)) > 0).to(p.dtype)).mean()


def build(Head, inp, dtype):
    c_exp = inp["d1"] // 4 + inp["c_skip"]
    head = Head(inp["c_in"], inp["c_hidden"], c_exp, inp["classes"], inp["d1"], with_drop=True, leaky_relu=True).to(dtype).eval()
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


def step(head, inp, dtype, sr):
    """One batch through the reference's head and the loss -> dict of detached tensors by seg_training_ref's names; the
    parameters' .grad are set.  The layers are called one by one, as SegmentationHead.forward does in eval mode, so that
    every intermediate and its gradient can be kept."""
    x = torch.from_numpy(inp["x"]).to(dtype)
    skip = torch.from_numpy(inp["skip"]).to(dtype)
    labels = torch.from_numpy(inp["labels"].astype(np.int64))
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
    wce, wd = inp["weights"]
    ce = torch.nn.CrossEntropyLoss(ignore_index=sr.IGNORE)(t["logits"], labels)
    dice = dice_loss(t["logits"], labels, sr.IGNORE)
    loss = wce * ce + wd * dice
    loss.backward()
    out = {k: v.detach() for k, v in t.items()}
    out.update({"d_" + k if k != "logits" else "dlogits": v.grad.detach() for k, v in t.items()})
    out.update(loss=loss.detach(), ce=ce.detach(), dice=dice.detach(), argmax=at)
    return out


def conditions(r64, r32, ours, inp, name):
    """-> (None or the reason the seed is refused, smallest pooling gap, smallest |pre-activation| of a BatchNorm layer)"""
    import seg_training_ref as sr
    gap = sr.pool_gap(r64["y1"].numpy())
    pre = min(float(torch.where(r64[f"y{i}"] > 0, r64[f"y{i}"], r64[f"y{i}"] / sr.SLOPE).abs().min()) for i in range(8))
    if not torch.equal(r64["argmax"], r32["argmax"]):
        return "the float32 pass picks another pooling argmax", gap, pre
    for i in range(8):
        if not torch.equal(r64[f"y{i}"] > 0, r32[f"y{i}"] > 0):
            return f"layer {i}: a BatchNorm output changes side between float32 and float64", gap, pre
    ls = sr.seg_loss(ours["logits"], inp["labels"], inp["weights"])
    if not (ls["S"][ls["present"]] > 1e-3).all():
        return "a class that occurs has S_c <= 1e-3", gap, pre
    lab = inp["labels"][:-1] if sr.CASES[name][9] == "B" else inp["labels"]
    if (lab != sr.IGNORE).mean() < 0.5:
        return "fewer than half the pixels are valid", gap, pre
    return None, gap, pre


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("KP2D_REFERENCE"), help="a checkout of the reference project")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        raise SystemExit("needs --reference PATH (or KP2D_REFERENCE): a checkout of the reference project")
    Head = reference_seg_head(args.reference)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import seg_training_ref as sr
    os.makedirs(sr.GOLDEN, exist_ok=True)
    seeds = {}

    def run(inp):
        out = {}
        for dtype in (torch.float64, torch.float32):
            head, params = build(Head, inp, dtype)
            r = step(head, inp, dtype, sr)
            r["grads"] = [p.grad.clone() for p in params]
            out[dtype] = r
        return out[torch.float64], out[torch.float32]

    for name, case in sr.CASES.items():
        src = case[9]
        if src not in seeds:
            seed = sr.BASE_SEED[src]
            while True:
                inp = sr.make_inputs(name, seed)
                r64, r32 = run(inp)
                why, gap, pre = conditions(r64, r32, sr.step_gradients(inp), inp, name)
                if why is None:
                    break
                print(f"case {name}: seed {seed} refused: {why}")
                seed += 1000
            seeds[src] = seed
            print(f"case {name}: seed {seed}; smallest pooling gap {gap:.3e}, smallest |pre-activation| {pre:.3e}")
        inp = sr.make_inputs(name, seeds[src])
        r64, r32 = run(inp)
        ours = sr.step_gradients(inp)
        assert conditions(r64, r32, ours, inp, name)[0] is None
        keys = sr.MAPS + sr.DMAPS
        data = {k: sr.stored(r64[k].numpy()) for k in keys}
        data.update({f"g{i}": sr.stored(g.numpy()) for i, g in enumerate(r64["grads"])})
        l64 = float(r64["loss"])
        data.update(loss=np.float64(l64), ce=np.float64(r64["ce"]), dice=np.float64(r64["dice"]), valid=np.int64(ours["valid"]),
                    max_stored=np.int64(sr.MAX_STORED), seed=np.int64(seeds[src]), weights=np.asarray(inp["weights"], np.float64),
                    err32_loss=np.float64(abs(float(r32["loss"]) - l64) / abs(l64)))
        for k in keys:
            data["err32_" + k] = np.float64(sr.rel_err(r32[k].numpy(), r64[k].numpy()))
        for i in range(26):
            data[f"err32_g{i}"] = np.float64(sr.rel_err(r32["grads"][i].numpy(), r64["grads"][i].numpy()))
        worst = max(sr.rel_err(np.asarray(a).reshape(b.shape), b.numpy()) for a, b in zip(ours["grads"], r64["grads"]))
        path = os.path.join(sr.GOLDEN, f"case_{name}.npz")
        np.savez_compressed(path, **data)
        print(f"case_{name}.npz: {os.path.getsize(path)} B  loss {l64!r} (CE {float(r64['ce']):.6f}, Dice {float(r64['dice']):.6f})  "
              f"valid {ours['valid']}  oracle-vs-reference gradients {worst:.1e}")
        print("  fp32 error: loss %.1e; largest of the maps %.1e, of the gradients %.1e" % (
            data["err32_loss"], max(float(data["err32_" + k]) for k in keys), max(float(data[f"err32_g{i}"]) for i in range(26))))

    with open(os.path.join(sr.GOLDEN, "seeds.json"), "w") as f:
        json.dump(seeds, f, indent=1, sort_keys=True)
        f.write("\n")

    # the trajectory: Adam on case A, all 26 parameters and the last layer's two
    inp = sr.make_inputs(sr.TRAJECTORY_CASE, seeds[sr.CASES[sr.TRAJECTORY_CASE][9]])
    data = {"lr": np.float64(sr.LR)}
    for mode, steps in (("head", sr.HEAD_STEPS), ("last", sr.LAST_STEPS)):
        runs = {}
        for dtype in (torch.float64, torch.float32):
            head, params = build(Head, inp, dtype)
            trained = params if mode == "head" else params[24:]
            opt = torch.optim.Adam(trained, lr=sr.LR)
            losses, after = [], []
            for _ in range(steps):
                opt.zero_grad()
                for p in params:
                    p.grad = None
                losses.append(float(step(head, inp, dtype, sr)["loss"]))
                opt.step()
                after.append([p.detach().numpy().copy() for p in trained])
            runs[dtype] = (np.asarray(losses, np.float64), after)
        l64, a64 = runs[torch.float64]
        l32, a32 = runs[torch.float32]
        data[f"losses_{mode}"] = l64
        data[f"err32_loss_{mode}"] = np.float64((np.abs(l32 - l64) / np.abs(l64)).max())
        for j in range(len(a64[0])):
            i = j if mode == "head" else 24 + j
            data[f"p{i}_{mode}"] = np.stack([sr.stored(a[j], sr.TRAJ_STORED) for a in a64])
            data[f"err32_p{i}_{mode}"] = np.float64(max(sr.rel_err(b[j], a[j]) for a, b in zip(a64, a32)))
        print(f"trajectory {mode}: losses", " ".join(f"{v:.6f}" for v in l64), f" fp32-vs-fp64 {float(data[f'err32_loss_{mode}']):.1e}; "
              f"parameters {max(float(data[k]) for k in data if k.startswith('err32_p') and k.endswith(mode)):.1e}")
    path = os.path.join(sr.GOLDEN, "trajectory.npz")
    np.savez_compressed(path, **data)
    print(f"trajectory.npz: {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
