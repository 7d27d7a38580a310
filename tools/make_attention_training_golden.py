"""Generate tests/golden/attention_training/ by running the REFERENCE's SegFormerAttentionModule (modules/segformer.py) and
SegmentationHeadATT (modules/decoders/segmentation.py with modules/base.py, loaded read-only from a checkout of the reference)
in .eval() in float64 under torch autograd, with torch.nn.CrossEntropyLoss(ignore_index=255), the Dice loss restated in
make_seg_training_golden.py, the depth loss restated in make_depth_training_golden.py and torch.optim.Adam, on the cases of
tests/attention_training_ref; and the same in float32, the yardstick of the GPU tests' bounds.

    python3 tools/make_attention_training_golden.py --reference PATH        (or KP2D_REFERENCE=PATH)

Runs only where the reference exists; no test, smoke() or bench.py reads it, they read the committed fixtures: case_*.npz
(outputs and settings only; of an array of more than MAX_STORED entries every stride_of(size)-th entry), trajectory_*.npz (five
Adam steps over all 47 parameters: the loss of and the parameters after every step) and seeds.json.  err32_*: the error of the
SAME modules run in float32 on the CPU against their float64 run, E = max|G - G64| / max|G64| per quantity (the loss: relative).
Every intermediate is taken by a forward hook on the reference's own submodule, never from a restated forward; the log-sum-exp,
which the reference does not form, is torch.logsumexp of its own q and k.

A seed is kept only when, element by element, every discrete choice is safe by 100 x its own float32 error: a LeakyReLU's
pre-activation is further from zero than 100 x that element's |float32 - float64|, a pooling window's two largest values
are further apart than 100 x their errors; and LayerNorm's sqrt(var) is above MIN_S at every pixel.  Refused seeds are printed.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(1, os.path.join(ROOT, "tools"))


import make_depth_training_golden as depth_tool  # noqa: E402  (the reference's SILogLoss and how the depth loss combines it)
import make_depth_pair_golden as pair_tool  # noqa: E402  (the warper restated by grid_sample)
import make_seg_training_golden as seg_tool  # noqa: E402  (the loading mechanism, its refusal of foreign files, the Dice loss)


def reference_classes(reference):
    """-> (SegFormerAttentionModule, SegmentationHeadATT) from the reference's own files (the seg generator's loader)."""
    seg_tool.reference_seg_head(reference)
    pkg = seg_tool.PKG
    return sys.modules[pkg + ".segformer"].SegFormerAttentionModule, sys.modules[pkg + ".decoders.segmentation"].SegmentationHeadATT


def module_tensors(mod):
    att, mff = mod.att, mod.mff
    net = mff.fn.net
    return [att.fn.to_q.weight, att.fn.to_kv.weight, att.fn.to_out.weight, att.norm.g, att.norm.b, net[0].weight, net[0].bias,
            net[1].net[0].weight, net[1].net[0].bias, net[1].net[1].weight, net[1].net[1].bias, net[3].weight, net[3].bias, mff.norm.g,
            mff.norm.b]


def load_module(mod, arrays, dtype):
    ts = module_tensors(mod)
    assert [id(t) for t in ts] == [id(t) for t in mod.parameters()], "not the reference's registration order"
    with torch.no_grad():
        for t, a in zip(ts, arrays):
            t.copy_(torch.from_numpy(a).to(dtype))
    return ts


class Taps:
    """Forward hooks that keep (and retain the gradient of) the outputs of named submodules."""

    def __init__(self):
        self.t, self.handles = {}, []

    def out(self, module, name):
        def hook(_m, _i, o):
            o.retain_grad()
            self.t[name] = o
        self.handles.append(module.register_forward_hook(hook))

    def inp(self, module, name):
        def hook(_m, i):
            i[0].retain_grad()
            self.t[name] = i[0]
        self.handles.append(module.register_forward_pre_hook(hook))

    def remove(self):
        for h in self.handles:
            h.remove()


def tap_module(taps, mod, prefix=""):
    esa, net = mod.att.fn, mod.mff.fn.net
    taps.out(mod.att.norm, prefix + "n1")
    taps.out(esa.to_q, prefix + "q")
    taps.out(esa.to_kv, prefix + "kv")
    taps.inp(esa.to_out, prefix + "o")
    taps.out(esa.to_out, prefix + "a")
    taps.out(mod.mff.norm, prefix + "n2")
    taps.out(net[0], prefix + "h0")
    taps.out(net[1].net[0], prefix + "h1")
    taps.out(net[1].net[1], prefix + "pre")
    taps.out(net[2], prefix + "h2")


def lse_of(q, kv, heads=4):
    N, C, H, W = q.shape
    qh = q.reshape(N, heads, C // heads, H * W).transpose(2, 3)
    kh = kv[:, :C].reshape(N, heads, C // heads, -1).transpose(2, 3)
    return torch.logsumexp(qh @ kh.transpose(2, 3) * (C // heads) ** -0.5, dim=3)


def run_module(Module, inp, dtype):
    mod = Module(inp["C"]).to(dtype).eval()
    params = load_module(mod, inp["params"], dtype)
    taps = Taps()
    tap_module(taps, mod)
    x = torch.from_numpy(inp["x"]).to(dtype).requires_grad_(True)
    y = mod(x)
    y.backward(torch.from_numpy(inp["dy"]).to(dtype))
    taps.remove()
    t = taps.t
    out = {k: v.detach() for k, v in t.items()}
    out["y"] = y.detach()
    out["lse"] = lse_of(out["q"], out["kv"])
    out.update({"d_" + k: t[k].grad for k in ("h2", "pre", "h1", "h0", "n2", "a", "o", "q", "kv", "n1")})
    out["dx"] = x.grad
    out["grads"] = [p.grad.clone() for p in params]
    s = [torch.var(v, dim=1, unbiased=False).sqrt().min() for v in (x.detach(), out["a"])]
    out["min_s"] = float(min(s))
    return out


def build_head(Head, inp, dtype):
    c_exp = inp["d1"] // 4 + inp["c_skip"]
    head = Head(inp["c_in"], inp["c_hidden"], c_exp, inp["classes"], inp["d1"], with_drop=True, leaky_relu=True).to(dtype).eval()
    p = inp["params"]
    params = []
    with torch.no_grad():
        at = 0
        for i in range(7):
            layer = head.convs[i]
            if i in (1, 2):
                params += load_module(layer, p[at:at + 15], dtype)
                at += 15
                continue
            for t, a in zip((layer.conv.weight, layer.bn.weight, layer.bn.bias), p[at:at + 3]):
                t.copy_(torch.from_numpy(a).to(dtype))
            layer.bn.running_mean.copy_(torch.from_numpy(inp["stats"][i][0]).to(dtype))
            layer.bn.running_var.copy_(torch.from_numpy(inp["stats"][i][1]).to(dtype))
            params += [layer.conv.weight, layer.bn.weight, layer.bn.bias]
            at += 3
        head.convs[7].weight.copy_(torch.from_numpy(p[45]).to(dtype))
        head.convs[7].bias.copy_(torch.from_numpy(p[46]).to(dtype))
    params += [head.convs[7].weight, head.convs[7].bias]
    named = [q for _, q in head.named_parameters()]
    assert len(named) == 47 and all(a is b for a, b in zip(named, params)), "not the reference's registration order"
    return head, params


def head_loss(inp, logits, dtype, SILog, ar):
    if inp["loss"] == "seg":
        labels = torch.from_numpy(inp["target"].astype(np.int64))
        ce = torch.nn.CrossEntropyLoss(ignore_index=ar.sr.IGNORE)(logits, labels)
        return 0.5 * ce + 1.5 * seg_tool.dice_loss(logits, labels, ar.sr.IGNORE)
    return depth_tool.reference_loss(SILog, logits, torch.from_numpy(inp["target"]).to(dtype)[:, None], ar.dr.WEIGHTS)[0]


def pair_loss(inp, logits, dtype, SILog, ar):
    """The reference's depth loss over a view pair as make_depth_pair_golden.pair_step forms it; keeps the warp's decisions."""
    t = lambda k: torch.from_numpy(inp[k]).to(dtype)
    n = inp["gt"].shape[0]
    plain = depth_tool.reference_loss(SILog, logits[:n], t("gt")[:, None], inp["weights"])[0]
    aug = depth_tool.reference_loss(SILog, logits[n:], t("gt_aug")[:, None], inp["weights"])[0]
    pred = logits.sigmoid()
    warped, grid = pair_tool.warper(pred[:n], t("homography"))
    size = torch.tensor([grid.shape[2] - 1, grid.shape[1] - 1], dtype=dtype)
    inp["decisions"][dtype] = torch.round((grid.detach() + 1) / 2 * size).double()
    return plain + aug + ar.CROSS_WEIGHT * torch.nn.functional.mse_loss(pred[n:], warped)


def run_head(Head, inp, dtype, loss_of, params_from=None):
    head, params = params_from if params_from is not None else build_head(Head, inp, dtype)
    taps = Taps()
    c = head.convs
    for m, name in ((c[0], "y0"), (c[1], "m1"), (head.pool, "pooled"), (c[2], "m2"), (c[3], "y3"), (c[4], "y4"), (c[5], "y5"), (c[6], "y6"),
                    (c[7], "logits")):
        taps.out(m, name)
    tap_module(taps, c[1], "m1.")
    tap_module(taps, c[2], "m2.")
    x = torch.from_numpy(inp["x"]).to(dtype)
    skip = torch.from_numpy(inp["skip"]).to(dtype)
    logits = head(x, skip)
    loss = loss_of(inp, logits, dtype)
    loss.backward()
    taps.remove()
    out = {k: v.detach() for k, v in taps.t.items()}
    out["dlogits"] = taps.t["logits"].grad
    out["loss"] = loss.detach()
    out["grads"] = [p.grad.clone() for p in params]
    out["argmax"] = torch.nn.functional.max_pool2d(out["m1"], 2, 2, return_indices=True)[1]
    ln_in = [out["y0"], out["m1.a"], out["pooled"], out["m2.a"]]
    out["min_s"] = float(min(torch.var(v, dim=1, unbiased=False).sqrt().min() for v in ln_in))
    return out, (head, params)


def head_conditions(r64, r32, ar):
    """-> None or the reason the seed is refused"""
    if min(r64["min_s"], r32["min_s"]) <= ar.MIN_S:
        return f"a LayerNorm's sqrt(var) is {min(r64['min_s'], r32['min_s']):.3e}"
    for k in ("y0", "y3", "y4", "y5", "y6"):
        pre = torch.where(r64[k] > 0, r64[k], r64[k] / ar.SLOPE).abs()
        err = (r32[k].double() - r64[k]).abs()
        err = torch.where(r64[k] > 0, err, err / ar.SLOPE)
        if not bool((pre > 100.0 * err).all()):
            return f"{k}: a pre-activation is within 100 x its float32 error of zero"
    if not torch.equal(r64["argmax"], r32["argmax"]):
        return "the float32 pass picks another pooling argmax"
    m, e = r64["m1"], (r32["m1"].double() - r64["m1"]).abs()
    N, C, H, W = m.shape
    win = lambda t: t[:, :, :H // 2 * 2, :W // 2 * 2].reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
    top = win(m).sort(dim=4).values
    if not bool(((top[..., 3] - top[..., 2]) > 100.0 * 2.0 * win(e).max(dim=4).values).all()):
        return "a pooling window's two largest values are within 100 x their float32 error"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("KP2D_REFERENCE"), help="a checkout of the reference project")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        raise SystemExit("needs --reference PATH (or KP2D_REFERENCE): a checkout of the reference project")
    Module, Head = reference_classes(args.reference)
    SILog = depth_tool.reference_silog(args.reference)
    import attention_training_ref as ar
    os.makedirs(ar.GOLDEN, exist_ok=True)
    seeds = {}
    loss_of = lambda inp, logits, dtype: head_loss(inp, logits, dtype, SILog, ar)
    rel = ar.rel_err

    # ---- the module cases -------------------------------------------------------------------------------------------------------
    for name in ar.MODULE_CASES:
        seed = ar.BASE_SEED[name]
        while True:
            inp = ar.make_module_inputs(name, seed)
            r64, r32 = run_module(Module, inp, torch.float64), run_module(Module, inp, torch.float32)
            if min(r64["min_s"], r32["min_s"]) > ar.MIN_S:
                break
            print(f"case {name}: seed {seed} refused: a LayerNorm's sqrt(var) is {r64['min_s']:.3e}")
            seed += 1000
        seeds[name] = seed
        ours = ar.module_step(inp)
        keys = ar.MODULE_MAPS + ar.MODULE_DMAPS
        data = {k: ar.stored(r64[k].numpy()) for k in keys}
        data.update({f"g{i}": ar.stored(g.numpy()) for i, g in enumerate(r64["grads"])})
        data.update(seed=np.int64(seed), max_stored=np.int64(ar.sr.MAX_STORED), min_s=np.float64(r64["min_s"]))
        for k in keys:
            data["err32_" + k] = np.float64(rel(r32[k].numpy(), r64[k].numpy()))
        for i in range(15):
            data[f"err32_g{i}"] = np.float64(rel(r32["grads"][i].numpy(), r64["grads"][i].numpy()))
        worst = max([rel(ours[k], r64[k].numpy()) for k in keys] + [rel(np.asarray(a).reshape(b.shape), b.numpy()) for a, b in zip(ours["grads"], r64["grads"])])
        path = os.path.join(ar.GOLDEN, f"case_{name}.npz")
        np.savez_compressed(path, **data)
        print(f"case_{name}.npz: {os.path.getsize(path)} B  seed {seed}  min sqrt(var) {r64['min_s']:.3f}  oracle-vs-reference {worst:.1e}  "
              f"fp32 error: maps {max(float(data['err32_' + k]) for k in keys):.1e}, gradients {max(float(data[f'err32_g{i}']) for i in range(15)):.1e}")

    # ---- the head cases ---------------------------------------------------------------------------------------------------------
    for name in ar.HEAD_CASES:
        seed = ar.BASE_SEED[name]
        for _ in range(400):
            inp = ar.make_head_inputs(name, seed)
            r64, r32 = run_head(Head, inp, torch.float64, loss_of)[0], run_head(Head, inp, torch.float32, loss_of)[0]
            why = head_conditions(r64, r32, ar)
            if why is None:
                break
            print(f"case {name}: seed {seed} refused: {why}")
            seed += 1000
        else:
            raise SystemExit(f"case {name}: no seed passed the conditions")
        seeds[name] = seed
        ours = ar.head_step(inp)
        data = {k: ar.stored(r64[k].numpy()) for k in ar.HEAD_MAPS + ("dlogits",)}
        data.update({f"g{i}": ar.stored(g.numpy()) for i, g in enumerate(r64["grads"])})
        l64 = float(r64["loss"])
        data.update(loss=np.float64(l64), seed=np.int64(seed), max_stored=np.int64(ar.sr.MAX_STORED), min_s=np.float64(r64["min_s"]),
                    err32_loss=np.float64(abs(float(r32["loss"]) - l64) / abs(l64)))
        for k in ar.HEAD_MAPS + ("dlogits",):
            data["err32_" + k] = np.float64(rel(r32[k].numpy(), r64[k].numpy()))
        for i in range(47):
            data[f"err32_g{i}"] = np.float64(rel(r32["grads"][i].numpy(), r64["grads"][i].numpy()))
        worst = max(rel(np.asarray(a).reshape(b.shape), b.numpy()) for a, b in zip(ours["grads"], r64["grads"]))
        path = os.path.join(ar.GOLDEN, f"case_{name}.npz")
        np.savez_compressed(path, **data)
        print(f"case_{name}.npz: {os.path.getsize(path)} B  seed {seed}  loss {l64!r} (oracle {ours['loss']!r})  min sqrt(var) {r64['min_s']:.3f}  "
              f"oracle-vs-reference gradients {worst:.1e}  fp32 error: loss {float(data['err32_loss']):.1e}, gradients "
              f"{max(float(data[f'err32_g{i}']) for i in range(47)):.1e}")

    with open(os.path.join(ar.GOLDEN, "seeds.json"), "w") as f:
        json.dump(seeds, f, indent=1, sort_keys=True)
        f.write("\n")

    # ---- the pair step's seed: the head's conditions on the batch of both views, and the warp's ------------------------------
    import depth_pair_ref as pr

    def pair_batch(seed):
        inp = ar.make_pair_inputs(seed)
        batch = dict(inp, x=np.concatenate([inp["x"], inp["x_aug"]]), skip=np.concatenate([inp["skip"], inp["skip_aug"]]), decisions={})
        return inp, batch

    pair_of = lambda inp, logits, dtype: pair_loss(inp, logits, dtype, SILog, ar)
    seed = ar.BASE_SEED["pair"]
    for _ in range(400):
        inp, batch = pair_batch(seed)
        margin = pr.nearest_margin(inp["homography"], 2 * inp["h"], 2 * inp["w"])
        why = None if margin > ar.NEAREST_SAFE else f"a nearest decision is {margin:.2e} pixel from a tie"
        if why is None:
            r64, r32 = run_head(Head, batch, torch.float64, pair_of)[0], run_head(Head, batch, torch.float32, pair_of)[0]
            why = head_conditions(r64, r32, ar)
            if why is None and not torch.equal(batch["decisions"][torch.float64], batch["decisions"][torch.float32]):
                why = "the float32 run rounds a coordinate the other way"
        if why is None:
            break
        print(f"pair: seed {seed} refused: {why}")
        seed += 1000
    else:
        raise SystemExit("pair: no seed passed the conditions")
    seeds["pair"] = seed
    ours = ar.pair_step(inp)
    worst = max(rel(np.asarray(a).reshape(b.shape), b.numpy()) for a, b in zip(ours["grads"], r64["grads"]))
    print(f"pair: seed {seed}  loss {float(r64['loss'])!r} (oracle {ours['loss']!r})  nearest margin {margin:.2e}  oracle-vs-reference gradients {worst:.1e}")
    assert abs(ours["loss"] - float(r64["loss"])) <= 1e-10 and worst <= 1e-10
    with open(os.path.join(ar.GOLDEN, "seeds.json"), "w") as f:
        json.dump(seeds, f, indent=1, sort_keys=True)
        f.write("\n")

    # ---- the trajectories: Adam on the first seg shape, on the depth head, and the depth head's pair step -----------------------
    for name in ("seg", "depth", "pair"):
        inp = ar.make_head_inputs(name, seeds[name]) if name != "pair" else pair_batch(seeds["pair"])[1]
        steps, of = (ar.PAIR_STEPS, pair_of) if name == "pair" else (ar.TRAJECTORY_STEPS, loss_of)
        runs = {}
        for dtype in (torch.float64, torch.float32):
            built = build_head(Head, inp, dtype)
            opt = torch.optim.Adam(built[1], lr=ar.LR)
            losses, after = [], []
            for _ in range(steps):
                opt.zero_grad()
                for p in built[1]:
                    p.grad = None
                losses.append(float(run_head(Head, inp, dtype, of, params_from=built)[0]["loss"]))
                opt.step()
                after.append([p.detach().numpy().copy() for p in built[1]])
            runs[dtype] = (np.asarray(losses, np.float64), after)
        (l64, a64), (l32, a32) = runs[torch.float64], runs[torch.float32]
        data = {"lr": np.float64(ar.LR), "losses": l64, "err32_loss": np.float64((np.abs(l32 - l64) / np.abs(l64)).max())}
        for i in range(47):
            data[f"p{i}"] = np.stack([ar.stored(a[i], ar.TRAJ_STORED) for a in a64])
            data[f"err32_p{i}"] = np.float64(max(rel(b[i], a[i]) for a, b in zip(a64, a32)))
        path = os.path.join(ar.GOLDEN, f"trajectory_{name}.npz")
        np.savez_compressed(path, **data)
        print(f"trajectory_{name}.npz: {os.path.getsize(path)} B  losses", " ".join(f"{v:.6f}" for v in l64),
              f" fp32-vs-fp64 {float(data['err32_loss']):.1e}; parameters {max(float(data[f'err32_p{i}']) for i in range(47)):.1e}")


if __name__ == "__main__":
    main()
