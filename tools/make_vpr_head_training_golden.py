"""Generate tests/golden/vpr_head_training/case_*.npz by running the REFERENCE's VPRHead (modules/decoders/vpr.py with
modules/base.py and modules/aggregators/netvlad.py, loaded read-only from a checkout of the reference) in .eval() in float64
under torch autograd, with TripletMarginLoss(margin ** 0.5, p=2, reduction="sum") / nNeg and torch.optim.Adam the way
train_visloc.py puts them together, on the cases of tests/vpr_head_training_ref.make_inputs; and the same in float32, the
yardstick of the GPU tests' bounds.

    python3 tools/make_vpr_head_training_golden.py --reference PATH        (or KP2D_REFERENCE=PATH)

Runs only where the reference exists; no test, smoke() or bench.py reads it, they read the committed fixtures.  Each
fixture holds outputs and settings only (the inputs are regenerated from seeds).  Of an array of more than MAX_STORED
entries it keeps every stride_of(size)-th entry of the flattened array (vpr_head_training_ref.stored); the float64 numpy
oracle there, held to the stored entries to 1e-10, stands in for the whole array.  Stored per case: y1, y2, y3 (each layer's
output), vlad, dvlad, loss, n_active, the eleven gradients g0..g10 (PARAMS order), dx_netvlad, dx3, dx2 (the gradients with
respect to the inputs of NetVLAD, convlad3, convlad2), and err32_*: the error of the SAME module run in float32 on the CPU
against its float64 run (|loss - loss64|; E = max|G - G64| / max|G64| per quantity, the maximum over a group's members).
The trajectory case adds the ten losses of ten Adam steps over all eleven parameters and every parameter after three.

Asserted here on the CPU, and printed: min |hinge| >= 1e-4 in every case (n_active cannot flip under fp32 rounding), at
least one active and one inactive triplet across the cases, and the float32 run's n_active equals the float64 run's.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "kp2d_reference_modules"


def reference_vpr_head(reference):
    """The reference's VPRHead from its own module files under a synthetic package; refuses anything that resolves outside
    ``reference``."""
    reference = os.path.realpath(reference)
    try:
        import sklearn.neighbors  # noqa: F401  (netvlad.py's import line; init_params' vladv2 branch alone uses it)
    except ImportError:
        pkg, sub = types.ModuleType("sklearn"), types.ModuleType("sklearn.neighbors")
        sub.NearestNeighbors = None
        pkg.neighbors = sub
        sys.modules.setdefault("sklearn", pkg)
        sys.modules.setdefault("sklearn.neighbors", sub)
    base = os.path.join(reference, "src", "kp2dtiny", "modules")
    for name in (PKG, PKG + ".aggregators", PKG + ".decoders"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []       # a package without a search path: only what is loaded below exists in it
        sys.modules[name] = pkg
    mods = {}
    for name, rel in ((".base", "base.py"), (".aggregators.netvlad", "aggregators/netvlad.py"), (".aggregators.gem", "aggregators/gem.py"),
                      (".aggregators.convap", "aggregators/convap.py"), (".decoders.vpr", "decoders/vpr.py")):
        path = os.path.join(base, rel)
        spec = importlib.util.spec_from_file_location(PKG + name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[PKG + name] = mod
        spec.loader.exec_module(mod)
        where = os.path.realpath(mod.__file__)
        if not where.startswith(reference + os.sep):
            raise RuntimeError(f"{mod.__name__} resolved to {where}: fixtures must come from the reference under {reference}")
        mods[name] = mod
    return mods[".decoders.vpr"].VPRHead


def build(VPRHead, inp, dtype):
    head = VPRHead(inp["Cin"], inp["C"], inp["K"], with_drop=True, leaky_relu=inp["slope"] != 0.0).to(dtype).eval()
    layers = (head.convlad1, head.convlad2, head.convlad3)
    p = [torch.from_numpy(a).to(dtype) for a in inp["params"]]
    with torch.no_grad():
        for i, layer in enumerate(layers):
            layer.conv.weight.copy_(p[3 * i])
            layer.bn.weight.copy_(p[3 * i + 1])
            layer.bn.bias.copy_(p[3 * i + 2])
            layer.bn.running_mean.copy_(torch.from_numpy(inp["stats"][i][0]).to(dtype))
            layer.bn.running_var.copy_(torch.from_numpy(inp["stats"][i][1]).to(dtype))
        head.netvlad.conv.weight.copy_(p[9].reshape(inp["K"], inp["C"], 1, 1))
        head.netvlad.centroids.copy_(p[10])
    params = []
    for layer in layers:
        params += [layer.conv.weight, layer.bn.weight, layer.bn.bias]
    return head, params + [head.netvlad.conv.weight, head.netvlad.centroids]


def step(head, inp, dtype, margin):
    """One batch through the reference's head and torch's loss -> dict of detached tensors; the parameters' .grad are set.
    The layers are called one by one, as VPRHead.forward does in eval mode (its dropout is the identity there), so that
    each layer's output and its gradient can be kept."""
    B, counts = inp["B"], list(inp["counts"])
    total = sum(counts)
    x = torch.from_numpy(inp["feat"]).to(dtype)
    y1 = head.convlad1(x)
    y2 = head.convlad2(head.dropout(y1) if head.with_drop else y1)
    y3 = head.convlad3(y2)
    vlad = head.netvlad(y3)
    for t in (y1, y2, y3, vlad):
        t.retain_grad()
    with torch.no_grad():
        assert torch.equal(head(x), vlad), "VPRHead.forward is not the layer sequence restated here"
    owner = torch.repeat_interleave(torch.arange(B), torch.tensor(counts))
    criterion = torch.nn.TripletMarginLoss(margin=margin ** 0.5, p=2, reduction="sum")
    loss = criterion(vlad[:B][owner], vlad[B:2 * B][owner], vlad[2 * B:]) / total
    loss.backward()
    return {"y1": y1.detach(), "y2": y2.detach(), "y3": y3.detach(), "vlad": vlad.detach(), "loss": loss.detach(),
            "dvlad": vlad.grad.detach(), "dx_netvlad": y3.grad.detach(), "dx3": y2.grad.detach(), "dx2": y1.grad.detach()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("KP2D_REFERENCE"), help="a checkout of the reference project")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        raise SystemExit("needs --reference PATH (or KP2D_REFERENCE): a checkout of the reference project")
    VPRHead = reference_vpr_head(args.reference)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import vpr_head_training_ref as hr
    os.makedirs(hr.GOLDEN, exist_ok=True)
    active = inactive = 0
    for name in hr.CASES:
        inp = hr.make_inputs(name)
        out = {}
        for dtype in (torch.float64, torch.float32):
            head, params = build(VPRHead, inp, dtype)
            r = {k: v.numpy() for k, v in step(head, inp, dtype, hr.MARGIN).items()}
            r["grads"] = [p.grad.numpy().copy() for p in params]
            out[dtype] = r
        r64, r32 = out[torch.float64], out[torch.float32]
        ours = hr.step_gradients(inp["feat"], inp["params"], inp["stats"], inp["B"], inp["counts"], inp["slope"])
        hinge32 = hr.vr.triplet_loss(r32["vlad"], inp["B"], inp["counts"])[3]
        n32 = int((hinge32 > 0).sum())
        assert np.abs(ours["hinge"]).min() >= 1e-4, (name, ours["hinge"])
        assert n32 == ours["n_active"], (name, n32, ours["n_active"])
        active += ours["n_active"]
        inactive += len(ours["hinge"]) - ours["n_active"]
        data = {k: hr.stored(r64[k]) for k in hr.MAPS + ("vlad", "dvlad")}
        data.update({f"g{i}": hr.stored(g) for i, g in enumerate(r64["grads"])})
        data.update(loss=np.float64(r64["loss"]), n_active=np.int64(ours["n_active"]), margin=np.float64(hr.MARGIN),
                    max_stored=np.int64(hr.MAX_STORED), err32_loss=np.float64(abs(float(r32["loss"]) - float(r64["loss"]))))
        for group, members in hr.GROUPS.items():
            data["err32_" + group] = np.float64(max(hr.rel_err(r32["grads"][i], r64["grads"][i]) for i in members))
        for k in hr.MAPS:
            data["err32_" + k] = np.float64(hr.rel_err(r32[k], r64[k]))
        worst = max(hr.rel_err(np.asarray(a).reshape(b.shape), b) for a, b in zip(ours["grads"], r64["grads"]))
        if name == hr.TRAJECTORY_CASE:
            traj = {}
            for dtype in (torch.float64, torch.float32):
                head, params = build(VPRHead, inp, dtype)
                opt = torch.optim.Adam(params, lr=hr.LR)
                losses = []
                for t in range(hr.TRAJECTORY_STEPS):
                    opt.zero_grad()
                    losses.append(float(step(head, inp, dtype, hr.MARGIN)["loss"]))
                    opt.step()
                    if t + 1 == hr.PARAM_STEPS:
                        kept = [p.detach().numpy().copy() for p in params]
                traj[dtype] = (np.asarray(losses, np.float64), kept)
            losses64, kept = traj[torch.float64]
            data.update(losses=losses64, lr=np.float64(hr.LR), err32_losses=np.float64(np.abs(traj[torch.float32][0] - losses64).max()))
            data.update({f"p{i}_after": hr.stored(p) for i, p in enumerate(kept)})
        path = os.path.join(hr.GOLDEN, f"case_{name}.npz")
        np.savez_compressed(path, **data)
        print(f"case_{name}.npz: {os.path.getsize(path)} B  loss {float(r64['loss'])!r}  active {ours['n_active']} of {sum(inp['counts'])}  "
              f"min|hinge| {np.abs(ours['hinge']).min():.2e}  oracle-vs-reference gradients {worst:.1e}")
        print("  fp32 error: loss %.1e " % data["err32_loss"] + " ".join(f"{g} {float(data['err32_' + g]):.1e}" for g in tuple(hr.GROUPS) + hr.MAPS))
        if "losses" in data:
            print("  losses", " ".join(f"{v:.6f}" for v in data["losses"]), f" fp32-vs-fp64 {data['err32_losses']:.1e}")
    assert active >= 1 and inactive >= 1, (active, inactive)
    print(f"triplets across the cases: {active} active, {inactive} inactive")


if __name__ == "__main__":
    main()
