"""Generate tests/golden/vlad_training/case_*.npz by running the REFERENCE's NetVLAD module
(src/kp2dtiny/modules/aggregators/netvlad.py, imported read-only from /root/reference) in float64 with torch autograd,
torch.nn.TripletMarginLoss and torch.optim.Adam, the way train_visloc.py:249-282 puts them together, on the cases of
tests/vlad_training_ref.make_inputs.

    python3 tools/make_vlad_training_golden.py

Runs only where the reference exists; no test, smoke() or bench.py reads it, they read the committed fixtures.  Each
fixture holds outputs and settings only (the inputs are regenerated from seeds): loss, dW, dcent, n_active in float64 and,
to keep a file to a few hundred KB, every fourth column of vlad and dvlad (all rows; dW and dcent, stored whole, depend on
every entry of both); err32_loss, err32_dW, err32_dcent: the error of the SAME module run in float32 on the CPU against its float64
run (|loss - loss64|, max|G - G64| / max|G64|), the yardstick of the GPU tests' bounds; and for the trajectory case the ten
losses of ten Adam steps and both parameters after three.  NetVLADMemoryEfficient is run beside NetVLAD and must agree.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REFERENCE = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_netvlad():
    """The reference's module file, and nothing else: refuses to run against anything outside /root/reference."""
    try:
        import sklearn.neighbors  # noqa: F401  (the module's import line; init_params' vladv2 branch alone uses it)
    except ImportError:
        pkg, sub = types.ModuleType("sklearn"), types.ModuleType("sklearn.neighbors")
        sub.NearestNeighbors = None
        pkg.neighbors = sub
        sys.modules.setdefault("sklearn", pkg)
        sys.modules.setdefault("sklearn.neighbors", sub)
    path = os.path.join(REFERENCE, "src", "kp2dtiny", "modules", "aggregators", "netvlad.py")
    spec = importlib.util.spec_from_file_location("reference_netvlad", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    where = os.path.realpath(mod.__file__)
    if not where.startswith(REFERENCE + os.sep):
        raise RuntimeError(f"{mod.__name__} resolved to {where}: fixtures must come from the reference under {REFERENCE}")
    return mod


def build(cls, inp, dtype):
    K, C = inp["K"], inp["C"]
    layer = cls(num_clusters=K, dim=C).to(dtype)
    with torch.no_grad():
        layer.conv.weight.copy_(torch.from_numpy(inp["W"]).to(dtype).reshape(K, C, 1, 1))
        layer.centroids.copy_(torch.from_numpy(inp["cent"]).to(dtype))
    return layer


def step(layer, inp, dtype, margin):
    """One batch through the reference's module and torch's loss -> (vlad, loss, dvlad); the parameters' .grad are set.
    The loss is the one of train_visloc.py:270-281 (one TripletMarginLoss term per (query, negative) pair, summed, divided
    by the number of negatives), written here as a single call on gathered rows: negative j belongs to query owner[j]."""
    B, counts = inp["B"], list(inp["counts"])
    total = sum(counts)
    x = torch.from_numpy(inp["x"]).to(dtype).unsqueeze(-1)              # [N, C, S, 1]: a map one pixel wide
    vlad = layer(x)
    vlad.retain_grad()
    owner = torch.repeat_interleave(torch.arange(B), torch.tensor(counts))
    criterion = torch.nn.TripletMarginLoss(margin=margin ** 0.5, p=2, reduction="sum")
    loss = criterion(vlad[:B][owner], vlad[B:2 * B][owner], vlad[2 * B:]) / total
    loss.backward()
    return vlad.detach(), loss.detach(), vlad.grad.detach()


def main():
    mod = reference_netvlad()
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import vlad_training_ref as vr
    os.makedirs(vr.GOLDEN, exist_ok=True)
    for name in vr.CASES:
        inp = vr.make_inputs(name)
        K, C = inp["K"], inp["C"]
        out = {}
        for dtype in (torch.float64, torch.float32):
            layer = build(mod.NetVLAD, inp, dtype)
            vlad, loss, dvlad = step(layer, inp, dtype, vr.MARGIN)
            out[dtype] = {"vlad": vlad.numpy(), "loss": float(loss), "dvlad": dvlad.numpy(),
                          "dW": layer.conv.weight.grad.reshape(K, C).numpy().copy(), "dcent": layer.centroids.grad.numpy().copy()}
        r64, r32 = out[torch.float64], out[torch.float32]
        eff = build(mod.NetVLADMemoryEfficient, inp, torch.float64)
        v2, l2, _ = step(eff, inp, torch.float64, vr.MARGIN)
        assert np.abs(v2.numpy() - r64["vlad"]).max() < 1e-12 and abs(float(l2) - r64["loss"]) < 1e-12
        assert vr.rel_err(eff.conv.weight.grad.reshape(K, C).numpy(), r64["dW"]) < 1e-10
        ours = vr.step_gradients(inp["x"], inp["W"], inp["cent"], inp["B"], inp["counts"])
        data = dict(vlad_cols=r64["vlad"][:, ::vr.COL_STRIDE], dvlad_cols=r64["dvlad"][:, ::vr.COL_STRIDE],
                    col_stride=np.int64(vr.COL_STRIDE), dW=r64["dW"], dcent=r64["dcent"], loss=np.float64(r64["loss"]), n_active=np.int64(ours["n_active"]), margin=np.float64(vr.MARGIN),
                    err32_loss=np.float64(abs(r32["loss"] - r64["loss"])),
                    err32_dW=np.float64(vr.rel_err(r32["dW"], r64["dW"])), err32_dcent=np.float64(vr.rel_err(r32["dcent"], r64["dcent"])))
        if name == vr.TRAJECTORY_CASE:
            traj = {}
            for dtype in (torch.float64, torch.float32):
                layer = build(mod.NetVLAD, inp, dtype)
                opt = torch.optim.Adam([layer.conv.weight, layer.centroids], lr=vr.LR)
                losses = []
                for t in range(vr.TRAJECTORY_STEPS):
                    opt.zero_grad()
                    losses.append(float(step(layer, inp, dtype, vr.MARGIN)[1]))
                    opt.step()
                    if t + 1 == vr.PARAM_STEPS:
                        kept = (layer.conv.weight.detach().reshape(K, C).numpy().copy(), layer.centroids.detach().numpy().copy())
                traj[dtype] = (np.asarray(losses, np.float64), kept)
            losses64, (W3, c3) = traj[torch.float64]
            data.update(losses=losses64, W_after=W3, cent_after=c3, lr=np.float64(vr.LR),
                        err32_losses=np.float64(np.abs(traj[torch.float32][0] - losses64).max()))
        path = os.path.join(vr.GOLDEN, f"case_{name}.npz")
        np.savez_compressed(path, **data)
        print(f"case_{name}.npz: {os.path.getsize(path)} B  loss {r64['loss']!r}  active {ours['n_active']} of {sum(inp['counts'])}  "
              f"oracle-vs-reference dW {vr.rel_err(ours['dW'], r64['dW']):.1e} dcent {vr.rel_err(ours['dcent'], r64['dcent']):.1e}  "
              f"fp32 error: loss {data['err32_loss']:.1e} dW {data['err32_dW']:.1e} dcent {data['err32_dcent']:.1e}  "
              f"min|hinge| {np.abs(ours['hinge']).min():.2e}")
        if "losses" in data:
            print("  losses", " ".join(f"{v:.6f}" for v in data["losses"]), f" fp32-vs-fp64 {data['err32_losses']:.1e}")


if __name__ == "__main__":
    main()
