"""Generate tests/golden/keypoint_training/ by running the REFERENCE's own KeypointNetwithIOLoss.forward
(src/kp2dtiny/models/KeypointNetwithIOLoss.py: its keypoint block, build_descriptor_loss and the helpers they call), loaded
read-only from a checkout of the reference, under torch autograd in float64 on the cases of tests/keypoint_training_ref; and
the same in float32, the yardstick of the GPU tests' bounds.

    python3 tools/make_keypoint_training_golden.py --reference PATH        (or KP2D_REFERENCE=PATH)

How the reference's module is run without its training stack: it imports cv2, torchgeometry and
segmentation_models_pytorch at module level, none of which the keypoint block reaches; EMPTY stand-in modules are registered
under exactly those names in THIS process before the import.  The object is built without its __init__ (object.__new__ plus
torch.nn.Module.__init__), with with_io = False and the segmentation, place-recognition and depth flags off, and a
``keypoint_net`` stand-in whose call returns the prepared maps (the loss cases) or runs the reference's own SimpleTaskHead /
UpscaleHead (modules/decoders/heads.py) in .eval() on prepared backbone maps (the trainer case), and whose post_processing /
remove_border are KP2DTinyV2's own functions.

The reference accumulates its total into a float32 tensor in place, so of a float64 run the loss-dict parts and every gradient
are float64 and the total is rounded to float32; the consistency term appears in no dict entry.  Stored per case
(case_*.npz): loc_loss, metric_loss, usp_loss as the dict gives them (loc and usp carry their weights), total, recall, the six
gradients (of an array of more than MAX_STORED entries every stride_of(size)-th entry), the counts, usp_abs (the float64
mean of |summand| behind usp) and err32_*: the error of the float32 run against the float64 run, E = max|G - G64| / max|G64|
per gradient, relative for a scalar, for usp relative to usp_abs.  err32_con alone comes from three torch calls restated
here (grid_sample, mse_loss on the reference's own decoded maps), since the reference exposes the term nowhere.  trainer.npz:
the heads' outputs, the 20 gradients and five Adam steps (the loss of and the parameters after every step), with err32_*.
seeds.json: the seed each case's inputs are regenerated from.

A seed is refused (seed + 1000, ..., at most 1000 times) unless every discrete choice is safe against float32 error, each by
100 x that quantity's own float32 error, element by element: the gap between the best and second best of each a_i, |d_i - 4|,
the margin of every pair's relax_field decision (a pair inside the field: the smaller of r - |dx| and r - |dy|; a pair outside
it: the larger of |dx| - r and |dy| - r, since one coordinate safely outside decides the pair whatever the other does)
against the summed float32 errors of the two points, the gap between each anchor's best and second-best admissible negative, every hinge
argument's distance from 0, every decoded coordinate's distance from its clamp ends, d_i away from 0; and the float32 run
gives the float64 run's recall.
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAND_INS = ("cv2", "torchgeometry", "segmentation_models_pytorch")


def reference_modules(reference):
    """-> (KeypointNetwithIOLoss module, kp2dtiny module, heads module) of the reference, empty stand-ins registered first."""
    reference = os.path.realpath(reference)
    for name in STAND_INS:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, reference)
    import importlib
    loss = importlib.import_module("src.kp2dtiny.models.KeypointNetwithIOLoss")
    net = importlib.import_module("src.kp2dtiny.models.kp2dtiny")
    heads = importlib.import_module("src.kp2dtiny.modules.decoders.heads")
    for mod in (loss, net, heads):
        if not os.path.realpath(mod.__file__).startswith(reference + os.sep):
            raise RuntimeError(f"{mod.__file__}: fixtures must come from the reference under {reference}")
    return loss, net, heads


class KeypointNetStandIn:
    """What KeypointNetwithIOLoss.forward needs of its keypoint_net: a call per view (the augmented view first) and
    KP2DTinyV2's post_processing / remove_border in training mode."""

    training = True
    cross_ratio = 2.0

    def __init__(self, net, cell, views):
        self.cell, self._views = cell, list(views)
        self.post_processing = types.MethodType(net.KP2DTinyV2.post_processing, self)
        self.remove_border = types.MethodType(net.KP2DTinyV2.remove_border, self)

    def __call__(self, image):
        return dict(self._views.pop(0)())


def loss_object(loss_mod, keypoint_net, weights):
    obj = object.__new__(loss_mod.KeypointNetwithIOLoss)
    torch.nn.Module.__init__(obj)
    obj.device, obj.debug, obj.relax_field = "cpu", False, 4
    obj.loc_loss_weight, obj.descriptor_loss_weight, obj.score_loss_weight, obj.keypoint_loss_weight = weights
    obj.segmentation_loss_weight = obj.vlad_loss_weight = obj.depth_loss_weight = obj.io_loss_weight = 0.0
    obj.descriptor_loss, obj.with_io, obj.train_keypoints = True, False, True
    obj.train_segmentation = obj.train_visloc = obj.train_depth = False
    obj.__dict__["keypoint_net"] = keypoint_net
    return obj


def run_reference(loss_mod, net, views, hom, H, W, cell, weights, dtype):
    """views: (target, source) callables -> dict of maps.  -> (total, loss_dict, recall, the decoded (out, out_aug))"""
    B = hom.shape[0]
    seen = []

    def keep(fn):
        def call():
            seen.append(fn())
            return seen[-1]
        return call

    stand_in = KeypointNetStandIn(net, cell, [keep(views[1]), keep(views[0])])      # forward asks for the augmented view first
    obj = loss_object(loss_mod, stand_in, weights)
    image = torch.zeros(B, 3, H, W, dtype=dtype)
    total, parts, recall = obj.forward({"image": image, "image_aug": image, "homography": torch.from_numpy(hom).to(dtype)})
    return total, parts, recall


def consistency(tgt, src, hom, H, W, cell, net, loss_mod, dtype):
    """2 MSE as the reference forms it, restated from three of its lines for err32_con alone."""
    stand_in = KeypointNetStandIn(net, cell, [])
    with torch.no_grad():
        t = stand_in.post_processing({k: torch.from_numpy(v).to(dtype) for k, v in (("score", tgt["score"]), ("coord", tgt["shift"]), ("feat", tgt["feat"]))}, H, W)
        s = stand_in.post_processing({k: torch.from_numpy(v).to(dtype) for k, v in (("score", src["score"]), ("coord", src["shift"]), ("feat", src["feat"]))}, H, W)
        B, _, Hc, Wc = t["score"].shape
        obj = loss_object(loss_mod, stand_in, (1, 1, 1, 1))
        grid = obj._warp_homography_batch(loss_mod._normalize_uv_coordinates(s["coord"], H, W), torch.from_numpy(hom).to(dtype))
        mask = loss_mod._create_border_mask(B, Hc, Wc).gt(1e-3).unsqueeze(1)
        res = torch.nn.functional.grid_sample(t["score"], grid, mode="bilinear", align_corners=True)
        return float(torch.nn.functional.mse_loss(res[mask], s["score"][mask]) * 2) if mask.any() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("KP2D_REFERENCE"), help="a checkout of the reference project")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        raise SystemExit("needs --reference PATH (or KP2D_REFERENCE): a checkout of the reference project")
    loss_mod, net, heads = reference_modules(args.reference)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import keypoint_training_ref as kr
    os.makedirs(kr.GOLDEN, exist_ok=True)
    seeds = {}

    def scalar_err(a, b):
        return np.float64(abs(a - b) / abs(b)) if b else np.float64(abs(a - b))

    # ---- the loss alone ----
    def run_loss(inp, dtype):
        leaves = []

        def view(v):
            def make():
                t = {k: torch.from_numpy(v[k]).to(dtype).requires_grad_(True) for k in ("score", "shift", "feat")}
                leaves.append(t)
                return {"score": t["score"], "coord": t["shift"], "feat": t["feat"]}
            return make

        total, parts, recall = run_reference(loss_mod, net, (view(inp["tgt"]), view(inp["src"])), inp["hom"], inp["H"], inp["W"],
                                             inp["cell"], inp["weights"], dtype)
        total.backward()
        src, tgt = leaves          # the augmented view was asked for first
        out = {"total": float(total), "loc_loss": float(parts["loc_loss"]), "metric_loss": float(parts["metric_loss"]),
               "usp_loss": float(parts["usp_loss"]), "recall": float(recall), "total_dtype": total.dtype}
        for k in ("score", "shift", "feat"):
            out[f"d{k}_t"] = (tgt[k].grad if tgt[k].grad is not None else torch.zeros_like(tgt[k])).numpy()
            out[f"d{k}_s"] = (src[k].grad if src[k].grad is not None else torch.zeros_like(src[k])).numpy()
        return out

    for name in kr.LOSS_CASES:
        seed, tries = kr.BASE_SEED[name], 0
        while True:
            inp = kr.make_loss_inputs(name, seed)
            call = (inp["tgt"], inp["src"], inp["hom"], inp["H"], inp["W"], inp["cell"], inp["weights"])
            o64, o32 = kr.keypoint_loss(*call), kr.keypoint_loss(*call, dtype=np.float32, grads=False)
            why = kr.conditions(o64, o32)
            if why is None:
                r64, r32 = run_loss(inp, torch.float64), run_loss(inp, torch.float32)
                if r64["recall"] != r32["recall"]:
                    why = "the reference's float32 run gives another recall"
            if why is None:
                break
            print(f"case {name}: seed {seed} refused: {why}")
            seed, tries = seed + 1000, tries + 1
            if tries >= 1000:
                raise SystemExit(f"case {name}: 1000 seeds refused")
        seeds[name] = seed
        assert r64["total_dtype"] == torch.float32, "the reference's total is expected to be a float32 tensor"
        lw, dw, sw, kw = inp["weights"]
        c64, c32 = (consistency(inp["tgt"], inp["src"], inp["hom"], inp["H"], inp["W"], inp["cell"], net, loss_mod, t)
                    for t in (torch.float64, torch.float32))
        data = {"total": np.float64(r64["total"]), "loc_loss": np.float64(r64["loc_loss"]), "metric_loss": np.float64(r64["metric_loss"]),
                "usp_loss": np.float64(r64["usp_loss"]), "con": np.float64(c64), "recall": np.float64(r64["recall"]),
                "M": np.int64(o64["M"]), "n": np.int64(o64["n"]), "hits": np.int64(o64["hits"]), "usp_abs": np.float64(o64["usp_abs"]),
                "weights": np.asarray(inp["weights"], np.float64), "seed": np.int64(seed), "max_stored": np.int64(kr.MAX_STORED),
                "err32_loss": scalar_err(r32["total"], r64["total"]), "err32_loc": scalar_err(r32["loc_loss"], r64["loc_loss"]),
                "err32_metric": scalar_err(r32["metric_loss"], r64["metric_loss"]),
                "err32_usp": np.float64(abs(r32["usp_loss"] - r64["usp_loss"]) / sw / o64["usp_abs"]) if o64["M"] else np.float64(0.0),
                "err32_con": scalar_err(c32, c64)}
        for k in kr.GRADS:
            data[k] = kr.stored(r64[k])
            data["err32_" + k] = np.float64(kr.rel_err(r32[k], r64[k])) if np.abs(r64[k]).max() > 0 else np.float64(0.0)
        worst = max([kr.rel_err(o64[k], r64[k]) for k in kr.GRADS if np.abs(r64[k]).max() > 0] +
                    [abs(lw * o64["loc"] - r64["loc_loss"]), abs(o64["metric"] - r64["metric_loss"]), abs(sw * o64["usp"] - r64["usp_loss"]),
                     abs(o64["con"] - c64), abs(o64["recall"] - r64["recall"])])
        path = os.path.join(kr.GOLDEN, f"case_{name}.npz")
        np.savez_compressed(path, **data)
        outside = int((np.abs(o64["q"]["wn"]) > 1).any(axis=0).sum())
        print(f"case_{name}.npz: {os.path.getsize(path)} B  seed {seed}  total {r64['total']!r}  loc {r64['loc_loss']:.6f} metric "
              f"{r64['metric_loss']:.6f} usp {r64['usp_loss']:.6f} con {c64:.6f}  M {o64['M']} n {o64['n']} hits {o64['hits']}  "
              f"warped points outside the image {outside}  oracle-vs-reference {worst:.1e} (total: {abs(o64['loss'] - r64['total']) / abs(r64['total']):.1e})")
        print("  fp32 error: " + ", ".join(f"{k} {float(data['err32_' + k]):.1e}" for k in kr.LOSS_KEYS))

    # ---- the trainer: the reference's own heads in .eval(), five Adam steps ----
    t = kr.TRAINER
    c3, c4 = t["c3"], t["c4"]

    def build(inp, dtype):
        score = heads.SimpleTaskHead(c4, c4, 1, with_drop=True, leaky_relu=True)
        loc = heads.SimpleTaskHead(c4, c4, 2, with_drop=True, leaky_relu=True)
        desc = heads.UpscaleHead(c4, c4, c3 * 4, c3 + c4, c4, t["nfeat"], True, leaky_relu=True)
        mods = torch.nn.ModuleDict({"score_head": score, "loc_head": loc, "desc_head": desc}).to(dtype).eval()
        named = dict(mods.named_parameters())
        assert [k for k in named if k in kr.PARAMS] == list(kr.PARAMS) and len(named) == 20, "not the reference's registration order"
        params = [named[k] for k in kr.PARAMS]
        with torch.no_grad():
            for p, a in zip(params, inp["params"]):
                p.copy_(torch.from_numpy(a).to(dtype))
            for bn, (mean, var) in zip((score.convDa.bn, loc.convDa.bn, desc.convA.bn, desc.confAa.bn), inp["stats"]):
                bn.running_mean.copy_(torch.from_numpy(mean).to(dtype))
                bn.running_var.copy_(torch.from_numpy(var).to(dtype))
        return mods, params

    def trainer_step(mods, inp, dtype):
        B = inp["B"]
        x, skip = torch.from_numpy(inp["x"]).to(dtype), torch.from_numpy(inp["skip"]).to(dtype)
        outs = []

        def view(sl):
            def make():
                o = {"score": mods["score_head"](x[sl]).sigmoid(), "coord": mods["loc_head"](x[sl]).tanh(), "feat": mods["desc_head"](x[sl], skip[sl])}
                outs.append({k: v.detach().clone() for k, v in o.items()})
                return o
            return make

        total, parts, recall = run_reference(loss_mod, net, (view(slice(0, B)), view(slice(B, 2 * B))), inp["hom"], inp["H"], inp["W"],
                                             inp["cell"], inp["weights"], dtype)
        total.backward()
        src, tgt = outs
        return float(total), float(recall), {k: torch.cat([tgt[k], src[k]]).numpy() for k in ("score", "coord", "feat")}

    seed, tries = kr.BASE_SEED["T"], 0
    while True:
        inp = kr.make_trainer_inputs(seed)
        ok = True
        runs = {}
        for dtype in (torch.float64, torch.float32):
            mods, params = build(inp, dtype)
            opt = torch.optim.Adam(params, lr=kr.LR)
            losses, after, first = [], [], None
            for step in range(kr.STEPS):
                opt.zero_grad()
                total, recall, outs = trainer_step(mods, inp, dtype)
                if step == 0:
                    first = (outs, [p.grad.detach().numpy().copy() for p in params], recall)
                losses.append(total)
                opt.step()
                after.append([p.detach().numpy().copy() for p in params])
            runs[dtype] = (np.asarray(losses, np.float64), after, first)
        # the conditions, on the oracle's walk, at every step of the trajectory
        oparams = [p.astype(np.float64) for p in inp["params"]]
        olosses, oafter = kr.trajectory(inp)
        why = None
        for step_params in [oparams] + oafter[:-1]:
            f64 = kr.heads_forward(inp, step_params)
            B = inp["B"]
            call = ({k: f64[k][:B] for k in ("score", "shift", "feat")}, {k: f64[k][B:] for k in ("score", "shift", "feat")},
                    inp["hom"], inp["H"], inp["W"], inp["cell"], inp["weights"])
            why = why or kr.conditions(kr.keypoint_loss(*call, grads=False), kr.keypoint_loss(*call, dtype=np.float32, grads=False))
        if why is None and runs[torch.float64][2][2] != runs[torch.float32][2][2]:
            why = "the reference's float32 run gives another recall"
        if why is None:
            break
        print(f"trainer: seed {seed} refused: {why}")
        seed, tries = seed + 1000, tries + 1
        if tries >= 1000:
            raise SystemExit("trainer: 1000 seeds refused")
    seeds["T"] = seed
    (l64, a64, (o64, g64, rec)), (l32, a32, (o32, g32, _)) = runs[torch.float64], runs[torch.float32]
    data = {"losses": l64, "err32_losses": np.float64((np.abs(l32 - l64) / np.abs(l64)).max()), "recall": np.float64(rec),
            "lr": np.float64(kr.LR), "seed": np.int64(seed)}
    for k in ("score", "coord", "feat"):
        data[k] = kr.stored(o64[k])
        data["err32_" + k] = np.float64(kr.rel_err(o32[k], o64[k]))
    for i in range(20):
        data[f"g{i}"] = kr.stored(g64[i])
        data[f"err32_g{i}"] = np.float64(kr.rel_err(g32[i], g64[i]))
        data[f"p{i}"] = np.stack([kr.stored(a[i], kr.TRAJ_STORED) for a in a64])
        data[f"err32_p{i}"] = np.float64(max(kr.rel_err(b[i], a[i]) for a, b in zip(a64, a32)))
    s = kr.step_gradients(inp)
    worst = max(kr.rel_err(np.asarray(a).reshape(b.shape), b) for a, b in zip(s["grads"], g64))
    path = os.path.join(kr.GOLDEN, "trainer.npz")
    np.savez_compressed(path, **data)
    print(f"trainer.npz: {os.path.getsize(path)} B  seed {seed}  losses", " ".join(f"{v:.6f}" for v in l64),
          f" oracle-vs-reference gradients {worst:.1e}, losses {np.abs(olosses - l64).max():.1e}")
    print("  fp32 error: losses %.1e, outputs %.1e, gradients %.1e, parameters %.1e" % (
        data["err32_losses"], max(float(data["err32_" + k]) for k in ("score", "coord", "feat")),
        max(float(data[f"err32_g{i}"]) for i in range(20)), max(float(data[f"err32_p{i}"]) for i in range(20))))
    with open(os.path.join(kr.GOLDEN, "seeds.json"), "w") as f:
        json.dump(seeds, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
