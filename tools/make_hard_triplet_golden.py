"""Generate tests/golden/hard_triplet/*.npz from the REFERENCE, loaded read-only from a checkout of it:

* its HardTripletLoss (src/kp2dtiny/utils/losses.py, from its own file) in float64 and in float32 under torch autograd on
  the loss cases of tests/hard_triplet_ref.LOSS_CASES, each in hardest and in batch-all mode.  The hardest runs build it
  the way the multitask run does, HardTripletLoss(margin=0.5, hardest=True): its branch adds the literal 0.1;
* its VPRHead (as tools/make_vpr_head_training_golden.py and make_vpr_head_bn_golden.py load it) with that loss on
  cat(vlad, vlad_aug) and cat(arange(N), arange(N)) and torch.optim.Adam on the trainer cases: .eval() for the
  running-statistics steps, .train() with Dropout2d(0.2) for the batch-statistics steps, where each view is its own call
  of the head (the reference's two keypoint_net(...) calls) and the masks its Dropout2d drew are recorded; and its NetVLAD
  layer alone on encoder maps.

    python3 tools/make_hard_triplet_golden.py --reference PATH        (or KP2D_REFERENCE=PATH)

Each fixture holds outputs, settings, seeds and the recorded masks only (the inputs are regenerated from seeds); an array of
more than MAX_STORED entries keeps every stride_of(size)-th entry (hard_triplet_ref.stored), and the float64 numpy oracle
of tests/hard_triplet_ref.py, held to the stored entries to 1e-10, stands in for the whole array.  err32_* is the error of
the SAME module run in float32 on the CPU against its float64 run, per tensor (E = max|G - G64| / max|G64|; for a loss the
absolute difference; for a tensor that is zero everywhere the absolute difference too).

Asserted here, conditions on the inputs: in cases B, C and D between a quarter and three quarters of the anchors have an
active hinge; every hinge and every arg-max / arg-min gap that decides a gradient is at least 100 x its own float32 error
(hard_triplet_ref.own_error: 4 x 2^-24 x the largest distance) away from flipping, and the reference's float32 run decides
as its float64 run does, so the yardstick measures rounding and not a flipped hinge (cases F and G, whose ties are the
point, are exempt from the gap condition); in the trainer cases the same holds at every step, against twice the float32
error of vlad itself.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_vpr_head_bn_golden import MaskRecorder, build_train  # noqa: E402
from make_vpr_head_training_golden import build, reference_vpr_head  # noqa: E402


def reference_losses(reference):
    reference = os.path.realpath(reference)
    path = os.path.join(reference, "src", "kp2dtiny", "utils", "losses.py")
    spec = importlib.util.spec_from_file_location("kp2d_reference_losses", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.realpath(mod.__file__).startswith(reference + os.sep):
        raise RuntimeError("losses.py resolved outside the reference")
    return mod


def err(a, b):
    """E(a against b): relative to max|b|, absolute where b is zero everywhere."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    top = np.abs(b).max() if b.size else 0.0
    return float(np.abs(a - b).max() / top) if top > 0 else float(np.abs(a - b).max() if b.size else 0.0)


def loss_fixtures(losses, tr):
    for name, (M, dim, _, noise, seed, squared) in tr.LOSS_CASES.items():
        emb, labels = tr.make_loss_inputs(name)
        for mode in tr.MODES:
            hardest = mode == "hardest"
            crit = losses.HardTripletLoss(margin=0.5, hardest=True, squared=squared) if hardest else \
                losses.HardTripletLoss(margin=tr.BATCH_ALL_MARGIN, hardest=False, squared=squared)
            margin = tr.QUIRK_MARGIN if hardest else tr.BATCH_ALL_MARGIN
            runs = {}
            for dtype in (torch.float64, torch.float32):
                x = torch.from_numpy(emb).to(dtype).requires_grad_(True)
                loss = crit(x, torch.from_numpy(labels))
                loss.backward()
                with torch.no_grad():
                    d = losses._pairwise_distance(x, squared=squared)
                runs[dtype] = (float(loss.detach()), x.grad.numpy().copy(), d.numpy().astype(np.float64))
            (l64, g64, d64), (l32, g32, d32) = runs[torch.float64], runs[torch.float32]
            ours = tr.hard_triplet(emb, labels, margin, hardest, squared)
            derr = float(np.abs(d32 - d64).max())
            assert np.abs(ours["d"] - d64).max() <= 1e-10, (name, mode, np.abs(ours["d"] - d64).max())
            assert abs(ours["loss"] - l64) <= 1e-10 and np.abs(ours["demb"] - g64).max() <= 1e-10, (name, mode, abs(ours["loss"] - l64), np.abs(ours["demb"] - g64).max())
            hinge_gap = tr.hinge_gap(ours)
            gap = tr.hardest_gaps(emb, labels, squared) if hardest else np.inf
            own = tr.own_error(emb, squared)
            assert hinge_gap >= 100 * own, (name, mode, hinge_gap, own)
            if name not in ("F", "G"):
                assert gap >= 100 * own, (name, mode, gap, own)
                in32 = tr.hard_triplet(emb, labels, margin, hardest, squared, d=d32)      # what the float32 run decided
                assert tr.decisions(in32) == tr.decisions(ours), (name, mode, "the float32 run decides differently")
            if name in ("B", "C", "D") and hardest:
                assert M / 4 <= ours["stats"][0] <= 3 * M / 4, (name, ours["stats"])
            if name == "F":
                assert ours["stats"][3] == 2 and d64[0, 1] == 0 and d64[1, 0] == 0
            if name == "G" and hardest:
                assert l64 == 0.1 and not g64.any()
            data = dict(loss=np.float64(l64), demb=tr.stored(g64), stats=ours["stats"], margin=np.float64(margin), seed=np.int64(seed),
                        noise=np.float64(noise), squared=np.int64(squared), max_stored=np.int64(tr.MAX_STORED),
                        err32_loss=np.float64(abs(l32 - l64)), err32_demb=np.float64(err(g32, g64)), err32_dist=np.float64(derr))
            path = os.path.join(tr.GOLDEN, f"loss_{name}_{mode}.npz")
            np.savez_compressed(path, **data)
            print(f"loss_{name}_{mode}.npz: {os.path.getsize(path)} B  loss {l64!r}  stats {ours['stats'].tolist()}  min|hinge| {hinge_gap:.1e}  "
                  f"arg gap {gap:.1e}  fp32 error: distances {derr:.1e} loss {abs(l32 - l64):.1e} demb {data['err32_demb']:.1e}")


def _crit(losses):
    return losses.HardTripletLoss(margin=0.5, hardest=True)      # KeypointNetwithIOLoss.py's construction


def head_step(head, crit, feats, dtype, masks):
    """One batch of pairs through the reference's head, a call per view -> dict of detached tensors; .grad are set.
    masks None: the head's own Dropout2d where it is in .train(), else the given (mask, mask_aug) factors."""
    ys, vs = [], []
    for i, f in enumerate(feats):
        x = torch.from_numpy(f).to(dtype)
        y1 = head.convlad1(x)
        if masks is not None:
            y1 = y1 * torch.from_numpy(masks[i]).to(dtype)[:, :, None, None]
        elif head.training and head.with_drop:
            y1 = head.dropout(y1)
        y3 = head.convlad3(head.convlad2(y1))
        if not head.training:
            with torch.no_grad():
                assert torch.equal(head(x), head.netvlad(y3)), "VPRHead.forward is not the layer sequence restated here"
        ys.append(y3)
        vs.append(head.netvlad(y3))
    vlad = torch.cat(vs)
    vlad.retain_grad()
    N = feats[0].shape[0]
    labels = torch.cat([torch.arange(N), torch.arange(N)])
    loss = crit(vlad, labels)
    loss.backward()
    return {"loss": float(loss), "vlad": vlad.detach().numpy().copy(), "dvlad": vlad.grad.numpy().copy(),
            "y3": torch.cat(ys).detach().numpy().copy()}


def head_fixture(VPRHead, losses, tr, case, batch):
    inp = tr.make_trainer_inputs(case)
    steps = tr.BATCH_STEPS if batch else tr.RUNNING_STEPS
    seed = tr.TRAINER_CASES[case][3] + 50
    layers_of = lambda head: (head.convlad1, head.convlad2, head.convlad3)      # noqa: E731
    runs, drops = {}, None
    for dtype in (torch.float64, torch.float32):
        head, params = build_train(VPRHead, inp, dtype, with_drop=True) if batch else build(VPRHead, inp, dtype)
        opt = torch.optim.Adam(params, lr=tr.LR)
        rec = MaskRecorder(head.dropout) if batch and drops is None else None
        torch.manual_seed(seed)
        r = {"losses": [], "vlads": []}
        for t in range(steps):
            opt.zero_grad()
            s = head_step(head, _crit(losses), (inp["feat"], inp["feat_aug"]), dtype, None if drops is None else drops[t])
            r["losses"].append(s["loss"])
            r["vlads"].append(s["vlad"])
            if t == 0:
                r.update(first=s, grads=[p.grad.numpy().copy() for p in params],
                         rstats=[(l.bn.running_mean.numpy().copy(), l.bn.running_var.numpy().copy()) for l in layers_of(head)])
            opt.step()
        r["after"] = [p.detach().numpy().copy() for p in params]
        r["rstats_after"] = [(l.bn.running_mean.numpy().copy(), l.bn.running_var.numpy().copy()) for l in layers_of(head)]
        r["tracked"] = [int(l.bn.num_batches_tracked) for l in layers_of(head)]
        if rec is not None:
            assert len(rec.masks) == 2 * steps
            drops = [(rec.masks[2 * t], rec.masks[2 * t + 1]) for t in range(steps)]
        runs[dtype] = r
    r64, r32 = runs[torch.float64], runs[torch.float32]
    if batch:
        assert r64["tracked"] == [2 * steps] * 3, r64["tracked"]
    ours = tr.head_views_gradients(inp["feat"], inp["feat_aug"], inp["params"], inp["stats"], inp["slope"], batch, None if drops is None else drops[0])
    worst = max(err(np.asarray(a).reshape(b.shape), b) for a, b in zip(ours["grads"], r64["grads"]))
    worst = max(worst, err(ours["vlad"], r64["first"]["vlad"]), err(ours["dvlad"], r64["first"]["dvlad"]), abs(ours["loss"] - r64["first"]["loss"]))
    assert worst <= 1e-9, worst
    verr = max(float(np.abs(a - b).max()) for a, b in zip(r32["vlads"], r64["vlads"]))
    for v32, v64 in zip(r32["vlads"], r64["vlads"]):
        a, b = (tr.hard_triplet(v, tr.view_labels(tr.PAIRS), tr.QUIRK_MARGIN) for v in (v32, v64))
        assert a["picks"] == b["picks"] and np.array_equal(a["hinge"] > 0, b["hinge"] > 0)
        assert min(tr.hinge_gap(b), tr.hardest_gaps(v64, tr.view_labels(tr.PAIRS))) >= 100 * 2 * verr, (tr.hinge_gap(b), verr)
    assert 1 <= ours["stats"][0] < (2 * tr.PAIRS + (1 if batch else 0)), ours["stats"]      # (two dropout masks pull every pair apart)
    first = r64["first"]
    data = dict(loss=np.float64(first["loss"]), vlad=tr.stored(first["vlad"]), dvlad=tr.stored(first["dvlad"]), y3=tr.stored(first["y3"]),
                stats=ours["stats"], losses=np.asarray(r64["losses"]), lr=np.float64(tr.LR), torch_seed=np.int64(seed),
                max_stored=np.int64(tr.MAX_STORED), err32_loss=np.float64(abs(r32["first"]["loss"] - first["loss"])),
                err32_losses=np.float64(np.abs(np.asarray(r32["losses"]) - np.asarray(r64["losses"])).max()),
                err32_vlad=np.float64(err(r32["first"]["vlad"], first["vlad"])), err32_dvlad=np.float64(err(r32["first"]["dvlad"], first["dvlad"])),
                err32_y3=np.float64(err(r32["first"]["y3"], first["y3"])))
    for i, (g32, g64) in enumerate(zip(r32["grads"], r64["grads"])):
        data[f"g{i}"], data[f"err32_g{i}"] = tr.stored(g64), np.float64(err(g32, g64))
    for i, p in enumerate(r64["after"]):
        data[f"p{i}_after"] = tr.stored(p)
    if batch:
        data["masks"] = np.stack([np.stack(d) for d in drops])
        for key in ("rstats", "rstats_after"):
            worst32 = 0.0
            for i, ((m64, v64), (m32, v32)) in enumerate(zip(r64[key], r32[key]), 1):
                data[f"{key}_mean{i}"], data[f"{key}_var{i}"] = m64, v64
                worst32 = max(worst32, err(m32, m64), err(v32, v64))
            data["err32_" + key] = np.float64(worst32)
    path = os.path.join(tr.GOLDEN, f"head_{case}_{'batch' if batch else 'running'}.npz")
    np.savez_compressed(path, **data)
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} B  losses {' '.join(f'{v:.6f}' for v in r64['losses'])}  stats {ours['stats'].tolist()}  "
          f"oracle-vs-reference {worst:.1e}  fp32 error: loss {data['err32_loss']:.1e} vlad {data['err32_vlad']:.1e} dvlad {data['err32_dvlad']:.1e} "
          f"gradients {max(float(data[f'err32_g{i}']) for i in range(11)):.1e}")


def netvlad_fixture(VPRHead, losses, tr, case):
    inp = tr.make_trainer_inputs(case)
    steps = tr.RUNNING_STEPS
    runs = {}
    for dtype in (torch.float64, torch.float32):
        head, params = build(VPRHead, inp, dtype)
        params = params[9:]
        opt = torch.optim.Adam(params, lr=tr.LR)
        r = {"losses": [], "vlads": []}
        for t in range(steps):
            opt.zero_grad()
            vlad = torch.cat([head.netvlad(torch.from_numpy(inp[k]).to(dtype)) for k in ("enc", "enc_aug")])
            vlad.retain_grad()
            loss = _crit(losses)(vlad, torch.cat([torch.arange(tr.PAIRS), torch.arange(tr.PAIRS)]))
            loss.backward()
            r["losses"].append(float(loss))
            r["vlads"].append(vlad.detach().numpy().copy())
            if t == 0:
                r.update(vlad=vlad.detach().numpy().copy(), dvlad=vlad.grad.numpy().copy(), grads=[p.grad.numpy().copy() for p in params])
            opt.step()
        r["after"] = [p.detach().numpy().copy() for p in params]
        runs[dtype] = r
    r64, r32 = runs[torch.float64], runs[torch.float32]
    K, C = inp["K"], inp["C"]
    ours = tr.netvlad_views_gradients(inp["enc"], inp["enc_aug"], inp["params"][9].reshape(K, C), inp["params"][10])
    worst = max(err(ours["dW"].reshape(r64["grads"][0].shape), r64["grads"][0]), err(ours["dcent"], r64["grads"][1]), err(ours["vlad"], r64["vlad"]),
                err(ours["dvlad"], r64["dvlad"]), abs(ours["loss"] - r64["losses"][0]))
    assert worst <= 1e-9, worst
    verr = max(float(np.abs(a - b).max()) for a, b in zip(r32["vlads"], r64["vlads"]))
    for v32, v64 in zip(r32["vlads"], r64["vlads"]):
        a, b = (tr.hard_triplet(v, tr.view_labels(tr.PAIRS), tr.QUIRK_MARGIN) for v in (v32, v64))
        assert a["picks"] == b["picks"] and np.array_equal(a["hinge"] > 0, b["hinge"] > 0)
        assert min(tr.hinge_gap(b), tr.hardest_gaps(v64, tr.view_labels(tr.PAIRS))) >= 100 * 2 * verr, (tr.hinge_gap(b), verr)
    assert 1 <= ours["stats"][0] < 2 * tr.PAIRS, ours["stats"]
    data = dict(loss=np.float64(r64["losses"][0]), vlad=tr.stored(r64["vlad"]), dvlad=tr.stored(r64["dvlad"]), stats=ours["stats"],
                losses=np.asarray(r64["losses"]), lr=np.float64(tr.LR), max_stored=np.int64(tr.MAX_STORED),
                err32_loss=np.float64(abs(r32["losses"][0] - r64["losses"][0])),
                err32_losses=np.float64(np.abs(np.asarray(r32["losses"]) - np.asarray(r64["losses"])).max()),
                err32_vlad=np.float64(err(r32["vlad"], r64["vlad"])), err32_dvlad=np.float64(err(r32["dvlad"], r64["dvlad"])))
    for i, k in enumerate(("dW", "dcent")):
        data[k], data["err32_" + k] = tr.stored(r64["grads"][i]), np.float64(err(r32["grads"][i], r64["grads"][i]))
    data["W_after"], data["cent_after"] = tr.stored(r64["after"][0]), tr.stored(r64["after"][1])
    path = os.path.join(tr.GOLDEN, f"netvlad_{case}.npz")
    np.savez_compressed(path, **data)
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} B  losses {' '.join(f'{v:.6f}' for v in r64['losses'])}  stats {ours['stats'].tolist()}  "
          f"oracle-vs-reference {worst:.1e}  fp32 error: loss {data['err32_loss']:.1e} vlad {data['err32_vlad']:.1e} dvlad {data['err32_dvlad']:.1e} "
          f"dW {data['err32_dW']:.1e} dcent {data['err32_dcent']:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("KP2D_REFERENCE"), help="a checkout of the reference project")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        raise SystemExit("needs --reference PATH (or KP2D_REFERENCE): a checkout of the reference project")
    losses = reference_losses(args.reference)
    VPRHead = reference_vpr_head(args.reference)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import hard_triplet_ref as tr
    os.makedirs(tr.GOLDEN, exist_ok=True)
    a, b = (float(losses.HardTripletLoss(margin=m, hardest=True)(torch.from_numpy(tr.make_loss_inputs("B")[0]).double(),
                                                                 torch.from_numpy(tr.make_loss_inputs("B")[1]))) for m in (0.5, 0.9))
    assert a == b, "the reference's hardest branch reads its margin after all"
    print(f"the margin quirk: hardest=True gives {a!r} at margin 0.5 and at 0.9")
    loss_fixtures(losses, tr)
    for case in tr.TRAINER_CASES:
        head_fixture(VPRHead, losses, tr, case, batch=False)
        head_fixture(VPRHead, losses, tr, case, batch=True)
        netvlad_fixture(VPRHead, losses, tr, case)


if __name__ == "__main__":
    main()
