"""Generate tests/golden/vpr_head_bn/*.npz by running the REFERENCE's VPRHead (loaded read-only from a checkout of the
reference by tools/make_vpr_head_training_golden.reference_vpr_head) in .train() in float64 under torch autograd: BatchNorm
on the batch's statistics with its running-statistics update, the reference's own Dropout2d(0.2) behind convlad1,
TripletMarginLoss(margin ** 0.5, p=2, reduction="sum") / nNeg and torch.optim.Adam the way train_visloc.py puts them
together, on the cases of tests/vpr_head_training_ref.make_inputs; and the same in float32, the yardstick of the GPU tests'
bounds.

    python3 tools/make_vpr_head_bn_golden.py --reference PATH        (or KP2D_REFERENCE=PATH)

The mask: under torch.manual_seed(the fixture's seed) the reference's Dropout2d module runs in the float64 pass; hooks on it
replay it on a map of ones from the same generator state, which gives its per-(frame, channel) factor exactly; asserted: the
factor is 0 or 1 / (1 - p), constant over a plane, and the module's output is its input times the factor.  The float32 pass
multiplies by the recorded factor, so both passes see one mask.  The mask is stored: it is an input of the device test.
Fixtures at p = 0 come from a head built without dropout (with_drop=False); their mask is all ones.

Each fixture holds outputs, settings and the mask only (the inputs are regenerated from seeds); an array of more than
MAX_STORED entries keeps every stride_of(size)-th entry (vpr_head_training_ref.stored), and the float64 numpy oracle of
tests/vpr_head_bn_ref.py, held to the stored entries to 1e-10, stands in for the whole array.  Stored: per layer the batch
mean and biased variance (of the BatchNorm module's input) and the running statistics after the step; y1..y3 (y1 after the
dropout), vlad, dvlad, loss, n_active; the eleven gradients g0..g10; dx_netvlad, dx3, dx2; err32_* of each: the error of the
SAME module run in float32 on the CPU against its float64 run.  The trajectory fixture adds ten Adam steps: the losses, the
mask of every step, and the parameters and running statistics after three steps.

Asserted here on the CPU, and printed: min |hinge| >= 1e-4 in every fixture, the float32 pass's n_active equals the float64
pass's, and at least one active and one inactive triplet across the set.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_vpr_head_training_golden import build, reference_vpr_head  # noqa: E402


def build_train(VPRHead, inp, dtype, with_drop):
    head, params = build(VPRHead, inp, dtype)
    head.with_drop = with_drop
    return head.train(), params


class MaskRecorder:
    """Hooks on a Dropout2d module: the factor it applied, exactly, per call."""

    def __init__(self, module):
        self.module, self.masks, self._state = module, [], None
        module.register_forward_pre_hook(self._before)
        module.register_forward_hook(self._after)

    def _before(self, module, args):
        self._state = torch.get_rng_state()

    def _after(self, module, args, output):
        after = torch.get_rng_state()
        torch.set_rng_state(self._state)
        factor = torch.nn.functional.dropout2d(torch.ones_like(args[0]), module.p, training=True)      # what the module calls
        assert torch.equal(torch.get_rng_state(), after), "the replay drew differently"
        kept = 1.0 / (1.0 - module.p)
        plane = factor[:, :, :1, :1]
        assert torch.equal(factor, plane.expand_as(factor)), "the factor varies over a plane"
        assert bool(((plane == 0) | (plane == kept)).all()), "a factor that is neither 0 nor 1 / (1 - p)"
        assert torch.equal(output, args[0] * factor)
        self.masks.append(plane[:, :, 0, 0].detach().numpy().astype(np.float32))


def step(head, inp, dtype, margin, mask=None):
    """One batch through the reference's head in .train() and torch's loss -> dict of detached tensors; the parameters'
    .grad are set.  The layers are called one by one as VPRHead.forward does; ``mask`` None: its own dropout module runs
    (with_drop) or none; else y1 is multiplied by the given factors."""
    B, counts = inp["B"], list(inp["counts"])
    total = sum(counts)
    layers = (head.convlad1, head.convlad2, head.convlad3)
    seen = []
    hooks = [l.bn.register_forward_hook(lambda m, a, o: seen.append(a[0].detach())) for l in layers]
    x = torch.from_numpy(inp["feat"]).to(dtype)
    y1 = head.convlad1(x)
    if mask is not None:
        y1 = y1 * torch.from_numpy(mask).to(dtype)[:, :, None, None]
    elif head.with_drop:
        y1 = head.dropout(y1)
    y2 = head.convlad2(y1)
    y3 = head.convlad3(y2)
    vlad = head.netvlad(y3)
    for h in hooks:
        h.remove()
    for t in (y1, y2, y3, vlad):
        t.retain_grad()
    owner = torch.repeat_interleave(torch.arange(B), torch.tensor(counts))
    criterion = torch.nn.TripletMarginLoss(margin=margin ** 0.5, p=2, reduction="sum")
    loss = criterion(vlad[:B][owner], vlad[B:2 * B][owner], vlad[2 * B:]) / total
    loss.backward()
    out = {"y1": y1.detach(), "y2": y2.detach(), "y3": y3.detach(), "vlad": vlad.detach(), "loss": loss.detach(),
           "dvlad": vlad.grad.detach(), "dx_netvlad": y3.grad.detach(), "dx3": y2.grad.detach(), "dx2": y1.grad.detach()}
    for i, (l, c) in enumerate(zip(layers, seen), 1):
        out[f"mean{i}"], out[f"var{i}"] = c.mean(dim=(0, 2, 3)), c.var(dim=(0, 2, 3), unbiased=False)
        out[f"rmean{i}"], out[f"rvar{i}"] = l.bn.running_mean.detach().clone(), l.bn.running_var.detach().clone()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("KP2D_REFERENCE"), help="a checkout of the reference project")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        raise SystemExit("needs --reference PATH (or KP2D_REFERENCE): a checkout of the reference project")
    VPRHead = reference_vpr_head(args.reference)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import vpr_head_bn_ref as br
    hr = br.hr
    os.makedirs(br.GOLDEN, exist_ok=True)
    active = inactive = 0
    for fname, (case, p, seed) in br.FIXTURES.items():
        inp = hr.make_inputs(case)
        N, C = inp["N"], inp["C"]

        def run(dtype, mask):
            head, params = build_train(VPRHead, inp, dtype, with_drop=p > 0)
            assert all(l.bn.momentum == br.MOMENTUM and l.bn.eps == hr.BN_EPS for l in (head.convlad1, head.convlad2, head.convlad3))
            rec = None
            if mask is None and p > 0:
                assert head.dropout.p == p
                rec = MaskRecorder(head.dropout)
                torch.manual_seed(seed)
            r = {k: v.numpy() for k, v in step(head, inp, dtype, hr.MARGIN, mask).items()}
            r["grads"] = [q.grad.numpy().copy() for q in params]
            return r, (rec.masks[0] if rec else mask)

        r64, mask = run(torch.float64, None)
        if mask is None:
            mask = np.ones((N, C), np.float32)
        r32, _ = run(torch.float32, mask)
        ours = br.step_gradients(inp["feat"], inp["params"], inp["stats"], inp["B"], inp["counts"], inp["slope"], mask)
        hinge32 = br.vr.triplet_loss(r32["vlad"], inp["B"], inp["counts"])[3]
        n32 = int((hinge32 > 0).sum())
        assert np.abs(ours["hinge"]).min() >= 1e-4, (fname, ours["hinge"])
        assert n32 == ours["n_active"], (fname, n32, ours["n_active"])
        active += ours["n_active"]
        inactive += len(ours["hinge"]) - ours["n_active"]
        data = {k: hr.stored(r64[k]) for k in hr.MAPS + ("vlad", "dvlad") + br.STATS}
        data.update({f"g{i}": hr.stored(g) for i, g in enumerate(r64["grads"])})
        data.update(loss=np.float64(r64["loss"]), n_active=np.int64(ours["n_active"]), margin=np.float64(hr.MARGIN), p=np.float64(p),
                    torch_seed=np.int64(seed), momentum=np.float64(br.MOMENTUM), mask=mask, max_stored=np.int64(hr.MAX_STORED),
                    err32_loss=np.float64(abs(float(r32["loss"]) - float(r64["loss"]))))
        for group, members in hr.GROUPS.items():
            data["err32_" + group] = np.float64(max(hr.rel_err(r32["grads"][i], r64["grads"][i]) for i in members))
        for k in hr.MAPS:
            data["err32_" + k] = np.float64(hr.rel_err(r32[k], r64[k]))
        for k in ("mean", "var", "rmean", "rvar"):
            data["err32_" + k] = np.float64(max(hr.rel_err(r32[f"{k}{i}"], r64[f"{k}{i}"]) for i in (1, 2, 3)))
        worst = max(hr.rel_err(np.asarray(a).reshape(b.shape), b) for a, b in zip(ours["grads"], r64["grads"]))
        worst = max([worst] + [hr.rel_err(ours[k], r64[k]) for k in hr.MAPS + br.STATS])
        if fname == br.TRAJECTORY:
            traj, drops = {}, None
            for dtype in (torch.float64, torch.float32):
                head, params = build_train(VPRHead, inp, dtype, with_drop=True)
                opt = torch.optim.Adam(params, lr=hr.LR)
                rec = MaskRecorder(head.dropout) if drops is None else None
                torch.manual_seed(seed)
                losses = []
                for t in range(hr.TRAJECTORY_STEPS):
                    opt.zero_grad()
                    losses.append(float(step(head, inp, dtype, hr.MARGIN, None if drops is None else drops[t])["loss"]))
                    opt.step()
                    if t + 1 == hr.PARAM_STEPS:
                        kept = [q.detach().numpy().copy() for q in params]
                        kept_stats = [(l.bn.running_mean.numpy().copy(), l.bn.running_var.numpy().copy())
                                      for l in (head.convlad1, head.convlad2, head.convlad3)]
                        tracked = [int(l.bn.num_batches_tracked) for l in (head.convlad1, head.convlad2, head.convlad3)]
                        assert tracked == [hr.PARAM_STEPS] * 3
                if drops is None:
                    drops = np.stack(rec.masks)
                    assert drops.shape == (hr.TRAJECTORY_STEPS, N, C) and np.array_equal(drops[0], mask)
                traj[dtype] = (np.asarray(losses, np.float64), kept, kept_stats)
            losses64, kept, kept_stats = traj[torch.float64]
            data.update(losses=losses64, lr=np.float64(hr.LR), masks=drops,
                        err32_losses=np.float64(np.abs(traj[torch.float32][0] - losses64).max()))
            data.update({f"p{i}_after": hr.stored(q) for i, q in enumerate(kept)})
            for i, (m, v) in enumerate(kept_stats, 1):
                data[f"rmean{i}_after"], data[f"rvar{i}_after"] = hr.stored(m), hr.stored(v)
            data["err32_rstats_after"] = np.float64(max(hr.rel_err(a, b) for s32, s64 in zip(traj[torch.float32][2], kept_stats)
                                                        for a, b in zip(s32, s64)))
        path = os.path.join(br.GOLDEN, f"{fname}.npz")
        np.savez_compressed(path, **data)
        print(f"{fname}.npz: {os.path.getsize(path)} B  loss {float(r64['loss'])!r}  active {ours['n_active']} of {sum(inp['counts'])}  "
              f"min|hinge| {np.abs(ours['hinge']).min():.2e}  dropped {int((mask == 0).sum())} of {mask.size}  oracle-vs-reference {worst:.1e}")
        print("  fp32 error: " + " ".join(f"{g} {float(data['err32_' + g]):.1e}" for g in br.QUANTITIES))
        if "losses" in data:
            print("  losses", " ".join(f"{v:.6f}" for v in data["losses"]), f" fp32-vs-fp64 {data['err32_losses']:.1e}",
                  f" running statistics after {hr.PARAM_STEPS} steps fp32-vs-fp64 {float(data['err32_rstats_after']):.1e}")
    assert active >= 1 and inactive >= 1, (active, inactive)
    print(f"triplets across the fixtures: {active} active, {inactive} inactive")


if __name__ == "__main__":
    main()
