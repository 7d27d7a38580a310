"""The batch-hard triplet loss and the trainers' view step on the device (nano_vs_slam_amd.vlad_training.hard_triplet_loss,
NetVLADTrainer.step_views_encoded, VPRHeadTrainer.step_views_features; csrc/hard_triplet.hip) against the float64 outputs of
the reference's HardTripletLoss and VPRHead under torch autograd (tests/golden/hard_triplet/, written by
tools/make_hard_triplet_golden.py; inputs regenerated from seeds, the reference's dropout masks read from the fixtures).  The
fixtures keep a stated stride of every larger array, so the numpy float64 oracle (hard_triplet_ref), held to the stored
entries to 1e-10, stands in for the whole arrays.

Error measure: for an array G, E(G) = max|G - G64| / max|G64|; for a loss |loss - loss64|.
Bound, per tensor and fixture: max(8 x the reference's own float32 error of that tensor, 16 x 2^-24 of its largest magnitude),
the error being that of the same module run in float32 on the CPU against its float64 run.  stats, and the zeros of case G,
are exact.  The unpinned cases (an exact tie between two negatives, M = 1, weight = 0) are held to the oracle alone with
16 x 2^-24; the case past 256 rows, where a thread takes two columns, to the forward error bound of its fp32 sums (stated
there).  Every test prints the share of its bound it used; profiles/hard_triplet_fp64.txt holds the lines of one run on an
MI355X.

Not tested, because it does not hold: a pair's rows of case B run alone as M = 2 against the same negatives do not
reproduce their bits of the larger batch; the mean over the anchors couples the rows.
"""
import numpy as np
import pytest
import torch

import hard_triplet_ref as tr
from conftest import product_model

hr, br = tr.hr, tr.br
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAP_TOL = 2e-4        # what test_gpu_parity.py applies to fp32-mode taps (its TOL)
LOSS_FIXTURES = [(n, m) for n in tr.LOSS_CASES for m in tr.MODES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _margin(mode):
    return tr.QUIRK_MARGIN if mode == "hardest" else tr.BATCH_ALL_MARGIN


def _device_loss(emb, labels, margin, hardest, squared, weight=1.0):
    from nano_vs_slam_amd import vlad_training as vt
    return vt.hard_triplet_loss(_dev(emb), _dev(labels), margin, hardest, squared, weight)


@pytest.fixture(scope="module")
def loss_runs():
    out = {}
    for name, mode in LOSS_FIXTURES:
        emb, labels = tr.make_loss_inputs(name)
        squared = tr.LOSS_CASES[name][5]
        fx = tr.load_fixture(f"loss_{name}_{mode}")
        ref = tr.hard_triplet(emb, labels, _margin(mode), mode == "hardest", squared)
        assert abs(ref["loss"] - float(fx["loss"])) <= 1e-10 and np.abs(tr.stored(ref["demb"]) - fx["demb"]).max() <= 1e-10
        assert np.array_equal(ref["stats"], fx["stats"])
        out[name, mode] = (emb, labels, fx, ref, _device_loss(emb, labels, _margin(mode), mode == "hardest", squared))
    torch.cuda.synchronize()
    return out


# ---- 1. the loss against the fixtures ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", LOSS_FIXTURES)
def test_loss_gradient_and_stats(loss_runs, name, mode):
    emb, labels, fx, ref, (loss, demb, stats) = loss_runs[name, mode]
    assert loss.shape == () and loss.dtype == torch.float32 and demb.shape == emb.shape and stats.dtype == torch.int64
    lb = tr.loss_bound(fx, ref["loss"])
    le = abs(float(loss) - ref["loss"])
    assert stats.tolist() == ref["stats"].tolist()
    if not ref["demb"].any():
        print(f"hard_triplet share loss_{name}_{mode}: loss {le / lb if lb else 0.0:.3f} of {lb:.3e}; demb exactly zero")
        assert not demb.any() and le <= lb
        return
    gb = tr.bound(fx, "demb")
    ge = tr.rel_err(_np(demb), ref["demb"])
    print(f"hard_triplet share loss_{name}_{mode}: loss {le / lb:.3f} of {lb:.3e}; demb {ge / gb:.3f} of {gb:.3e}")
    assert le <= lb and ge <= gb


def test_case_G_is_exact(loss_runs):
    """No negatives: hardest gives margin (0.1 rounded to fp32 once) and plus and minus cancel in the integer coefficients;
    batch-all has no triplet at all."""
    _, _, _, _, (loss, demb, stats) = loss_runs["G", "hardest"]
    assert float(loss) == float(np.float32(0.1)) and not demb.any() and stats.tolist() == [2, 0, 2, 0]
    _, _, _, _, (loss, demb, stats) = loss_runs["G", "all"]
    assert float(loss) == 0.0 and not demb.any() and stats.tolist() == [0, 0, 2, 0]


def test_case_F_zero_distance_passes_no_gradient(loss_runs):
    for mode in tr.MODES:
        _, _, _, ref, (_, demb, stats) = loss_runs["F", mode]
        assert int(stats[3]) == 2 and torch.isfinite(demb).all()


@pytest.mark.parametrize("name,mode", LOSS_FIXTURES)
def test_bit_reproducible(loss_runs, name, mode):
    emb, labels, _, _, first = loss_runs[name, mode]
    again = _device_loss(emb, labels, _margin(mode), mode == "hardest", tr.LOSS_CASES[name][5])
    for a, b in zip(again, first):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["B", "C", "D", "H"])      # (E: ten of twelve anchors are active and reach every row)
def test_untouched_rows_are_exactly_zero(loss_runs, name):
    _, _, _, ref, (_, demb, _) = loss_runs[name, "hardest"]
    s = ref["w"] + ref["w"].T
    idle = ~s.any(axis=1)
    rows = demb.any(dim=1).cpu().numpy()
    print(f"{name}: {int(idle.sum())} of {idle.size} rows untouched by any active triplet")
    assert idle.any() and not idle.all()
    assert not rows[idle].any() and rows[~idle].all()


# ---- 2. unpinned cases, against the oracle alone -----------------------------------------------------------------------------------
def _against_oracle(emb, labels, margin, hardest, squared=False, weight=1.0, what=""):
    ref = tr.hard_triplet(emb, labels, margin, hardest, squared, weight)
    loss, demb, stats = _device_loss(emb, np.asarray(labels, np.int64), margin, hardest, squared, weight)
    assert stats.tolist() == ref["stats"].tolist()
    le = abs(float(loss) - ref["loss"])
    top = np.abs(ref["demb"]).max()
    ge = np.abs(_np(demb) - ref["demb"]).max()
    print(f"hard_triplet share {what}: loss {le / (tr.FLOOR * abs(ref['loss'])) if ref['loss'] else 0.0:.3f}, "
          f"demb {ge / (tr.FLOOR * top) if top else 0.0:.3f} of 16 x 2^-24")
    assert le <= tr.FLOOR * abs(ref["loss"]) and ge <= tr.FLOOR * top
    return ref, loss, demb


TIE = np.array([(1, 0, 0, 0), (-0.6, 0, 0, 0.8), (0, 1, 0, 0), (0, 0, 1, 0)], np.float32)


@pytest.mark.parametrize("hardest", [True, False])
def test_exact_tie_between_two_negatives(hardest):
    """Columns 2 and 3 are at exactly sqrt(2) from anchor 0: the lowest index wins, so in hardest mode anchor 0 pushes row 2
    and leaves row 3 to its own anchor's triplet."""
    ref, _, demb = _against_oracle(TIE, [0, 0, 1, 2], 1.0, hardest, what=f"tie hardest={hardest}")
    assert ref["d"][0, 2] == ref["d"][0, 3]
    if hardest:
        assert ref["picks"][0][1] == 2
        alone = tr.hard_triplet(TIE, [0, 0, 1, 2], 1.0)["w"]
        assert alone[0, 2] < 0 and alone[0, 3] == 0


@pytest.mark.parametrize("hardest", [True, False])
def test_one_row_and_zero_weight(hardest):
    ref, loss, demb = _against_oracle(np.ones((1, 5), np.float32), [7], 0.3, hardest, weight=2.0, what=f"M=1 hardest={hardest}")
    assert not demb.any() and (float(loss) == float(np.float32(0.6)) if hardest else float(loss) == 0.0)
    emb, labels = tr.make_loss_inputs("B")
    ref, loss, demb = _against_oracle(emb, labels, 0.1, hardest, weight=0.0, what=f"weight=0 hardest={hardest}")
    assert float(loss) == 0.0 and not demb.any() and ref["stats"][0] > 0


@pytest.mark.parametrize("hardest", [True, False])
def test_past_256_rows(hardest):
    """M = 300 with ten labelled pairs: a thread of the mining and gradient kernels takes two columns.  Bound of a gradient entry: its fp32 sum has
    n terms s_ij (x_ik - x_jk), each from a handful of roundings (the difference, s_ij = scale c / d_ij, the fma), so
    |error| <= (n + 8) 2^-24 sum_j |s_ij| |x_ik - x_jk| (the standard forward bound of a recursive sum) plus the same factor
    on the entry itself; the loss, a float64 sum rounded once from fp32 hinges of three roundings each, to 16 x 2^-24.
    Condition on the inputs, asserted: no hinge within 100 x its own float32 error of 0."""
    rng = np.random.default_rng(78)
    M, dim, P = 300, 20, 10
    common = tr._unit(rng.standard_normal(dim))
    emb = tr._unit(common + 0.5 * tr._unit(rng.standard_normal((M, dim))))
    emb[M - P:] = tr._unit(emb[:P] + 0.7 * (0.25 + 1.5 * rng.random((P, 1))) * tr._unit(rng.standard_normal((P, dim))))
    emb = emb.astype(np.float32)
    labels = np.arange(M)
    labels[M - P:] = labels[:P]                       # ten pairs; 280 anchors without a positive
    ref = tr.hard_triplet(emb, labels, 0.1, hardest)
    assert min(tr.hinge_gap(ref), tr.hardest_gaps(emb, labels)) >= 100 * tr.own_error(emb)
    loss, demb, stats = _device_loss(emb, labels, 0.1, hardest, False)
    assert stats.tolist() == ref["stats"].tolist() and 0 < ref["stats"][0] and ref["stats"][1] == M - 2 * P
    x = emb.astype(np.float64)
    s = ref["w"] + ref["w"].T
    s = np.where(ref["d"] > 0, s / np.where(ref["d"] > 0, ref["d"], 1.0), 0.0)
    mass = np.stack([(np.abs(s[i])[:, None] * np.abs(x[i][None, :] - x)).sum(axis=0) for i in range(M)])
    n = (s != 0).sum(axis=1)[:, None]
    tol = (n + 8) * 2.0 ** -24 * mass
    diff = np.abs(_np(demb) - ref["demb"])
    live = tol > 0
    le = abs(float(loss) - ref["loss"])
    print(f"hard_triplet share M=300 hardest={hardest}: loss {le / (tr.FLOOR * ref['loss']):.3f} of 16 x 2^-24; "
          f"demb {np.max(diff[live] / tol[live]):.3f} of its forward bound; up to {int(n.max())} terms per row")
    assert (diff <= tol).all() and le <= tr.FLOOR * ref["loss"]


# ---- 3. the trainers ------------------------------------------------------------------------------------------------------------------
def _model_with(inp):
    """A config-S model (64 -> 64, K = 64) whose vlad_head holds the case's parameters and statistics, in fp32 mode."""
    model, _ = product_model("S", False, 28, DEV)
    head = model.vlad_head
    with torch.no_grad():
        for i, layer in enumerate((head.convlad1, head.convlad2, head.convlad3)):
            layer.conv.weight.copy_(_dev(inp["params"][3 * i]))
            layer.bn.weight.copy_(_dev(inp["params"][3 * i + 1]))
            layer.bn.bias.copy_(_dev(inp["params"][3 * i + 2]))
            layer.bn.running_mean.copy_(_dev(inp["stats"][i][0]))
            layer.bn.running_var.copy_(_dev(inp["stats"][i][1]))
            assert layer.bn.eps == hr.BN_EPS and layer.bn.momentum == br.MOMENTUM
        head.netvlad.conv.weight.copy_(_dev(inp["params"][9]).view(inp["K"], inp["C"], 1, 1))
        head.netvlad.centroids.copy_(_dev(inp["params"][10]))
    return model.set_precision("fp32")


def _record_gradients(trainer):
    """-> a list that receives every step's gradients: the trainer's own _apply, watched."""
    seen, apply = [], trainer._apply

    def watched(params, grads):
        seen.append([g.detach().clone() for g in grads])
        return apply(params, grads)
    trainer._apply = watched
    return seen


def _check_parameters(kept, want, grads, bounds, names, steps, fixture):
    """The parameters after ``steps`` Adam steps, by the rule of test_gpu_vpr_head_training.py's trajectory test: an element
    whose oracle gradient at some step was below the gradient's bound may have moved the other way (Adam's first steps move
    by lr * sign(g)) and is held to 2.5 lr steps; every other element to 1e-2 lr steps."""
    tol = 1e-2 * tr.LR * steps
    for i, got in enumerate(kept):
        assert np.abs(tr.stored(want[i]) - fixture(i)).max() <= 1e-10
        skip = np.zeros(want[i].shape, bool)
        for g in grads:
            skip |= np.abs(g[i]) < bounds[i] * np.abs(g[i]).max()
        diff = np.abs(_np(got).reshape(want[i].shape) - want[i])
        print(f"{names[i]} after {steps} steps: max|diff| {diff[~skip].max():.3e} = {diff[~skip].max() / tol:.3f} of {tol:.1e}; "
              f"sign-driven elements {int(skip.sum())} of {skip.size}")
        assert diff[~skip].max() <= tol, names[i]
        assert diff.max() <= 2.5 * tr.LR * steps, names[i]


@pytest.mark.parametrize("case", list(tr.TRAINER_CASES))
@pytest.mark.parametrize("batch", [False, True])
def test_head_trainer_follows_the_reference(case, batch):
    """step_views_features: the first step's loss, eleven gradients and stats, the losses of every step, the parameters after
    the last one, and in batch mode (each step under the two masks the reference's Dropout2d drew for its two calls) the
    running statistics after the first and after the last step and num_batches_tracked + 2 per step."""
    from nano_vs_slam_amd import vpr_head_training as ht
    kind = "batch" if batch else "running"
    fx = tr.load_fixture(f"head_{case}_{kind}")
    inp = tr.make_trainer_inputs(case)
    steps = tr.BATCH_STEPS if batch else tr.RUNNING_STEPS
    drops = [tuple(m) for m in fx["masks"]] if batch else None
    model = _model_with(inp)
    trainer = ht.VPRHeadTrainer(model, lr=tr.LR, bn=kind, dropout=tr.P_DROP) if batch else ht.VPRHeadTrainer(model, lr=tr.LR)
    seen = _record_gradients(trainer)
    feat, feat_aug = _dev(inp["feat"]), _dev(inp["feat_aug"])
    tracked0 = [int(l.bn.num_batches_tracked) for l in trainer.layers]
    stats0 = [(l.bn.running_mean.clone(), l.bn.running_var.clone()) for l in trainer.layers]
    losses, first_stats, first_rstats = [], None, None
    for t in range(steps):
        versions = [p._version for p in trainer.parameters()]
        drop = None if drops is None else tuple(_dev(m) for m in drops[t])
        losses.append(float(trainer.step_views_features(feat, feat_aug, drop=drop)))
        assert all(p._version > v for p, v in zip(trainer.parameters(), versions)) and trainer.steps == t + 1
        if t == 0:
            first_stats = trainer.ht_stats.tolist()
            first_rstats = [(l.bn.running_mean.clone(), l.bn.running_var.clone()) for l in trainer.layers]
    ref = tr.head_views_gradients(inp["feat"], inp["feat_aug"], inp["params"], inp["stats"], inp["slope"], batch, drops[0] if batch else None)
    assert abs(ref["loss"] - float(fx["loss"])) <= 1e-10 and first_stats == ref["stats"].tolist() == fx["stats"].tolist()
    lb = tr.loss_bound(fx, ref["loss"])
    shares = {"loss": abs(losses[0] - ref["loss"]) / lb}
    assert len(seen) == steps and len(seen[0]) == 11
    for i, want in enumerate(ref["grads"]):
        want = np.asarray(want)
        assert np.abs(tr.stored(want) - fx[f"g{i}"]).max() <= 1e-10
        assert seen[0][i].numel() == want.size
        shares[hr.PARAMS[i]] = tr.rel_err(_np(seen[0][i]).reshape(want.shape), want) / tr.bound(fx, f"g{i}")
    tb = [max(8.0 * float(fx["err32_losses"]), tr.FLOOR * abs(l)) for l in fx["losses"]]
    shares["losses"] = max(abs(a - b) / c for a, b, c in zip(losses, fx["losses"], tb))
    want_losses, want, want_stats, grads = tr.head_views_trajectory(inp, steps, batch, drops)
    assert np.abs(want_losses - fx["losses"]).max() <= 1e-10
    if batch:
        assert [int(l.bn.num_batches_tracked) for l in trainer.layers] == [n + 2 * steps for n in tracked0]
        for key, got, ref_stats in (("rstats", first_rstats, ref["rstats"]), ("rstats_after", [(l.bn.running_mean, l.bn.running_var) for l in trainer.layers], want_stats)):
            sb = tr.bound(fx, key)
            for i, ((m, v), (m64, v64)) in enumerate(zip(got, ref_stats), 1):
                assert np.abs(m64 - fx[f"{key}_mean{i}"]).max() <= 1e-10 and np.abs(v64 - fx[f"{key}_var{i}"]).max() <= 1e-10
                shares[f"{key}{i}"] = max(tr.rel_err(_np(m), m64), tr.rel_err(_np(v), v64)) / sb
    else:
        assert [int(l.bn.num_batches_tracked) for l in trainer.layers] == tracked0
        for l, (m0, v0) in zip(trainer.layers, stats0):
            assert torch.equal(l.bn.running_mean, m0) and torch.equal(l.bn.running_var, v0)
    worst = max(shares, key=shares.get)
    print(f"hard_triplet share head_{case}_{kind}: largest {shares[worst]:.3f} ({worst}); " + " ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert shares[worst] <= 1.0, worst
    _check_parameters([p.detach() for p in trainer.parameters()], want, grads, [tr.bound(fx, f"g{i}") for i in range(11)], hr.PARAMS, steps,
                      lambda i: fx[f"p{i}_after"])


@pytest.mark.parametrize("case", list(tr.TRAINER_CASES))
def test_netvlad_trainer_follows_the_reference(case):
    from nano_vs_slam_amd import vlad_training as vt
    fx = tr.load_fixture(f"netvlad_{case}")
    inp = tr.make_trainer_inputs(case)
    K, Cc = inp["K"], inp["C"]
    trainer = vt.NetVLADTrainer(_model_with(inp), lr=tr.LR)
    seen = _record_gradients(trainer)
    enc, enc_aug = _dev(inp["enc"]), _dev(inp["enc_aug"])
    losses, first_stats = [], None
    for t in range(tr.RUNNING_STEPS):
        losses.append(float(trainer.step_views_encoded(enc, enc_aug)))
        first_stats = trainer.ht_stats.tolist() if t == 0 else first_stats
    ref = tr.netvlad_views_gradients(inp["enc"], inp["enc_aug"], inp["params"][9].reshape(K, Cc), inp["params"][10])
    assert abs(ref["loss"] - float(fx["loss"])) <= 1e-10 and first_stats == ref["stats"].tolist() == fx["stats"].tolist()
    shares = {"loss": abs(losses[0] - ref["loss"]) / tr.loss_bound(fx, ref["loss"])}
    for i, k in enumerate(("dW", "dcent")):
        assert np.abs(tr.stored(ref[k]) - fx[k]).max() <= 1e-10
        shares[k] = tr.rel_err(_np(seen[0][i]).reshape(ref[k].shape), ref[k]) / tr.bound(fx, k)
    tb = [max(8.0 * float(fx["err32_losses"]), tr.FLOOR * abs(l)) for l in fx["losses"]]
    shares["losses"] = max(abs(a - b) / c for a, b, c in zip(losses, fx["losses"], tb))
    worst = max(shares, key=shares.get)
    print(f"hard_triplet share netvlad_{case}: largest {shares[worst]:.3f} ({worst}); " + " ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert shares[worst] <= 1.0, worst
    want_losses, W, cent, grads = tr.netvlad_views_trajectory(inp, tr.RUNNING_STEPS)
    assert np.abs(want_losses - fx["losses"]).max() <= 1e-10
    layer = trainer.layer
    _check_parameters([layer.conv.weight.detach(), layer.centroids.detach()], [W, cent], grads, [tr.bound(fx, "dW"), tr.bound(fx, "dcent")],
                      ("netvlad.conv.weight", "netvlad.centroids"), tr.RUNNING_STEPS, lambda i: fx[("W_after", "cent_after")[i]])


def test_view_steps_are_bit_reproducible_and_draw_a_mask_per_view():
    """Two trainers on equal models take the same steps bit for bit; without injected masks the batch-mode step draws
    dropout2d_scale(..., layer 1) for the plain view and layer 2 for the augmented view at its own step number."""
    from nano_vs_slam_amd import vpr_head_training as ht
    inp = tr.make_trainer_inputs("S6x8")
    feat, feat_aug = _dev(inp["feat"]), _dev(inp["feat_aug"])
    N, Cc = tr.PAIRS, inp["C"]
    out = []
    for injected in (False, True, False):
        trainer = ht.VPRHeadTrainer(_model_with(inp), lr=tr.LR, bn="batch", dropout=0.2, seed=9)
        losses = []
        for step in (1, 2):
            drop = tuple(ht.dropout2d_scale(N, Cc, 0.2, 9, step, layer, DEV) for layer in (1, 2)) if injected else None
            losses.append(trainer.step_views_features(feat, feat_aug, drop=drop))
        out.append((losses, [p.detach().clone() for p in trainer.parameters()], trainer.ht_stats.clone()))
    for other in out[1:]:
        assert all(torch.equal(a, b) for a, b in zip(out[0][0], other[0])) and torch.equal(out[0][2], other[2])
        assert all(torch.equal(a, b) for a, b in zip(out[0][1], other[1]))
    same = ht.dropout2d_scale(N, Cc, 0.2, 9, 1, 1, DEV)
    swapped = ht.VPRHeadTrainer(_model_with(inp), lr=tr.LR, bn="batch", dropout=0.2, seed=9).step_views_features(feat, feat_aug, drop=(same, same))
    assert not torch.equal(swapped, out[0][0][0])
    # on running statistics the two views are one batch of 2 N: the step's loss and stats have the bits of the head's own calls
    # chained by hand on the concatenation
    from nano_vs_slam_amd import vlad_training as vt
    model = _model_with(inp)
    trainer = ht.VPRHeadTrainer(model, lr=tr.LR)
    y3 = trainer.forward_features(torch.cat([feat, feat_aug]))[-1][1]
    netvlad = model.vlad_head.netvlad
    vlad = vt.netvlad_forward(y3, netvlad.conv.weight, netvlad.centroids)[0]
    want, _, want_stats = vt.hard_triplet_loss(vlad, vt.view_labels(N, DEV), 0.1, True)
    got = trainer.step_views_features(feat, feat_aug)
    assert torch.equal(got, want) and torch.equal(trainer.ht_stats, want_stats) and float(want) > 0


def test_engine_follows_three_view_steps():
    """After three step_views over frames the engine's vlad output agrees with the training forward on the updated
    parameters within the 2e-4 contract of fp32-mode taps: the engine re-packed through the version bumps."""
    from nano_vs_slam_amd import vlad_training as vt, vpr_head_training as ht
    from oracle.weights import synthetic_frames
    model, _ = product_model("S", False, 28, DEV)
    model.set_precision("fp32")
    H, W = 64, 96
    f = _dev(synthetic_frames(6, H, W, seed=41))
    frames = f[:3]
    frames_aug = torch.stack([0.7 * f[0] + 0.3 * f[3], 0.5 * f[1] + 0.5 * f[4], f[5]])
    x = torch.cat([frames, frames_aug])
    trainer = ht.VPRHeadTrainer(model, lr=1e-3)
    frozen = ht.VPRHeadTrainer(model)

    def both():
        with torch.no_grad():
            own = model(x)["vlad"].clone()
            y3 = frozen.forward_features(model.backbone_features(x))[-1][1]
            netvlad = model.vlad_head.netvlad
            return own, vt.netvlad_forward(y3, netvlad.conv.weight, netvlad.centroids)[0]

    own0, mine0 = both()
    losses = [float(trainer.step_views(frames, frames_aug)) for _ in range(3)]
    own1, mine1 = both()
    err0, err1, moved = float((own0 - mine0).abs().max()), float((own1 - mine1).abs().max()), float((own1 - own0).abs().max())
    print(f"engine vlad vs training forward: before {err0:.3e}, after three view steps {err1:.3e} of {TAP_TOL}; the steps moved vlad by {moved:.3e}; "
          f"losses {losses}; stats {trainer.ht_stats.tolist()}")
    assert trainer.steps == 3 and losses[0] > 0 and (losses[2] > 0) == (int(trainer.ht_stats[0]) > 0)
    assert err0 <= TAP_TOL and err1 <= TAP_TOL
    assert moved > err1
    # NetVLADTrainer.step_views is step_views_encoded on only_encoder of the same frames: the loss, formed by hand first
    layer = vt.NetVLADTrainer(model, lr=1e-3)
    with torch.no_grad():
        enc = model.only_encoder(x).clone()
    netvlad = model.vlad_head.netvlad
    want, _, want_stats = vt.hard_triplet_loss(vt.netvlad_forward(enc, netvlad.conv.weight, netvlad.centroids)[0], vt.view_labels(3, DEV), 0.1, True)
    got = layer.step_views(frames, frames_aug)
    assert torch.equal(got, want) and torch.equal(layer.ht_stats, want_stats) and float(want) > 0 and layer.steps == 1
    own2, mine2 = both()
    assert float((own2 - mine2).abs().max()) <= TAP_TOL
