"""The NetVLAD training step on the device (nano_vs_slam_amd.vlad_training, csrc/vlad_train.hip) against the float64
outputs of the reference's NetVLAD module under torch autograd, TripletMarginLoss and Adam (tests/golden/vlad_training/,
written by tools/make_vlad_training_golden.py; inputs regenerated from seeds by vlad_training_ref.make_inputs).
loss, dW and dcent are compared with the fixtures; of vlad and dvlad the fixtures keep every fourth column, so the numpy
float64 oracle, held to those columns to 1e-10, stands in for the whole arrays.

Error measure: for a gradient G, E(G) = max|G - G64| / max|G64|; for the loss |loss - loss64|.
Bound: 8 x the reference's own float32 error (the same module run in float32 on the CPU against its float64 run), the
maximum over the five cases per quantity, as stored in the fixtures:
    loss   8 x 6.6e-08 = 5.3e-07   (cases A..E: 2.0e-08, 1.2e-08, 6.6e-08, 4.2e-08, 1.3e-08), floor 16 ulp of the loss in fp32
    dW     8 x 1.4e-06 = 1.1e-05   (1.1e-06, 1.3e-06, 2.8e-07, 1.4e-06, 8.5e-07)
    dcent  8 x 1.7e-06 = 1.4e-05   (1.1e-06, 1.0e-06, 6.2e-07, 9.6e-07, 1.7e-06)
dvlad, for which the fixtures store no float32 error of its own, is held to the smaller gradient bound (dW's).  The factor
8 is for another summation order (tiles, then frames) and another exponential; a missing or wrong term gives E >= 1e-2.
The device results are chained as a training step chains them: the loss takes the device's vlad, the backward the
device's dvlad.  Every test prints the fraction of its bound it used.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import vlad_training_ref as vr
from conftest import product_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = 1e-5        # the project's fwd_vlad figure


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run_step(inp, x=None):
    """forward, loss, backward on the device as a training step chains them -> dict of device tensors."""
    from nano_vs_slam_amd import vlad_training as vt
    x = _dev(inp["x"]) if x is None else x
    W, cent = _dev(inp["W"]).view(inp["K"], inp["C"], 1, 1), _dev(inp["cent"])
    vlad, saved = vt.netvlad_forward(x, W, cent)
    loss, dvlad, n_active = vt.triplet_margin_loss(vlad, inp["B"], inp["counts"], vr.MARGIN)
    dW, dcent = vt.netvlad_backward(x, W, cent, saved, dvlad)
    return {"x": x, "W": W, "cent": cent, "vlad": vlad, "saved": saved, "loss": loss, "dvlad": dvlad, "n_active": n_active,
            "dW": dW, "dcent": dcent}


@pytest.fixture(scope="module")
def bounds():
    return vr.bounds()


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in vr.CASES:
        inp = vr.make_inputs(name)
        # loss, dW, dcent: the fixture's.  vlad and dvlad: the fixture keeps every fourth column, so the float64 oracle
        # stands in for the whole arrays, held to the fixture's columns here (and in test_vlad_training_cpu.py)
        ref = dict(vr.load_fixture(name))
        s = vr.step_gradients(inp["x"], inp["W"], inp["cent"], inp["B"], inp["counts"])
        st = int(ref["col_stride"])
        assert np.abs(s["vlad"][:, ::st] - ref["vlad_cols"]).max() <= 1e-10 and np.abs(s["dvlad"][:, ::st] - ref["dvlad_cols"]).max() <= 1e-10
        ref.update(vlad=s["vlad"], dvlad=s["dvlad"])
        out[name] = (inp, _run_step(inp), ref)
    torch.cuda.synchronize()
    return out


def _model_with(inp):
    """A config-S model (K = 64, C = 64) whose NetVLAD layer holds the case's parameters, in fp32 mode."""
    model, _ = product_model("S", False, 28, DEV)
    layer = model.vlad_head.netvlad
    with torch.no_grad():
        layer.conv.weight.copy_(_dev(inp["W"]).view(inp["K"], inp["C"], 1, 1))
        layer.centroids.copy_(_dev(inp["cent"]))
    return model.set_precision("fp32")


# ---- 1. forward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(vr.CASES))
def test_forward(runs, name):
    inp, r, fx = runs[name]
    err = np.abs(r["vlad"].cpu().numpy().astype(np.float64) - fx["vlad"]).max()
    print(f"case {name}: vlad max|diff| {err:.3e} = {err / FWD_TOL:.3f} of {FWD_TOL}")
    assert err <= FWD_TOL
    K, C = inp["K"], inp["C"]
    sv = r["saved"].cpu().numpy().astype(np.float64)
    fwd = vr.forward(inp["x"], inp["W"], inp["cent"])
    assert np.abs(sv[:, :K * C] - fwd["V"].reshape(inp["N"], -1)).max() <= 1e-4
    assert np.abs(sv[:, K * C:K * C + K] / fwd["n"] - 1).max() <= 1e-4 and np.abs(sv[:, K * C + K:K * C + 2 * K] - fwd["r"]).max() <= 1e-3
    assert np.abs(sv[:, K * C + 2 * K] / fwd["g"] - 1).max() <= 1e-5 and not sv[:, K * C + 2 * K + 1:].any()


def test_forward_equals_the_models_own_vlad():
    from nano_vs_slam_amd import vlad_training as vt
    from oracle.weights import synthetic_frames
    model, _ = product_model("S", False, 28, DEV)
    model.set_precision("fp32")
    H, W = 120, 160
    x = _dev(synthetic_frames(3, H, W, seed=21))
    with torch.no_grad():
        own = model.post_processing(model(x), H, W)["vlad"]
        layer = model.vlad_head.netvlad
        vlad, _ = vt.netvlad_forward(model.only_encoder(x), layer.conv.weight, layer.centroids)
    assert vlad.shape == own.shape == (3, 64 * 64)
    err = float((vlad - own).abs().max())
    print(f"netvlad_forward(only_encoder(x)) vs model vlad: max|diff| {err:.3e} = {err / FWD_TOL:.3f} of {FWD_TOL}")
    assert err <= FWD_TOL


# ---- 2. loss ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(vr.CASES))
def test_loss(runs, bounds, name):
    inp, r, fx = runs[name]
    loss64 = float(fx["loss"])
    lb = vr.loss_bound(loss64, bounds)
    err = abs(float(r["loss"]) - loss64)
    dv = r["dvlad"].cpu().numpy().astype(np.float64)
    abs_dv = np.abs(dv - fx["dvlad"]).max()
    e_dv = vr.rel_err(dv, fx["dvlad"])
    print(f"case {name}: loss err {err:.3e} = {err / lb:.3f} of {lb:.3e}; dvlad abs {abs_dv:.3e} = {abs_dv / lb:.3f} of the loss "
          f"bound, E {e_dv:.3e} = {e_dv / bounds['grad']:.3f} of {bounds['grad']:.3e}")
    assert err <= lb
    assert abs_dv <= lb and e_dv <= bounds["grad"]
    assert int(r["n_active"]) == int(fx["n_active"])
    B = inp["B"]
    for i, cnt in enumerate(inp["counts"]):
        if cnt == 0:                                    # a query without negatives: its q and p rows are exactly zero
            assert not r["dvlad"][i].any() and not r["dvlad"][B + i].any()
    hinge = vr.triplet_loss(fx["vlad"], B, inp["counts"])[3]
    for j, h in enumerate(hinge):                       # an inactive negative's row too
        assert bool(r["dvlad"][2 * B + j].any()) == bool(h > 0)


# ---- 3. backward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(vr.CASES))
def test_backward(runs, bounds, name):
    inp, r, fx = runs[name]
    assert r["dW"].shape == (inp["K"], inp["C"], 1, 1) and r["dcent"].shape == (inp["K"], inp["C"])
    for k in ("dW", "dcent"):
        e = vr.rel_err(r[k].cpu().numpy().reshape(inp["K"], inp["C"]), fx[k])
        print(f"case {name}: E({k}) {e:.3e} = {e / bounds[k]:.3f} of {bounds[k]:.3e}")
        assert e <= bounds[k]


# ---- 4. determinism and frame isolation -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_bit_reproducible_and_frames_isolated(runs, name):
    from nano_vs_slam_amd import vlad_training as vt
    inp, r, _ = runs[name]
    again = _run_step(inp)
    for k in ("vlad", "saved", "loss", "dvlad", "n_active", "dW", "dcent"):
        assert torch.equal(again[k], r[k]), k
    # three more frames behind the others whose dvlad rows are zero: no bit of dW or dcent changes, and the first frames'
    # vlad and saved rows do not change either
    x2 = torch.cat([r["x"], r["x"][[1, 0, 2]]])
    vlad2, saved2 = vt.netvlad_forward(x2, r["W"], r["cent"])
    N = inp["N"]
    assert torch.equal(vlad2[:N], r["vlad"]) and torch.equal(saved2[:N], r["saved"])
    dv2 = torch.cat([r["dvlad"], torch.zeros_like(r["dvlad"][:3])])
    dW2, dcent2 = vt.netvlad_backward(x2, r["W"], r["cent"], saved2, dv2)
    assert torch.equal(dW2, r["dW"]) and torch.equal(dcent2, r["dcent"])


# ---- 5. Adam ----------------------------------------------------------------------------------------------------------
def test_adam_step_against_torch():
    from nano_vs_slam_amd import vlad_training as vt
    rng = np.random.default_rng(7)
    n, lr = 4099, vr.LR
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32) for _ in range(3)]
    grads[1][::7] = 0.0
    ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([ref], lr=lr)
    p, m, v = _dev(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    worst = 0.0
    for t, g in enumerate(grads, 1):
        ref.grad = torch.from_numpy(g.copy())
        opt.step()
        version = p._version
        vt.adam_step(p, _dev(g), m, v, t, lr=lr)
        assert p._version > version
        want = ref.detach().numpy()
        tol = 4.0 * np.spacing(np.abs(want)) + 1e-6 * lr
        used = (np.abs(p.cpu().numpy() - want) / tol).max()
        worst = max(worst, float(used))
        assert used <= 1.0, (t, used)
    st = opt.state[ref]
    # the moments: three steps of a few fp32 operations each on terms no larger than max|g| (max g^2), which may cancel
    gmax = np.abs(np.stack(grads)).max(axis=0).astype(np.float64)
    assert (np.abs(m.cpu().numpy() - st["exp_avg"].numpy()) <= 1e-6 * gmax + 1e-30).all()
    assert (np.abs(v.cpu().numpy() - st["exp_avg_sq"].numpy()) <= 1e-6 * gmax * gmax + 1e-37).all()
    print(f"adam: {worst:.3f} of 4 ulp + 1e-6 lr")


# ---- 6. trainer -------------------------------------------------------------------------------------------------------
def test_trainer_follows_the_reference_trajectory(bounds):
    from nano_vs_slam_amd import vlad_training as vt
    inp = vr.make_inputs(vr.TRAJECTORY_CASE)
    fx = vr.load_fixture(vr.TRAJECTORY_CASE)
    model = _model_with(inp)
    trainer = vt.NetVLADTrainer(model, lr=vr.LR, margin=vr.MARGIN)
    enc = _dev(inp["x"]).view(inp["N"], inp["C"], 15, 20)
    losses, kept = [], None
    for t in range(vr.TRAJECTORY_STEPS):
        losses.append(trainer.step_encoded(enc, inp["B"], inp["counts"]))
        if t + 1 == vr.PARAM_STEPS:
            layer = model.vlad_head.netvlad
            kept = (layer.conv.weight.detach().clone(), layer.centroids.detach().clone())
    losses = np.asarray([float(l) for l in losses])
    used = [abs(l - l64) / vr.loss_bound(l64, bounds) for l, l64 in zip(losses, fx["losses"])]
    print("trainer losses", losses, "fractions of the loss bound", np.round(used, 3))
    assert max(used) <= 1.0
    assert (losses[1:] < losses[:-1]).all()
    _, _, _, grads = vr.trajectory(inp, steps=vr.PARAM_STEPS)
    mw, mc = vr.sign_driven(grads, bounds)
    tol = 1e-2 * vr.LR * vr.PARAM_STEPS
    for got, want, skip, what in ((kept[0], fx["W_after"], mw, "W"), (kept[1], fx["cent_after"], mc, "cent")):
        diff = np.abs(got.cpu().numpy().reshape(want.shape).astype(np.float64) - want)
        print(f"{what} after {vr.PARAM_STEPS} steps: max|diff| {diff[~skip].max():.3e} = {diff[~skip].max() / tol:.3f} of {tol:.1e}; "
              f"sign-driven elements {int(skip.sum())}")
        assert diff[~skip].max() <= tol and skip.mean() <= 0.01
        assert diff.max() <= 2.5 * vr.LR * vr.PARAM_STEPS          # even a flipped sign moves at most lr per step, either way


# ---- 7. the engine takes the new weights ------------------------------------------------------------------------------
def test_models_next_forward_uses_the_updated_layer():
    from nano_vs_slam_amd import vlad_training as vt
    from oracle.weights import synthetic_frames
    model, _ = product_model("S", False, 28, DEV)
    model.set_precision("fp32")
    H, W = 120, 160
    f = _dev(synthetic_frames(3, H, W, seed=31))
    query, positives = f[0:1], f[1:2]
    negatives = torch.stack([0.9 * f[0] + 0.1 * f[2], f[2]])
    x = torch.cat([query, positives, negatives])
    with torch.no_grad():
        before = model.post_processing(model(x), H, W)["vlad"].clone()
    trainer = vt.NetVLADTrainer(model, lr=1e-3, margin=vr.MARGIN)
    loss = trainer.step(query, positives, negatives, torch.tensor([2]))
    assert float(loss) > 0 and int(trainer.n_active) >= 1 and trainer.steps == 1
    with torch.no_grad():
        after = model.post_processing(model(x), H, W)["vlad"]
        layer = model.vlad_head.netvlad
        want, _ = vt.netvlad_forward(model.only_encoder(x), layer.conv.weight, layer.centroids)
    err, moved = float((after - want).abs().max()), float((after - before).abs().max())
    print(f"after one step: model vlad vs netvlad_forward(updated) {err:.3e} = {err / FWD_TOL:.3f} of {FWD_TOL}; moved {moved:.3e}")
    assert err <= FWD_TOL
    assert moved > FWD_TOL


# ---- 8. degenerate inputs ---------------------------------------------------------------------------------------------
def test_no_negatives_moves_nothing():
    from nano_vs_slam_amd import vlad_training as vt
    inp = vr.make_inputs("A")
    model = _model_with(inp)
    layer = model.vlad_head.netvlad
    w0, c0 = layer.conv.weight.detach().clone(), layer.centroids.detach().clone()
    trainer = vt.NetVLADTrainer(model)
    enc = _dev(inp["x"][:4]).view(4, inp["C"], 15, 20)
    loss = trainer.step_encoded(enc, 2, [0, 0])
    assert float(loss) == 0.0 and int(trainer.n_active) == 0 and trainer.steps == 1
    assert torch.equal(layer.conv.weight.detach(), w0) and torch.equal(layer.centroids.detach(), c0)
    vlad, _ = vt.netvlad_forward(enc, layer.conv.weight, layer.centroids)
    loss, dvlad, n_active = vt.triplet_margin_loss(vlad, 2, torch.zeros(2, dtype=torch.int64, device=DEV))
    assert float(loss) == 0.0 and int(n_active) == 0 and not dvlad.any()


def test_wrong_prefix_stays_inside_its_buffers(runs):
    """Offsets outside [0, n_neg] and out of order are clamped by the kernels: the result is unspecified, but nothing is
    written outside dvlad (guard rows on both sides keep their fill).  The offsets are wrong by one row at most and vlad,
    dvlad and the scratch carry a spare row on either side, so even an unclamped index would stay inside this test's own
    allocations: a regression fails the assertions below and touches nothing else."""
    from nano_vs_slam_amd import _lib
    inp, r, _ = runs["B"]
    lib = _lib.load()
    N, dim, B = inp["N"], inp["K"] * inp["C"], inp["B"]
    n_neg = N - 2 * B
    big = torch.full((N + 2, dim), 7.0, device=DEV)
    src = torch.zeros(N + 2, dim, device=DEV)
    src[1:N + 1] = r["vlad"]
    off = torch.tensor([-1, n_neg + 1, 2, n_neg + 1], dtype=torch.int32, device=DEV)
    out = torch.full((4,), 7.0, device=DEV)
    scratch = torch.empty(4 * (N + 8), dtype=torch.uint8, device=DEV)
    vp = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.kp2d_triplet_loss(vp(src[1:]), B, vp(off), n_neg, dim, vr.MARGIN, vp(out), vp(big[1:]), vp(out[1:]), vp(scratch),
                               scratch.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((big[0] == 7.0).all()) and bool((big[N + 1] == 7.0).all()) and bool((out[2:] == 7.0).all())
    assert bool(torch.isfinite(big[1:N + 1]).all())


def test_c_abi_refuses_before_launching():
    from nano_vs_slam_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    p, null = C.c_void_p(buf.data_ptr()), None
    assert lib.kp2d_vlad_train_scratch_bytes(4, 300, 64, 64) > 0
    for N, S, Cc, K in ((0, 300, 64, 64), (4, 0, 64, 64), (4, 300, 62, 64), (4, 300, 64, 68), (4, 300, 256, 64), (4, 300, 512, 16)):
        assert lib.kp2d_vlad_train_scratch_bytes(N, S, Cc, K) == 0
    assert lib.kp2d_vlad_forward_train(p, p, p, 4, 0, 64, 64, p, p, p, 1 << 18, null) == -1          # KP2D_ERR_ARG
    assert lib.kp2d_vlad_forward_train(p, p, p, 4, 300, 512, 16, p, p, p, 1 << 18, null) == -2       # KP2D_ERR_UNSUPPORTED
    assert lib.kp2d_vlad_forward_train(p, p, p, 1, 8, 16, 8, p, p, p, 16, null) == -1 and b"scratch" in lib.kp2d_last_error()
    assert lib.kp2d_vlad_backward(p, p, p, p, null, 1, 8, 16, 8, p, p, p, 1 << 18, null) == -1 and b"null" in lib.kp2d_last_error()
    assert lib.kp2d_triplet_loss(p, 1, p, 1, 128, -0.5, p, p, p, p, 1 << 18, null) == -1
    assert lib.kp2d_triplet_loss(p, 1, p, 1, 128, 0.1, p, p, p, p, 4, null) == -1 and b"scratch" in lib.kp2d_last_error()
    assert lib.kp2d_adam_step(p, p, p, p, 16, 0, 1e-4, 0.9, 0.999, 1e-8, null) == -1
    assert lib.kp2d_adam_step(p, p, p, p, 16, 1, 1e-4, 1.0, 0.999, 1e-8, null) == -1
    torch.cuda.synchronize()
    assert not buf.any()
