"""The head training step on the device (nano_vs_slam_amd.vpr_head_training, csrc/vpr_head_train.hip, csrc/vlad_train.hip)
against the float64 outputs of the reference's VPRHead in .eval() under torch autograd, TripletMarginLoss and Adam
(tests/golden/vpr_head_training/, written by tools/make_vpr_head_training_golden.py; inputs regenerated from seeds by
vpr_head_training_ref.make_inputs).  The fixtures keep a stated stride of every larger array, so the numpy float64 oracle,
held to the stored entries to 1e-10, stands in for the whole arrays.

Error measure: for an array G, E(G) = max|G - G64| / max|G64|; for the loss |loss - loss64|.
Bound: 8 x the reference's own float32 error of that quantity (the same module run in float32 on the CPU against its
float64 run), the maximum over the five cases, per gradient group (conv weights, BatchNorm vectors, NetVLAD weight,
centroids) and per map (each layer's y, the three dx), read from the fixtures (vpr_head_training_ref.bounds); the loss has a
floor of 16 ulp in fp32.  The factor 8 is for another summation order (tiles, slabs, frames) and another exponential; a
missing or wrong term gives E >= 1e-2.  The device results are chained as a training step chains them: every layer takes
the device's output of the one before it, the backward the device's dy.  Every test prints the fraction of its bound it used.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import vpr_head_training_ref as hr
from conftest import product_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAP_TOL = 2e-4        # what test_gpu_parity.py applies to fp32-mode taps (its TOL)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _vectors(inp, i, params=None):
    """(scale, shift, mean, invstd) of layer i as device tensors, formed with torch on the device (float32)."""
    params = inp["params"] if params is None else params
    gamma, beta = _dev(params[3 * i + 1]), _dev(params[3 * i + 2])
    mean, var = _dev(inp["stats"][i][0]), _dev(inp["stats"][i][1])
    invstd = 1.0 / torch.sqrt(var + hr.BN_EPS)
    scale = gamma * invstd
    return scale, beta - mean * scale, mean, invstd


def _run_step(inp, feat=None, need_dx1=False):
    """forward, loss, backward on the device as a training step chains them -> dict of device tensors."""
    from nano_vs_slam_amd import vlad_training as vt, vpr_head_training as ht
    K, Cc = inp["K"], inp["C"]
    x = _dev(inp["feat"]) if feat is None else feat
    r = {"feat": x}
    acts = []
    for i in range(3):
        vec = _vectors(inp, i)
        w = _dev(inp["params"][3 * i])
        y, c = ht.cbr_forward(x, w, vec[0], vec[1], inp["slope"])
        acts.append((x, w, vec, y, c))
        r[f"y{i + 1}"] = y
        x = y
    W, cent = _dev(inp["params"][9]).view(K, Cc, 1, 1), _dev(inp["params"][10])
    vlad, saved = vt.netvlad_forward(x, W, cent)
    loss, dvlad, n_active = vt.triplet_margin_loss(vlad, inp["B"], inp["counts"], hr.MARGIN)
    dW, dcent = vt.netvlad_backward(x, W, cent, saved, dvlad)
    dy = ht.netvlad_backward_input(x, W, cent, saved, dvlad)
    r.update(vlad=vlad, saved=saved, loss=loss, dvlad=dvlad, n_active=n_active, dx_netvlad=dy, acts=acts)
    grads = [None] * 9 + [dW, dcent]
    for i in (2, 1, 0):
        lx, w, (scale, _, mean, invstd), y, c = acts[i]
        r[f"dy{i + 1}"] = dy
        dw, dgamma, dbeta, dy = ht.cbr_backward(lx, w, scale, mean, invstd, y, c, dy, inp["slope"], need_dx=i > 0 or need_dx1)
        grads[3 * i:3 * i + 3] = [dw, dgamma, dbeta]
        if dy is not None:
            r[f"dx{i + 1}"] = dy
    r["grads"] = grads
    return r


@pytest.fixture(scope="module")
def bounds():
    return hr.bounds()


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in hr.CASES:
        inp = hr.make_inputs(name)
        fx = hr.load_fixture(name)
        ref = hr.step_gradients(inp["feat"], inp["params"], inp["stats"], inp["B"], inp["counts"], inp["slope"])
        for k in hr.MAPS + ("vlad", "dvlad"):           # the oracle stands in for the whole arrays: held to the fixture here
            assert np.abs(hr.stored(ref[k]) - fx[k]).max() <= 1e-10, k
        for i, g in enumerate(ref["grads"]):
            assert np.abs(hr.stored(g) - fx[f"g{i}"]).max() <= 1e-10, hr.PARAMS[i]
        assert abs(ref["loss"] - float(fx["loss"])) <= 1e-10 and ref["n_active"] == int(fx["n_active"])
        out[name] = (inp, _run_step(inp), ref)
    torch.cuda.synchronize()
    return out


def _np(t):
    return t.cpu().numpy().astype(np.float64)


# ---- 1. the chained step against the fixtures ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hr.CASES))
def test_forward_maps(runs, bounds, name):
    inp, r, ref = runs[name]
    for k in ("y1", "y2", "y3"):
        assert r[k].shape == ref[k].shape
        e = hr.rel_err(_np(r[k]), ref[k])
        print(f"case {name}: E({k}) {e:.3e} = {e / bounds[k]:.3f} of {bounds[k]:.3e}")
        assert e <= bounds[k]


@pytest.mark.parametrize("name", list(hr.CASES))
def test_loss_and_active_count(runs, bounds, name):
    inp, r, ref = runs[name]
    lb = hr.loss_bound(ref["loss"], bounds)
    err = abs(float(r["loss"]) - ref["loss"])
    print(f"case {name}: loss err {err:.3e} = {err / lb:.3f} of {lb:.3e}; n_active {int(r['n_active'])}")
    assert err <= lb
    assert int(r["n_active"]) == ref["n_active"]


@pytest.mark.parametrize("name", list(hr.CASES))
def test_gradients(runs, bounds, name):
    inp, r, ref = runs[name]
    for group, members in hr.GROUPS.items():
        for i in members:
            want = np.asarray(ref["grads"][i])
            got = _np(r["grads"][i]).reshape(want.shape)
            assert r["grads"][i].numel() == inp["params"][i].size
            e = hr.rel_err(got, want)
            print(f"case {name}: E(d {hr.PARAMS[i]}) {e:.3e} = {e / bounds[group]:.3f} of {bounds[group]:.3e}")
            assert e <= bounds[group], hr.PARAMS[i]


@pytest.mark.parametrize("name", list(hr.CASES))
def test_input_gradients(runs, bounds, name):
    inp, r, ref = runs[name]
    assert "dx1" not in r                                # the backbone is frozen: convlad1 forms no dx
    for k in ("dx_netvlad", "dx3", "dx2"):
        assert r[k].shape == ref[k].shape
        e = hr.rel_err(_np(r[k]), ref[k])
        print(f"case {name}: E({k}) {e:.3e} = {e / bounds[k]:.3f} of {bounds[k]:.3e}")
        assert e <= bounds[k]


# ---- 2. determinism, frame isolation, gamma = 0, dx = NULL ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(hr.CASES))
def test_bit_reproducible(runs, name):
    inp, r, _ = runs[name]
    again = _run_step(inp)
    for k in ("y1", "y2", "y3", "vlad", "loss", "dvlad", "n_active", "dx_netvlad", "dx3", "dx2"):
        assert torch.equal(again[k], r[k]), k
    for i, (a, b) in enumerate(zip(again["grads"], r["grads"])):
        assert torch.equal(a, b), hr.PARAMS[i]


def test_frames_with_zero_dy_change_no_bit(runs):
    """Case B: query 1 has no negatives, so its frame and its positive's have exactly zero dvlad rows and zero dy in every
    layer.  Other data in those two frames changes no bit of any gradient."""
    inp, r, _ = runs["B"]
    B = inp["B"]
    rows = [1, B + 1]
    for k in ("dvlad", "dx_netvlad", "dx3", "dx2"):
        assert not r[k][rows].any(), k
    feat = r["feat"].clone()
    feat[rows] = torch.flip(r["feat"][[0, B]], dims=(1, 3)) * 1.5 + 0.25
    other = _run_step(inp, feat)
    assert not torch.equal(other["y3"][rows], r["y3"][rows])
    assert torch.equal(other["loss"], r["loss"]) and torch.equal(other["n_active"], r["n_active"])
    for i, (a, b) in enumerate(zip(other["grads"], r["grads"])):
        assert torch.equal(a, b), hr.PARAMS[i]
    keep = [i for i in range(inp["N"]) if i not in rows]
    for k in ("dx_netvlad", "dx3", "dx2"):
        assert torch.equal(other[k][keep], r[k][keep]) and not other[k][rows].any(), k


def test_gamma_zero_channels(runs, bounds):
    """Case E: one channel per layer has gamma = 0 (scale 0, y constant): its dgamma comes from c itself and is held to
    the BatchNorm bound like every other entry; its dc, and with it its rows of dw, are exactly zero."""
    inp, r, ref = runs["E"]
    for i in range(3):
        ch = int(np.flatnonzero(inp["params"][3 * i + 1] == 0)[0])
        want = ref["grads"][3 * i + 1]
        got = _np(r["grads"][3 * i + 1])
        assert want[ch] != 0
        e = abs(got[ch] - want[ch]) / np.abs(want).max()
        print(f"layer {i + 1} channel {ch}: dgamma {got[ch]:.6e} vs {want[ch]:.6e}, {e / bounds['bn']:.3f} of {bounds['bn']:.3e}")
        assert e <= bounds["bn"]
        assert not r["grads"][3 * i][ch].any()


@pytest.mark.parametrize("name", ["B", "C"])
def test_backward_without_dx_has_the_same_bits(runs, name):
    from nano_vs_slam_amd import vpr_head_training as ht
    inp, r, _ = runs[name]
    for i in range(3):
        lx, w, (scale, _, mean, invstd), y, c = r["acts"][i]
        dy = r[f"dy{i + 1}"]
        with_dx = ht.cbr_backward(lx, w, scale, mean, invstd, y, c, dy, inp["slope"], need_dx=True)
        without = ht.cbr_backward(lx, w, scale, mean, invstd, y, c, dy, inp["slope"], need_dx=False)
        assert without[3] is None and with_dx[3].shape == lx.shape
        for a, b, g in zip(with_dx[:3], without[:3], r["grads"][3 * i:3 * i + 3]):
            assert torch.equal(a, b) and torch.equal(a, g)
        if i > 0:
            assert torch.equal(with_dx[3], r[f"dx{i + 1}"])


def test_netvlad_input_gradient_with_more_clusters_than_channels(bounds):
    """K > C: the tile keeps `a` in LDS of its own (for K <= C, every case above, it sits in the rows of xh).  One ragged
    tile and a full one, against the float64 oracle, held to the bound of the NetVLAD input gradient."""
    from nano_vs_slam_amd import vlad_training as vt, vpr_head_training as ht
    rng = np.random.default_rng(17)
    N, C, K, S = 3, 16, 32, 70
    x = rng.standard_normal((N, C, S)).astype(np.float32)
    W = (3.0 * rng.standard_normal((K, C))).astype(np.float32)
    cent = (0.3 * rng.standard_normal((K, C))).astype(np.float32)
    dv = rng.standard_normal((N, K * C)).astype(np.float32)
    fwd = hr.vr.forward(x, W, cent)
    _, _, dU = hr.vr.backward(fwd, cent, dv)
    want = hr.netvlad_dx(fwd, x, W, cent, dU)
    xd, Wd, cd = _dev(x), _dev(W).view(K, C, 1, 1), _dev(cent)
    vlad, saved = vt.netvlad_forward(xd, Wd, cd)
    got = ht.netvlad_backward_input(xd, Wd, cd, saved, _dev(dv))
    assert torch.equal(got, ht.netvlad_backward_input(xd, Wd, cd, saved, _dev(dv)))
    e = hr.rel_err(_np(got), want)
    print(f"K {K} > C {C}: E(dx_netvlad) {e:.3e} = {e / bounds['dx_netvlad']:.3f} of {bounds['dx_netvlad']:.3e}")
    assert e <= bounds["dx_netvlad"]


# ---- 3. the trainer ---------------------------------------------------------------------------------------------------------
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
            assert layer.bn.eps == hr.BN_EPS
        head.netvlad.conv.weight.copy_(_dev(inp["params"][9]).view(inp["K"], inp["C"], 1, 1))
        head.netvlad.centroids.copy_(_dev(inp["params"][10]))
    return model.set_precision("fp32")


def test_trainer_follows_the_reference_trajectory(bounds):
    from nano_vs_slam_amd import vpr_head_training as ht
    inp = hr.make_inputs(hr.TRAJECTORY_CASE)
    fx = hr.load_fixture(hr.TRAJECTORY_CASE)
    model = _model_with(inp)
    trainer = ht.VPRHeadTrainer(model, lr=hr.LR, margin=hr.MARGIN)
    feat = _dev(inp["feat"])
    stats0 = [(l.bn.running_mean.clone(), l.bn.running_var.clone()) for l in trainer.layers]
    losses, kept = [], None
    for t in range(hr.TRAJECTORY_STEPS):
        versions = [p._version for p in trainer.parameters()]
        losses.append(trainer.step_features(feat, inp["B"], inp["counts"]))
        assert all(p._version > v for p, v in zip(trainer.parameters(), versions))
        if t + 1 == hr.PARAM_STEPS:
            kept = [p.detach().clone() for p in trainer.parameters()]
    losses = np.asarray([float(l) for l in losses])
    used = [abs(l - l64) / hr.loss_bound(l64, bounds) for l, l64 in zip(losses, fx["losses"])]
    print("trainer losses", losses, "fractions of the loss bound", np.round(used, 3))
    assert max(used) <= 1.0
    assert (losses[1:] < losses[:-1]).all()
    for l, (m0, v0) in zip(trainer.layers, stats0):      # the running statistics are not updated
        assert torch.equal(l.bn.running_mean, m0) and torch.equal(l.bn.running_var, v0)
    # parameters after three steps.  Adam's first steps move every element by about lr * sign(g): an element whose oracle
    # gradient at one of those steps was below the gradient bound may have the other sign on the device and is exempt from
    # the tight comparison; even a flipped sign moves at most lr per step, either way.  How many elements that is depends on
    # the float64 oracle alone (the share of a parameter's gradient entries below 5e-5 of its largest: 0 to 14 % here, most
    # for convlad3's weights, whose gradient is concentrated in few entries), so it is printed and not bounded.
    _, want, grads = hr.trajectory(inp, steps=hr.PARAM_STEPS)
    group_of = {i: g for g, members in hr.GROUPS.items() for i in members}
    tol = 1e-2 * hr.LR * hr.PARAM_STEPS
    for i, got in enumerate(kept):
        assert np.abs(hr.stored(want[i]) - fx[f"p{i}_after"]).max() <= 1e-10
        skip = np.zeros(want[i].shape, bool)
        for g in grads:
            skip |= np.abs(g[i]) < bounds[group_of[i]] * np.abs(g[i]).max()
        diff = np.abs(_np(got).reshape(want[i].shape) - want[i])
        print(f"{hr.PARAMS[i]} after {hr.PARAM_STEPS} steps: max|diff| {diff[~skip].max():.3e} = {diff[~skip].max() / tol:.3f} of {tol:.1e}; "
              f"sign-driven elements {int(skip.sum())} of {skip.size}")
        assert diff[~skip].max() <= tol, hr.PARAMS[i]
        assert diff.max() <= 2.5 * hr.LR * hr.PARAM_STEPS, hr.PARAMS[i]


def test_engine_repacks_conv_and_batchnorm_after_a_step():
    """The training forward's L2-normalised y3 against the engine's own only_encoder in fp32 mode on one model, before and
    after a step over frames: after it the engine has re-packed the updated conv weights with BatchNorm re-folded, and the
    map has moved."""
    from nano_vs_slam_amd import vpr_head_training as ht
    from oracle.weights import synthetic_frames
    model, _ = product_model("S", False, 28, DEV)
    model.set_precision("fp32")
    H, W = 64, 96
    f = _dev(synthetic_frames(3, H, W, seed=31))
    query, positives = f[0:1], f[1:2]
    negatives = torch.stack([0.9 * f[0] + 0.1 * f[2], f[2]])
    x = torch.cat([query, positives, negatives])
    trainer = ht.VPRHeadTrainer(model, lr=1e-3, margin=hr.MARGIN)

    def both():
        with torch.no_grad():
            own = model.only_encoder(x).clone()
            feat = model.backbone_features(x)
            _, tap = model.forward_with_tap(x, "backbone.conv4b", feat.shape[1:])
            assert torch.isfinite(feat).all() and torch.equal(feat, tap)      # the tap passes an only-encoder forward
            y3 = trainer.forward_features(feat)[-1][1]
            return own, torch.nn.functional.normalize(y3, p=2.0, dim=1)

    own0, mine0 = both()
    err0 = float((own0 - mine0).abs().max())
    loss = trainer.step(query, positives, negatives, torch.tensor([2]))
    assert float(loss) > 0 and int(trainer.n_active) >= 1 and trainer.steps == 1
    own1, mine1 = both()
    err1, moved = float((own1 - mine1).abs().max()), float((own1 - own0).abs().max())
    print(f"training forward vs only_encoder: before {err0:.3e} = {err0 / TAP_TOL:.3f}, after {err1:.3e} = {err1 / TAP_TOL:.3f} of {TAP_TOL}; "
          f"moved {moved:.3e}")
    assert err0 <= TAP_TOL and err1 <= TAP_TOL
    assert moved > TAP_TOL


def test_netvlad_trainer_still_works_on_the_same_model():
    """NetVLADTrainer after a VPRHeadTrainer step on one model: both step, both bump versions, the engine follows."""
    from nano_vs_slam_amd import vlad_training as vt, vpr_head_training as ht
    inp = hr.make_inputs("C")
    model = _model_with(inp)
    feat = _dev(inp["feat"])
    l0 = float(ht.VPRHeadTrainer(model, lr=hr.LR).step_features(feat, inp["B"], inp["counts"]))
    trainer = ht.VPRHeadTrainer(model, lr=hr.LR)
    enc = trainer.forward_features(feat)[-1][1]
    w0 = model.vlad_head.netvlad.conv.weight.detach().clone()
    c1 = model.vlad_head.convlad1.conv.weight.detach().clone()
    l1 = float(vt.NetVLADTrainer(model, lr=hr.LR).step_encoded(enc, inp["B"], inp["counts"]))
    assert 0 < l1 < l0
    assert not torch.equal(model.vlad_head.netvlad.conv.weight.detach(), w0)
    assert torch.equal(model.vlad_head.convlad1.conv.weight.detach(), c1)


# ---- 4. the C ABI refuses before launching ----------------------------------------------------------------------------------
def test_c_abi_refuses_before_launching():
    from nano_vs_slam_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    p, null = C.c_void_p(buf.data_ptr()), None
    big = 1 << 18
    assert lib.kp2d_cbr_train_scratch_bytes(4, 5, 7, 16, 32) > 0
    for N, H, W, ci, co in ((0, 5, 7, 16, 16), (70000, 5, 7, 16, 16), (4, 0, 7, 16, 16), (4, 5, 0, 16, 16), (4, 5, 7, 24, 16), (4, 5, 7, 16, 8),
                            (4, 5, 7, 144, 16), (4, 5, 7, 16, 0)):
        assert lib.kp2d_cbr_train_scratch_bytes(N, H, W, ci, co) == 0
    assert lib.kp2d_cbr_forward_train(p, p, p, p, 0.01, 0, 5, 7, 16, 16, p, p, p, big, null) == -1          # KP2D_ERR_ARG
    assert lib.kp2d_cbr_forward_train(p, p, p, p, 0.01, 1, 5, 7, 24, 16, p, p, p, big, null) == -2          # KP2D_ERR_UNSUPPORTED
    assert lib.kp2d_cbr_forward_train(p, p, p, p, 1.5, 1, 5, 7, 16, 16, p, p, p, big, null) == -1
    assert lib.kp2d_cbr_forward_train(p, p, p, p, 0.01, 1, 5, 7, 16, 16, p, null, p, big, null) == -1 and b"null" in lib.kp2d_last_error()
    assert lib.kp2d_cbr_forward_train(p, p, p, p, 0.01, 1, 5, 7, 16, 16, p, p, p, 16, null) == -1 and b"scratch" in lib.kp2d_last_error()
    assert lib.kp2d_cbr_backward(p, p, p, p, p, 0.01, p, p, p, 1, 5, 7, 16, 160, p, p, p, null, p, big, null) == -2
    assert lib.kp2d_cbr_backward(p, p, p, p, p, 0.01, p, p, null, 1, 5, 7, 16, 16, p, p, p, null, p, big, null) == -1
    assert lib.kp2d_cbr_backward(p, p, p, p, p, 0.01, p, p, p, 1, 5, 7, 16, 16, p, p, p, null, p, 16, null) == -1 and b"scratch" in lib.kp2d_last_error()
    assert lib.kp2d_vlad_backward_input(p, p, p, p, p, 1, 8, 16, 8, null, p, big, null) == -1 and b"null" in lib.kp2d_last_error()
    assert lib.kp2d_vlad_backward_input(p, p, p, p, p, 1, 8, 256, 8, p, p, big, null) == -2
    assert lib.kp2d_vlad_backward_input(p, p, p, p, p, 1, 8, 16, 8, p, p, 16, null) == -1 and b"scratch" in lib.kp2d_last_error()
    torch.cuda.synchronize()
    assert not buf.any()
