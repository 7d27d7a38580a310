"""The depth head's training step on the device (nano_vs_slam_amd.depth_training, csrc/depth_train.hip, csrc/seg_train.hip,
csrc/vpr_head_train.hip) against the float64 outputs of the reference's SegmentationHead with one class in .eval(), .sigmoid(),
SILogLoss + torch.nn.HuberLoss under torch autograd and Adam (tests/golden/depth_training/, written by
tools/make_depth_training_golden.py; inputs regenerated from seeds by depth_training_ref).  The fixtures keep a stated stride
of every larger array, so the numpy float64 oracle, held to the stored entries to 1e-10, stands in for the whole arrays.

Error measure: for an array G, E(G) = max|G - G64| / max|G64|; for a scalar |v - v64| / |v64|.
Bound per quantity: max(8 x the reference modules' own float32 error of that quantity (the same modules run in float32 on the
CPU against their float64 run, the maximum over the cases), 16 x 2^-24), read from the fixtures (depth_training_ref.bounds).
The unpinned cases (saturated logits, M = 0, 1, 2, Dg = 0, non-finite pixels) are checked against the oracle ONLY, never
torch, with 16 x 2^-24 alone.  Counts are exact.  Every test prints the largest share of a bound it used.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import depth_training_ref as dr
from conftest import product_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4        # the project's inference contract in fp32 mode (test_gpu_parity.py)
sr = dr.sr


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _f32(a):
    return _dev(np.asarray(a, np.float32))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


class _Share:
    """Checks E <= bound, keeps the largest share of a bound."""

    def __init__(self, bounds, label):
        self.bounds, self.label, self.worst = bounds, label, (0.0, "")

    def __call__(self, key, got, want, bound_key=None):
        want = np.asarray(want, np.float64)
        got = (_np(got) if torch.is_tensor(got) else np.asarray(got, np.float64)).reshape(want.shape)
        scale = np.abs(want).max() if want.ndim else abs(float(want))
        diff = np.abs(got - want).max()
        e = diff / scale if scale > 0 else (0.0 if diff == 0 else np.inf)       # a quantity that is 0 must be 0
        b = self.bounds[bound_key or key]
        print(f"{self.label}: E({key}) {e:.3e} of {b:.3e}")
        if e / b > self.worst[0]:
            self.worst = (e / b, key)
        assert e <= b, f"{self.label}: E({key}) {e:.3e} above {b:.3e}"

    def report(self):
        print(f"{self.label}: largest share of a bound {self.worst[0]:.3f} ({self.worst[1]})")


def _loss(z, gt, **kw):
    from nano_vs_slam_amd import depth_training as dt
    return dt.depth_loss(_f32(z), _f32(gt), return_parts=True, **kw)


def _check_loss(chk, got, ref):
    loss, dz, valid, stray, parts = got
    assert loss.shape == () and dz.shape == ref["dz"].shape and parts.shape == (2,)
    assert int(valid) == ref["valid"] and int(stray) == ref["stray"]
    chk("loss", loss, ref["loss"])
    chk("silog", parts[0], ref["silog"])
    chk("huber", parts[1], ref["huber"])
    chk("dlogits", dz, ref["dz"])
    assert torch.isfinite(dz).all() and not dz[~_dev(ref["ok"])].any()


# ---- 1. the loss alone ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bounds():
    return dr.bounds()


@pytest.mark.parametrize("name", list(dr.LOSS_CASES))
def test_loss_alone(bounds, name):
    z, gt = dr.make_loss_inputs(name)
    ref, fx = dr.depth_loss(z, gt), dr.load_fixture(name)
    assert np.abs(dr.stored(ref["dz"]) - fx["dlogits"]).max() <= 1e-10 and abs(ref["loss"] - float(fx["loss"])) <= 1e-10
    chk = _Share(bounds, f"case {name} loss")
    _check_loss(chk, _loss(z, gt), ref)
    z4 = _loss(z[:, None], gt[:, None])                          # [N, 1, H, W] is the same call
    assert z4[1].shape == (z.shape[0], 1) + z.shape[1:] and torch.equal(z4[1][:, 0], _loss(z, gt)[1]) and torch.equal(z4[0], _loss(z, gt)[0])
    if name == "L2":                                             # other weights: the parts stay, the sum follows
        w = _loss(z, gt, silog_weight=0.25, huber_weight=3.0)
        _check_loss(chk, w, dr.depth_loss(z, gt, (0.25, 3.0)))
        assert torch.equal(w[4], _loss(z, gt)[4])
    chk.report()


def test_unpinned_cases_against_the_oracle():
    """Checked against the float64 oracle only (torch gives NaN or inf in each of them), bound 16 x 2^-24."""
    chk = _Share(dr.floor_bounds(), "unpinned")
    z, gt = dr.make_loss_inputs("L2")
    for big in (30.0, 200.0):                                    # saturation
        zz = np.where(np.arange(z.size).reshape(z.shape) % 2, big, -big).astype(np.float32)
        _check_loss(chk, _loss(zz, gt), dr.depth_loss(zz, gt))
    none = _loss(z, np.zeros_like(gt))                           # M = 0
    assert float(none[0]) == 0.0 and not none[1].any() and int(none[2]) == 0 and int(none[3]) == 0 and not none[4].any()
    for M in (1, 2):                                             # M = 1: Huber alone; M = 2: the smallest variance
        few = np.zeros_like(gt)
        few[1, 4, 7] = 2.5
        if M == 2:
            few[2, 16, 22] = 0.4
        ref = dr.depth_loss(z, few)
        got = _loss(z, few)
        _check_loss(chk, got, ref)
        assert int(got[2]) == M and (M == 2 or float(got[4][0]) == 0.0)
    flat = _loss(np.zeros((2, 5, 7), np.float32), np.full((2, 5, 7), 0.5, np.float32))       # Dg = 0
    print("Dg = 0:", float(flat[0]), flat[4].tolist(), float(flat[1].abs().max()))
    assert float(flat[0]) == 0.0 and not flat[1].any() and int(flat[2]) == 70
    bad_gt, bad_z, base = gt.copy(), z.copy(), gt.copy()         # non-finite pixels are stray: counted, and move nothing
    where = np.argwhere(gt > 0)[[0, 9, 33]]
    for i, v in zip(where, (np.nan, np.inf, -np.inf)):
        bad_gt[tuple(i)] = v
        base[tuple(i)] = 0.0
    bad_z[tuple(where[0])] = np.nan
    bad_z[tuple(np.argwhere(gt <= 0)[0])] = np.inf               # a non-finite logit where there is no ground truth: stray too
    a, b, c = _loss(z, bad_gt), _loss(z, base), _loss(bad_z, base)
    assert int(a[3]) == 3 and int(b[3]) == 0 and int(c[3]) == 2 and int(a[2]) == int(b[2]) == int(c[2])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(c[0], b[0]) and torch.equal(c[1], b[1])
    assert dr.depth_loss(bad_z, base)["stray"] == 2
    chk.report()


def test_loss_bits():
    """Two runs of L3 give identical bits; a wholly invalid frame changes no bit elsewhere, whatever finite values it holds."""
    z, gt = dr.make_loss_inputs("L3")
    a, b = _loss(z, gt), _loss(z, gt)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    z2, gt2 = z.copy(), gt.copy()
    rng = np.random.default_rng(5)
    z2[1] = (50.0 * rng.standard_normal(z[1].shape)).astype(np.float32)
    gt2[1] = -np.abs(rng.standard_normal(z[1].shape)).astype(np.float32) * 1e3
    c = _loss(z2, gt2)
    assert all(torch.equal(x, y) for x, y in zip(a, c)) and not c[1][1].any()


# ---- 2. the whole step ----------------------------------------------------------------------------------------------------
def _stand_in(inp):
    """A model-shaped holder of a V2 depth_head with the case's channel counts, parameters and statistics."""
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import _SegHead
    head = _SegHead(inp["c_in"], inp["c_hidden"], inp["d1"] // 4 + inp["c_skip"], 1, inp["d1"], 0.1, False).to(DEV)
    with torch.no_grad():
        for i in range(8):
            layer = head.convs[i]
            layer.conv.weight.copy_(_dev(inp["params"][3 * i]))
            layer.bn.weight.copy_(_dev(inp["params"][3 * i + 1]))
            layer.bn.bias.copy_(_dev(inp["params"][3 * i + 2]))
            layer.bn.running_mean.copy_(_dev(inp["stats"][i][0]))
            layer.bn.running_var.copy_(_dev(inp["stats"][i][1]))
            assert layer.bn.eps == dr.BN_EPS
        head.convs[8].weight.copy_(_dev(inp["params"][24]))
        head.convs[8].bias.copy_(_dev(inp["params"][25]))
    return types.SimpleNamespace(depth_head=head, _version_id=2, upscale_method="pixelshuffle", use_attention=False, leaky_relu=True)


def _run_step(inp):
    """forward, loss, backward through the layer calls as a training step chains them -> dict of device tensors."""
    from nano_vs_slam_amd import depth_training as dt, seg_training as st, vpr_head_training as ht
    x, skip, gt = _dev(inp["x"]), _dev(inp["skip"]), _dev(inp["gt"])
    r, acts = {}, {}

    def vectors(i):
        gamma, beta = _dev(inp["params"][3 * i + 1]), _dev(inp["params"][3 * i + 2])
        mean, var = _dev(inp["stats"][i][0]), _dev(inp["stats"][i][1])
        invstd = 1.0 / torch.sqrt(var + dr.BN_EPS)
        scale = gamma * invstd
        return scale, beta - mean * scale, mean, invstd

    def cbr(i, v):
        vec, w = vectors(i), _dev(inp["params"][3 * i])
        y, c = ht.cbr_forward(v, w, vec[0], vec[1], dr.SLOPE)
        acts[i] = (v, w, vec, y, c)
        r[f"y{i}"] = y
        return y

    y1 = cbr(1, cbr(0, x))
    r["pooled"] = st.maxpool2_forward(y1)
    y4 = cbr(4, cbr(3, cbr(2, r["pooled"])))
    r["cat1"] = st.shuffle_cat_forward(y4, x)
    y6 = cbr(6, cbr(5, r["cat1"]))
    r["cat2"] = st.shuffle_cat_forward(y6, skip)
    y7 = cbr(7, r["cat2"])
    w8, b8 = _dev(inp["params"][24]), _dev(inp["params"][25])
    r["logits"] = st.conv_bias_forward(y7, w8, b8)
    r["loss"], r["dlogits"], r["valid"], r["stray"], r["parts"] = dt.depth_loss(r["logits"], gt, *inp["weights"], return_parts=True)
    grads = [None] * 26
    grads[24], grads[25], r["d_y7"] = st.conv_bias_backward(y7, w8, r["dlogits"])

    def back(i, dy, need_dx=True):
        lx, w, (scale, _, mean, invstd), y, c = acts[i]
        dw, dgamma, dbeta, dx = ht.cbr_backward(lx, w, scale, mean, invstd, y, c, dy, dr.SLOPE, need_dx=need_dx)
        grads[3 * i:3 * i + 3] = [dw, dgamma, dbeta]
        return dx

    C4 = inp["d1"] // 4
    r["d_cat2"] = back(7, r["d_y7"])
    r["d_y6"] = st.shuffle_cat_backward(r["d_cat2"], C4)
    r["d_y5"] = back(6, r["d_y6"])
    r["d_cat1"] = back(5, r["d_y5"])
    r["d_y4"] = st.shuffle_cat_backward(r["d_cat1"], C4)
    r["d_y3"] = back(4, r["d_y4"])
    r["d_y2"] = back(3, r["d_y3"])
    r["d_pooled"] = back(2, r["d_y2"])
    r["d_y1"] = st.maxpool2_backward(y1, r["d_pooled"])
    r["d_y0"] = back(1, r["d_y1"])
    assert back(0, r["d_y0"], need_dx=False) is None
    r["grads"] = grads
    return r


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in dr.STEP_CASES:
        inp = dr.make_inputs(name)
        fx = dr.load_fixture(name)
        ref = dr.step_gradients(inp)
        for k in dr.MAPS + dr.DMAPS:                     # the oracle stands in for the whole arrays: held to the fixture here
            assert np.abs(dr.stored(ref[k]) - fx[k]).max() <= 1e-10, k
        for i, g in enumerate(ref["grads"]):
            assert np.abs(dr.stored(g) - fx[f"g{i}"]).max() <= 1e-10, dr.PARAMS[i]
        assert abs(ref["loss"] - float(fx["loss"])) <= 1e-10 and ref["valid"] == int(fx["valid"])
        out[name] = (inp, _run_step(inp), ref)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(dr.STEP_CASES))
def test_whole_step(runs, bounds, name):
    inp, r, ref = runs[name]
    chk = _Share(bounds, f"case {name} whole step")
    for k in dr.MAPS + dr.DMAPS:
        assert tuple(r[k].shape) == ref[k].shape, k
        chk(k, r[k], ref[k])
    chk("loss", r["loss"], ref["loss"])
    chk("silog", r["parts"][0], ref["silog"])
    chk("huber", r["parts"][1], ref["huber"])
    assert int(r["valid"]) == ref["valid"] and int(r["stray"]) == 0
    for i in range(26):
        assert r["grads"][i].numel() == inp["params"][i].size
        chk(f"g{i}", r["grads"][i], ref["grads"][i])
    chk.report()


@pytest.mark.parametrize("name", list(dr.STEP_CASES))
def test_trainer_gradients_in_both_modes(runs, bounds, name):
    """DepthHeadTrainer.gradients walks the head as the chained layer calls do: the same bits (so a second run of the step
    is bit-identical too).  "last" mode on the last layer's input: both gradients, the same bits again."""
    from nano_vs_slam_amd import depth_training as dt
    inp, r, ref = runs[name]
    model = _stand_in(inp)
    x, skip, gt = _dev(inp["x"]), _dev(inp["skip"]), _dev(inp["gt"])
    trainer = dt.DepthHeadTrainer(model, train="head")
    loss, logits, grads = trainer.gradients(x, skip, gt[:, None])
    assert len(grads) == 26 and torch.equal(loss, r["loss"]) and torch.equal(logits, r["logits"]) and logits.shape[1] == 1
    for i, (a, b) in enumerate(zip(grads, r["grads"])):
        assert torch.equal(a, b), dr.PARAMS[i]
    assert torch.equal(trainer.forward_features(x, skip), r["logits"]) and torch.equal(trainer.parts, r["parts"])
    last = dt.DepthHeadTrainer(model, train="last")
    loss2, logits2, g2 = last.gradients(r["y7"], None, gt)
    assert len(g2) == 2 and len(last.parameters()) == 2
    assert torch.equal(loss2, r["loss"]) and torch.equal(logits2, r["logits"])
    assert torch.equal(g2[0], r["grads"][24]) and torch.equal(g2[1], r["grads"][25])
    chk = _Share(bounds, f"case {name} last mode")
    chk("g24", g2[0], ref["grads"][24])
    chk("g25", g2[1], ref["grads"][25])
    chk.report()
    assert int(last.valid) == ref["valid"] and int(last.stray) == 0


def test_trajectories():
    """Case C: ten Adam steps over all 26 parameters and three over the last layer's two, the loss of and every trained
    parameter after every step."""
    from nano_vs_slam_amd import depth_training as dt
    inp = dr.make_inputs(dr.TRAJECTORY_CASE)
    fx = dr.load_trajectory()
    tb = dr.trajectory_bounds()
    x, skip, gt = _dev(inp["x"]), _dev(inp["skip"]), _dev(inp["gt"])
    y7 = dt.DepthHeadTrainer(_stand_in(inp))._forward(x, skip)[1]["feat"]      # the last layer's input, which "last" mode takes
    for mode, steps, trained in (("head", dr.HEAD_STEPS, list(range(26))), ("last", dr.LAST_STEPS, [24, 25])):
        model = _stand_in(inp)
        trainer = dt.DepthHeadTrainer(model, lr=float(fx["lr"]), train=mode)
        chk = _Share(tb, f"trajectory {mode}")
        frozen = [p.detach().clone() for p in model.depth_head.parameters()]
        stats0 = [(l.bn.running_mean.clone(), l.bn.running_var.clone()) for l in model.depth_head.convs[:8]]
        feat = (x, skip) if mode == "head" else (y7, None)
        losses = []
        for t in range(steps):
            versions = [p._version for p in trainer.parameters()]
            losses.append(trainer.step_features(feat[0], feat[1], gt))
            assert all(p._version > v for p, v in zip(trainer.parameters(), versions))
            for i, p in zip(trained, trainer.parameters()):
                chk(f"p{i}_{mode}", dr.stored(_np(p), dr.TRAJ_STORED), fx[f"p{i}_{mode}"][t])
        losses = np.asarray([float(l) for l in losses])
        for l, l64 in zip(losses, fx[f"losses_{mode}"]):
            chk(f"loss_{mode}", l, np.float64(l64))
        assert (losses[1:] < losses[:-1]).all() and trainer.steps == steps
        chk.report()
        for l, (m0, v0) in zip(model.depth_head.convs[:8], stats0):      # the running statistics do not move
            assert torch.equal(l.bn.running_mean, m0) and torch.equal(l.bn.running_var, v0)
        if mode == "last":                                               # and nothing but the last layer does
            assert all(torch.equal(a, b) for a, b in zip(frozen[:24], model.depth_head.parameters()))


def test_step_bits(runs):
    inp, r, _ = runs["A"]
    again = _run_step(inp)
    for k in dr.MAPS + dr.DMAPS + ("loss", "valid", "stray", "parts"):
        assert torch.equal(again[k], r[k]), k
    for i, (a, b) in enumerate(zip(again["grads"], r["grads"])):
        assert torch.equal(a, b), dr.PARAMS[i]


# ---- 3. wiring ----------------------------------------------------------------------------------------------------------------
def test_engine_follows_three_steps():
    """A config-S depth=True model at 64 x 96: before and after three steps the engine's own forward, which re-packs the
    updated weights, agrees with sigmoid(training forward) within the inference contract; the loss and abs_rel have fallen."""
    from nano_vs_slam_amd import dense_metrics as dm, depth_training as dt
    from oracle.weights import synthetic_frames
    model, _ = product_model("S+depth", False, 28, DEV)
    model.set_precision("fp32")
    frames = _dev(synthetic_frames(2, 64, 96, seed=43))
    rng = np.random.default_rng(43)
    gt = (0.02 + 0.04 * rng.random((2, 32, 48))).astype(np.float32)     # a near range well below what the untrained head gives,
                                                                        # so that the first steps' direction is not in doubt
    gt[rng.random(gt.shape) < 0.2] = 0.0
    gt = _dev(gt)
    with torch.no_grad():
        x, skip = model.backbone_maps(frames)
        trainer = dt.DepthHeadTrainer(model, lr=1e-4)
        seg0 = model(frames)["seg"].clone()
        d0 = model(frames)["depth"].clone()
        err0 = float((d0 - torch.sigmoid(trainer.forward_features(x, skip))).abs().max())
        rel0 = float(dm.compute_errors_torch(gt[:, None], d0)["abs_rel"])
        losses = [float(trainer.step_features(x, skip, gt)) for _ in range(3)]
        out = model(frames)
        d1 = out["depth"]
        err1 = float((d1 - torch.sigmoid(trainer.forward_features(x, skip))).abs().max())
        rel1 = float(dm.compute_errors_torch(gt[:, None], d1)["abs_rel"])
    moved = float((d1 - d0).abs().max())
    print(f"sigmoid(training forward) vs the engine: before {err0:.3e}, after {err1:.3e} of {TOL}; moved {moved:.3e}; losses {losses}; "
          f"abs_rel {rel0:.4f} -> {rel1:.4f}")
    assert d0.shape == (2, 1, 32, 48) and err0 <= TOL and err1 <= TOL and moved > TOL
    assert losses[2] < losses[0] and rel1 < rel0
    assert torch.equal(out["seg"], seg0)                                # the segmentation head is not touched
    # "last" mode through step(): the tap on the last layer's input
    last = dt.DepthHeadTrainer(model, lr=1e-4, train="last")
    w0 = model.depth_head.convs[7].conv.weight.detach().clone()
    l0 = float(last.step(frames, gt))
    l1 = float(last.step(frames, gt[:, None]))
    assert l1 < l0 and torch.equal(model.depth_head.convs[7].conv.weight.detach(), w0)
    l_head = float(dt.DepthHeadTrainer(model, lr=1e-4).step(frames, gt))
    assert l_head < l1


# ---- 4. the C ABI refuses before launching -----------------------------------------------------------------------------------
def test_c_abi_refuses_before_launching():
    from nano_vs_slam_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    p, null = C.c_void_p(buf.data_ptr()), None
    big = 1 << 18
    assert lib.kp2d_depth_loss_scratch_bytes(2, 35) > 0
    for N, HW in ((0, 35), (70000, 35), (1, 0), (1, -4), (1, (1 << 30) + 1)):
        assert lib.kp2d_depth_loss_scratch_bytes(N, HW) == 0
    assert lib.kp2d_depth_loss(p, p, 0, 35, 1.0, 1.0, p, p, p, p, p, p, big, null) == -1                # KP2D_ERR_ARG
    assert lib.kp2d_depth_loss(p, p, 1, 0, 1.0, 1.0, p, p, p, p, p, p, big, null) == -1
    assert lib.kp2d_depth_loss(p, p, 1, (1 << 30) + 1, 1.0, 1.0, p, p, p, p, p, p, big, null) == -2     # KP2D_ERR_UNSUPPORTED
    for ws, wh in ((-0.5, 1.0), (1.0, -1.0), (float("nan"), 1.0), (1.0, float("inf"))):
        assert lib.kp2d_depth_loss(p, p, 1, 35, ws, wh, p, p, p, p, p, p, big, null) == -1 and b"weights" in lib.kp2d_last_error()
    for k in range(7):                                                   # each pointer in turn
        a = [p] * 7
        a[k] = null
        assert lib.kp2d_depth_loss(a[0], a[1], 1, 35, 1.0, 1.0, a[2], a[3], a[4], a[5], a[6], p, big, null) == -1 and b"null" in lib.kp2d_last_error()
    assert lib.kp2d_depth_loss(p, p, 1, 35, 1.0, 1.0, p, p, p, p, p, null, big, null) == -1
    assert lib.kp2d_depth_loss(p, p, 1, 35, 1.0, 1.0, p, p, p, p, p, p, 16, null) == -1 and b"scratch" in lib.kp2d_last_error()
    torch.cuda.synchronize()
    assert not buf.any()
