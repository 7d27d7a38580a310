"""The segmentation head's training step on the device (nano_vs_slam_amd.seg_training, csrc/seg_train.hip,
csrc/vpr_head_train.hip) against the float64 outputs of the reference's SegmentationHead in .eval() under torch autograd,
CrossEntropyLoss, the restated Dice loss and Adam (tests/golden/seg_training/, written by tools/make_seg_training_golden.py;
inputs regenerated from seeds by seg_training_ref.make_inputs).  The fixtures keep a stated stride of every larger array, so
the numpy float64 oracle, held to the stored entries to 1e-10, stands in for the whole arrays.

Error measure: for an array G, E(G) = max|G - G64| / max|G64|; for the loss |loss - loss64| / |loss64|.
Bound per quantity: max(8 x the reference module's own float32 error of that quantity (the same module run in float32 on the
CPU against its float64 run, the maximum over the cases), 16 x 2^-24), read from the fixtures (seg_training_ref.bounds).  The
factor 8 is for another summation order (tiles, slabs, chunks, frames) and another exponential; a missing or wrong term gives
E >= 1e-2.  Counts are exact; pooling and shuffling are bit-exact against torch.  Every test prints the largest share of a
bound it used.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import seg_training_ref as sr
from conftest import product_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4        # the project's inference contract in fp32 mode (test_gpu_parity.py)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _f32(a):
    return _dev(np.asarray(a, np.float32))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _vectors(inp, i):
    """(scale, shift, mean, invstd) of BatchNorm layer i, formed with torch on the device in float32."""
    gamma, beta = _dev(inp["params"][3 * i + 1]), _dev(inp["params"][3 * i + 2])
    mean, var = _dev(inp["stats"][i][0]), _dev(inp["stats"][i][1])
    invstd = 1.0 / torch.sqrt(var + sr.BN_EPS)
    scale = gamma * invstd
    return scale, beta - mean * scale, mean, invstd


def _run_step(inp):
    """forward, loss, backward through the layer calls as a training step chains them -> dict of device tensors."""
    from nano_vs_slam_amd import seg_training as st, vpr_head_training as ht
    x, skip, labels = _dev(inp["x"]), _dev(inp["skip"]), _dev(inp["labels"])
    r, acts = {}, {}

    def cbr(i, v):
        vec, w = _vectors(inp, i), _dev(inp["params"][3 * i])
        y, c = ht.cbr_forward(v, w, vec[0], vec[1], sr.SLOPE)
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
    r["loss"], r["dlogits"], r["valid"], r["stray"] = st.segmentation_loss(r["logits"], labels, *inp["weights"], ignore_index=sr.IGNORE)
    grads = [None] * 26
    grads[24], grads[25], r["d_y7"] = st.conv_bias_backward(y7, w8, r["dlogits"])

    def back(i, dy, need_dx=True):
        lx, w, (scale, _, mean, invstd), y, c = acts[i]
        dw, dgamma, dbeta, dx = ht.cbr_backward(lx, w, scale, mean, invstd, y, c, dy, sr.SLOPE, need_dx=need_dx)
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
    assert back(0, r["d_y0"], need_dx=False) is None      # the backbone is frozen: convs.0 forms no dx
    r["grads"] = grads
    return r


def _stand_in(inp):
    """A model-shaped holder of a V2 seg_head with the case's channel counts, parameters and statistics (the trainer reads
    nothing else of a model in step_features)."""
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import _SegHead
    head = _SegHead(inp["c_in"], inp["c_hidden"], inp["d1"] // 4 + inp["c_skip"], inp["classes"], inp["d1"], 0.1, False).to(DEV)
    with torch.no_grad():
        for i in range(8):
            layer = head.convs[i]
            layer.conv.weight.copy_(_dev(inp["params"][3 * i]))
            layer.bn.weight.copy_(_dev(inp["params"][3 * i + 1]))
            layer.bn.bias.copy_(_dev(inp["params"][3 * i + 2]))
            layer.bn.running_mean.copy_(_dev(inp["stats"][i][0]))
            layer.bn.running_var.copy_(_dev(inp["stats"][i][1]))
            assert layer.bn.eps == sr.BN_EPS
        head.convs[8].weight.copy_(_dev(inp["params"][24]))
        head.convs[8].bias.copy_(_dev(inp["params"][25]))
    return types.SimpleNamespace(seg_head=head, _version_id=2, upscale_method="pixelshuffle", use_attention=False, leaky_relu=True)


@pytest.fixture(scope="module")
def bounds():
    return sr.bounds()


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in sr.CASES:
        inp = sr.make_inputs(name)
        fx = sr.load_fixture(name)
        ref = sr.step_gradients(inp)
        for k in sr.MAPS + sr.DMAPS:                     # the oracle stands in for the whole arrays: held to the fixture here
            assert np.abs(sr.stored(ref[k]) - fx[k]).max() <= 1e-10, k
        for i, g in enumerate(ref["grads"]):
            assert np.abs(sr.stored(g) - fx[f"g{i}"]).max() <= 1e-10, sr.PARAMS[i]
        assert abs(ref["loss"] - float(fx["loss"])) <= 1e-10 and ref["valid"] == int(fx["valid"])
        out[name] = (inp, _run_step(inp), ref)
    torch.cuda.synchronize()
    return out


class _Share:
    """Checks E <= bound, keeps the largest share of a bound."""

    def __init__(self, bounds, label):
        self.bounds, self.label, self.worst = bounds, label, (0.0, "")

    def __call__(self, key, got, want, bound_key=None):
        want = np.asarray(want, np.float64)
        got = (_np(got) if torch.is_tensor(got) else np.asarray(got, np.float64)).reshape(want.shape)
        e = sr.rel_err(got, want) if want.ndim else abs(float(got) - float(want)) / abs(float(want))
        b = self.bounds[bound_key or key]
        if e / b > self.worst[0]:
            self.worst = (e / b, key)
        assert e <= b, f"{self.label}: E({key}) {e:.3e} above {b:.3e}"

    def report(self):
        print(f"{self.label}: largest share of a bound {self.worst[0]:.3f} ({self.worst[1]})")


# ---- 1. each layer call alone, on the oracle's inputs rounded to float32 -------------------------------------------------
@pytest.mark.parametrize("name", list(sr.CASES))
def test_last_layer_alone(runs, bounds, name):
    from nano_vs_slam_amd import seg_training as st
    inp, _, ref = runs[name]
    chk = _Share(bounds, f"case {name} conv + bias")
    y7, w, b = _f32(ref["y7"]), _dev(inp["params"][24]), _dev(inp["params"][25])
    logits = st.conv_bias_forward(y7, w, b)
    assert logits.shape == ref["logits"].shape
    chk("logits", logits, ref["logits"])
    dz = _f32(ref["dlogits"])
    dw, db, dx = st.conv_bias_backward(y7, w, dz)
    dw2, db2, none = st.conv_bias_backward(y7, w, dz, need_dx=False)
    assert none is None and torch.equal(dw, dw2) and torch.equal(db, db2)
    assert dw.shape == w.shape and db.shape == b.shape and dx.shape == y7.shape
    chk("g24", dw, ref["grads"][24])
    chk("g25", db, ref["grads"][25])
    chk("d_y7", dx, ref["d_y7"])
    chk.report()


@pytest.mark.parametrize("name", list(sr.CASES))
def test_loss_alone(runs, bounds, name):
    from nano_vs_slam_amd import seg_training as st
    inp, _, ref = runs[name]
    chk = _Share(bounds, f"case {name} loss")
    z = _f32(ref["logits"])
    outs = []
    for dtype in (torch.uint8, torch.int32, torch.int64):
        loss, dz, valid, stray = st.segmentation_loss(z, _dev(inp["labels"]).to(dtype), *inp["weights"], ignore_index=sr.IGNORE)
        assert int(valid) == ref["valid"] and int(stray) == 0
        assert loss.shape == () and dz.shape == z.shape
        outs.append((loss, dz))
    for loss, dz in outs[1:]:
        assert torch.equal(loss, outs[0][0]) and torch.equal(dz, outs[0][1])
    chk("loss", outs[0][0], ref["loss"])
    chk("dlogits", outs[0][1], ref["dlogits"])
    chk.report()


@pytest.mark.parametrize("name", list(sr.CASES))
def test_pool_and_shuffle_alone(runs, bounds, name):
    from nano_vs_slam_amd import seg_training as st
    inp, _, ref = runs[name]
    chk = _Share(bounds, f"case {name} pool, shuffle")
    C4 = inp["d1"] // 4
    chk("pooled", st.maxpool2_forward(_f32(ref["y1"])), ref["pooled"])
    chk("d_y1", st.maxpool2_backward(_f32(ref["y1"]), _f32(ref["d_pooled"])), ref["d_y1"])
    chk("cat1", st.shuffle_cat_forward(_f32(ref["y4"]), _dev(inp["x"])), ref["cat1"])
    chk("cat2", st.shuffle_cat_forward(_f32(ref["y6"]), _dev(inp["skip"])), ref["cat2"])
    chk("d_y4", st.shuffle_cat_backward(_f32(ref["d_cat1"]), C4), ref["d_y4"])
    chk("d_y6", st.shuffle_cat_backward(_f32(ref["d_cat2"]), C4), ref["d_y6"])
    chk.report()


# ---- 2. the whole step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.CASES))
def test_whole_step(runs, bounds, name):
    inp, r, ref = runs[name]
    chk = _Share(bounds, f"case {name} whole step")
    for k in sr.MAPS + sr.DMAPS:
        assert tuple(r[k].shape) == ref[k].shape, k
        chk(k, r[k], ref[k])
    chk("loss", r["loss"], ref["loss"])
    assert int(r["valid"]) == ref["valid"] and int(r["stray"]) == 0
    for i in range(26):
        assert r["grads"][i].numel() == inp["params"][i].size
        chk(f"g{i}", r["grads"][i], ref["grads"][i])
    chk.report()


@pytest.mark.parametrize("name", list(sr.CASES))
def test_trainer_gradients_in_both_modes(runs, bounds, name):
    """SegHeadTrainer.gradients walks the head as the chained layer calls do: the same bits.  "last" mode on the device's
    own input of the last layer: both gradients, the same bits again, and no other parameter is touched."""
    from nano_vs_slam_amd import seg_training as st
    inp, r, ref = runs[name]
    model = _stand_in(inp)
    x, skip, labels = _dev(inp["x"]), _dev(inp["skip"]), _dev(inp["labels"])
    wce, wd = inp["weights"]
    trainer = st.SegHeadTrainer(model, train="head", ce_weight=wce, dice_weight=wd)
    loss, logits, grads = trainer.gradients(x, skip, labels)
    assert len(grads) == 26 and torch.equal(loss, r["loss"]) and torch.equal(logits, r["logits"])
    for i, (a, b) in enumerate(zip(grads, r["grads"])):
        assert torch.equal(a, b), sr.PARAMS[i]
    assert torch.equal(trainer.forward_features(x, skip), r["logits"])
    last = st.SegHeadTrainer(model, train="last", ce_weight=wce, dice_weight=wd)
    loss2, logits2, g2 = last.gradients(r["y7"], None, labels)
    assert len(g2) == 2 and len(last.parameters()) == 2
    assert torch.equal(loss2, r["loss"]) and torch.equal(logits2, r["logits"])
    assert torch.equal(g2[0], r["grads"][24]) and torch.equal(g2[1], r["grads"][25])
    chk = _Share(bounds, f"case {name} last mode")
    chk("g24", g2[0], ref["grads"][24])
    chk("g25", g2[1], ref["grads"][25])
    chk.report()
    assert int(last.valid) == ref["valid"] and int(last.stray) == 0


def test_trajectories():
    """Case A: ten Adam steps over all 26 parameters and three over the last layer's two, the loss of and every trained
    parameter after every step."""
    from nano_vs_slam_amd import seg_training as st
    inp = sr.make_inputs(sr.TRAJECTORY_CASE)
    fx = sr.load_trajectory()
    tb = sr.trajectory_bounds()
    x, skip, labels = _dev(inp["x"]), _dev(inp["skip"]), _dev(inp["labels"])
    y7 = st.SegHeadTrainer(_stand_in(inp))._forward(x, skip)[1]["feat"]      # the last layer's input, which "last" mode takes
    for mode, steps, trained in (("head", sr.HEAD_STEPS, list(range(26))), ("last", sr.LAST_STEPS, [24, 25])):
        model = _stand_in(inp)
        trainer = st.SegHeadTrainer(model, lr=float(fx["lr"]), train=mode)
        chk = _Share(tb, f"trajectory {mode}")
        frozen = [p.detach().clone() for p in model.seg_head.parameters()]
        stats0 = [(l.bn.running_mean.clone(), l.bn.running_var.clone()) for l in model.seg_head.convs[:8]]
        feat = (x, skip) if mode == "head" else (y7, None)
        losses = []
        for t in range(steps):
            versions = [p._version for p in trainer.parameters()]
            losses.append(trainer.step_features(feat[0], feat[1], labels))
            assert all(p._version > v for p, v in zip(trainer.parameters(), versions))
            for i, p in zip(trained, trainer.parameters()):
                chk(f"p{i}_{mode}", sr.stored(_np(p), sr.TRAJ_STORED), fx[f"p{i}_{mode}"][t])
        losses = np.asarray([float(l) for l in losses])
        for l, l64 in zip(losses, fx[f"losses_{mode}"]):
            chk(f"loss_{mode}", l, np.float64(l64))
        assert (losses[1:] < losses[:-1]).all() and trainer.steps == steps
        chk.report()
        for l, (m0, v0) in zip(model.seg_head.convs[:8], stats0):       # the running statistics do not move
            assert torch.equal(l.bn.running_mean, m0) and torch.equal(l.bn.running_var, v0)
        if mode == "last":                                              # and nothing but the last layer does
            assert all(torch.equal(a, b) for a, b in zip(frozen[:24], model.seg_head.parameters()))


# ---- 3. bits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.CASES))
def test_bit_reproducible(runs, name):
    inp, r, _ = runs[name]
    again = _run_step(inp)
    for k in sr.MAPS + sr.DMAPS + ("loss", "valid", "stray"):
        assert torch.equal(again[k], r[k]), k
    for i, (a, b) in enumerate(zip(again["grads"], r["grads"])):
        assert torch.equal(a, b), sr.PARAMS[i]


def test_padding_is_inert(runs):
    """19 classes are padded to 32 in the packed weights: scratch pre-filled with NaN changes no bit of the logits or of the
    last layer's gradients, and none of them is NaN."""
    from nano_vs_slam_amd import _lib, seg_training as st
    inp, r, _ = runs["B"]
    y7, w, b, dz = r["y7"], _dev(inp["params"][24]), _dev(inp["params"][25]), r["dlogits"]
    N, Cin, H, W = y7.shape
    nbytes = int(_lib.load().kp2d_conv_bias_scratch_bytes(N, H, W, Cin, 19))
    nan = torch.full((nbytes + 1024,), 0xFF, dtype=torch.uint8, device=DEV)
    assert torch.isnan(nan[:nbytes // 4 * 4].view(torch.float32)).all()
    logits = st.conv_bias_forward(y7, w, b, scratch=nan)
    nan.fill_(0xFF)
    dw, db, dx = st.conv_bias_backward(y7, w, dz, scratch=nan)
    assert torch.equal(logits, r["logits"]) and torch.equal(dw, r["grads"][24]) and torch.equal(db, r["grads"][25]) and torch.equal(dx, r["d_y7"])
    for t in (logits, dw, db, dx):
        assert torch.isfinite(t).all()


def test_all_ignored_batch(runs):
    from nano_vs_slam_amd import seg_training as st
    inp, r, _ = runs["A"]
    labels = torch.full_like(_dev(inp["labels"]), sr.IGNORE)
    loss, dz, valid, stray = st.segmentation_loss(r["logits"], labels)
    assert float(loss) == 0.0 and not dz.any() and int(valid) == 0 and int(stray) == 0
    model = _stand_in(inp)
    trainer = st.SegHeadTrainer(model)
    before = [p.detach().clone() for p in trainer.parameters()]
    loss, _, grads = trainer.gradients(_dev(inp["x"]), _dev(inp["skip"]), labels)
    assert float(loss) == 0.0 and all(torch.isfinite(g).all() and not g.any() for g in grads)
    assert float(trainer.step_features(_dev(inp["x"]), _dev(inp["skip"]), labels)) == 0.0
    assert all(torch.equal(a, b) and torch.isfinite(b).all() for a, b in zip(before, trainer.parameters()))


def test_stray_labels_are_counted_and_move_nothing(runs):
    from nano_vs_slam_amd import seg_training as st
    inp, r, _ = runs["A"]
    lab = inp["labels"].astype(np.int64)
    where = np.argwhere(lab != sr.IGNORE)[[0, 5, 11]]
    stray, ignored = lab.copy(), lab.copy()
    for n, (i, v) in enumerate(zip(where, (5, -1, 1000))):       # the first class that does not exist, a negative, a large one
        stray[tuple(i)] = v
        ignored[tuple(i)] = sr.IGNORE
    a = st.segmentation_loss(r["logits"], _dev(stray))
    b = st.segmentation_loss(r["logits"], _dev(ignored))
    assert int(a[3]) == 3 and int(b[3]) == 0 and int(a[2]) == int(b[2]) == int(r["valid"]) - 3
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    none = st.segmentation_loss(r["logits"], _dev(lab), ignore_index=None)       # 255 is then a stray label, not an ignored one
    assert int(none[3]) == int((lab == sr.IGNORE).sum()) and torch.equal(none[1], r["dlogits"])


def test_pool_and_shuffle_are_bit_exact_against_torch():
    from nano_vs_slam_amd import seg_training as st
    g = torch.Generator(device="cpu").manual_seed(5)
    for shape in ((2, 3, 6, 10), (1, 5, 7, 9), (3, 2, 2, 2), (2, 16, 33, 47)):
        x = torch.randn(shape, generator=g).to(DEV)
        assert torch.equal(st.maxpool2_forward(x), torch.nn.functional.max_pool2d(x, 2, 2))
        ties = torch.randint(0, 3, shape, generator=g).float().to(DEV).requires_grad_(True)       # equal maxima in most windows
        y = torch.nn.functional.max_pool2d(ties, 2, 2)
        dy = torch.randn(tuple(y.shape), generator=g).to(DEV)
        y.backward(dy)
        assert torch.equal(st.maxpool2_forward(ties.detach()), y.detach())
        assert torch.equal(st.maxpool2_backward(ties.detach(), dy), ties.grad)
    for N, Cc, Cb, h, w in ((2, 4, 3, 3, 5), (1, 16, 16, 6, 10), (2, 1, 1, 1, 1), (1, 32, 64, 9, 7)):
        a = torch.randn((N, 4 * Cc, h, w), generator=g).to(DEV).requires_grad_(True)
        b = torch.randn((N, Cb, 2 * h, 2 * w), generator=g).to(DEV)
        out = torch.cat([torch.nn.functional.pixel_shuffle(a, 2), b], dim=1)
        d = torch.randn(tuple(out.shape), generator=g).to(DEV)
        out.backward(d)
        assert torch.equal(st.shuffle_cat_forward(a.detach(), b), out.detach())
        assert torch.equal(st.shuffle_cat_backward(d, Cc), a.grad)


# ---- 4. wiring ----------------------------------------------------------------------------------------------------------------
def test_engine_follows_three_steps():
    """A config-S model at 64 x 96: after three steps on the maps of model.backbone_maps the engine's own forward, which
    re-packs the updated weights, agrees with the training forward within the inference contract; the loss has fallen."""
    from nano_vs_slam_amd import seg_training as st
    from oracle.weights import synthetic_frames
    model, _ = product_model("S", False, 28, DEV)
    model.set_precision("fp32")
    frames = _dev(synthetic_frames(2, 64, 96, seed=41))
    rng = np.random.default_rng(41)
    labels = rng.integers(0, 28, (2, 32, 48)).astype(np.uint8)
    labels[rng.random(labels.shape) < 0.1] = 255
    labels = _dev(labels)
    with torch.no_grad():
        x, skip = model.backbone_maps(frames)
        assert x.shape == (2, 64, 16, 24) and skip.shape == (2, 64, 32, 48) and torch.isfinite(x).all() and torch.isfinite(skip).all()
        assert torch.equal(x, model.backbone_features(frames))
        trainer = st.SegHeadTrainer(model, lr=1e-3)
        seg0 = model(frames)["seg"].clone()
        err0 = float((seg0 - trainer.forward_features(x, skip)).abs().max())
        losses = [float(trainer.step_features(x, skip, labels)) for _ in range(3)]
        seg1 = model(frames)["seg"]
        err1 = float((seg1 - trainer.forward_features(x, skip)).abs().max())
    moved = float((seg1 - seg0).abs().max())
    print(f"training forward vs the engine: before {err0:.3e}, after {err1:.3e} of {TOL}; moved {moved:.3e}; losses {losses}")
    assert err0 <= TOL and err1 <= TOL and moved > TOL
    assert losses[2] < losses[0]
    # "last" mode through step(): the tap on the last layer's input
    last = st.SegHeadTrainer(model, lr=1e-3, train="last")
    w0 = model.seg_head.convs[7].conv.weight.detach().clone()
    l0 = float(last.step(frames, labels))
    l1 = float(last.step(frames, labels))
    assert l1 < l0 and torch.equal(model.seg_head.convs[7].conv.weight.detach(), w0)
    l_head = float(st.SegHeadTrainer(model, lr=1e-3).step(frames, labels))
    assert l_head < l1


# ---- 5. the C ABI refuses before launching -----------------------------------------------------------------------------------
def test_c_abi_refuses_before_launching():
    from nano_vs_slam_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    p, null = C.c_void_p(buf.data_ptr()), None
    big = 1 << 18
    assert lib.kp2d_conv_bias_scratch_bytes(2, 5, 7, 16, 19) > 0 and lib.kp2d_seg_loss_scratch_bytes(2, 35, 19) > 0
    for N, H, W, ci, co in ((0, 5, 7, 16, 5), (70000, 5, 7, 16, 5), (2, 0, 7, 16, 5), (2, 5, 7, 24, 5), (2, 5, 7, 144, 5), (2, 5, 7, 16, 0),
                            (2, 5, 7, 16, 129)):
        assert lib.kp2d_conv_bias_scratch_bytes(N, H, W, ci, co) == 0
    assert lib.kp2d_conv_bias_forward_train(p, p, p, 0, 5, 7, 16, 5, p, p, big, null) == -1           # KP2D_ERR_ARG
    assert lib.kp2d_conv_bias_forward_train(p, p, p, 1, 5, 7, 24, 5, p, p, big, null) == -2           # KP2D_ERR_UNSUPPORTED
    assert lib.kp2d_conv_bias_forward_train(p, p, null, 1, 5, 7, 16, 5, p, p, big, null) == -1 and b"null" in lib.kp2d_last_error()
    assert lib.kp2d_conv_bias_forward_train(p, p, p, 1, 5, 7, 16, 5, p, p, 16, null) == -1 and b"scratch" in lib.kp2d_last_error()
    assert lib.kp2d_conv_bias_backward(p, p, p, 1, 5, 7, 16, 200, p, p, null, p, big, null) == -2
    assert lib.kp2d_conv_bias_backward(p, p, null, 1, 5, 7, 16, 5, p, p, null, p, big, null) == -1
    assert lib.kp2d_conv_bias_backward(p, p, p, 1, 5, 7, 16, 5, p, p, null, p, 16, null) == -1 and b"scratch" in lib.kp2d_last_error()
    assert lib.kp2d_seg_loss_scratch_bytes(0, 35, 5) == 0 and lib.kp2d_seg_loss_scratch_bytes(1, 0, 5) == 0 and lib.kp2d_seg_loss_scratch_bytes(1, 35, 129) == 0
    assert lib.kp2d_seg_loss(p, p, 7, 1, 35, 5, 255, 0.5, 1.5, p, p, p, p, p, big, null) == -1
    assert lib.kp2d_seg_loss(p, p, 0, 1, 35, 5, 255, -0.5, 1.5, p, p, p, p, p, big, null) == -1
    assert lib.kp2d_seg_loss(p, p, 0, 1, 35, 200, 255, 0.5, 1.5, p, p, p, p, p, big, null) == -2
    assert lib.kp2d_seg_loss(p, p, 0, 1, 35, 5, 255, 0.5, 1.5, p, null, p, p, p, big, null) == -1 and b"null" in lib.kp2d_last_error()
    assert lib.kp2d_seg_loss(p, p, 0, 1, 35, 5, 255, 0.5, 1.5, p, p, p, p, p, 16, null) == -1 and b"scratch" in lib.kp2d_last_error()
    assert lib.kp2d_maxpool2_forward_train(p, 1, 4, 1, 6, p, null) == -1 and lib.kp2d_maxpool2_forward_train(p, 1, 4, 6, 6, null, null) == -1
    assert lib.kp2d_maxpool2_backward(p, null, 1, 4, 6, 6, p, null) == -1 and lib.kp2d_maxpool2_backward(p, p, 0, 4, 6, 6, p, null) == -1
    assert lib.kp2d_shuffle_cat_forward(p, null, 1, 4, 3, 3, 5, p, null) == -1 and lib.kp2d_shuffle_cat_forward(p, p, 1, 0, 3, 3, 5, p, null) == -1
    assert lib.kp2d_shuffle_cat_backward(null, 1, 4, 3, 3, 5, p, null) == -1 and lib.kp2d_shuffle_cat_backward(p, 1, 4, -1, 3, 5, p, null) == -1
    torch.cuda.synchronize()
    assert not buf.any()
