"""The float64 oracle of the depth head's training step (depth_training_ref) against the fixtures written from the reference's
SegmentationHead, SILogLoss and torch.nn.HuberLoss (to 1e-10 on every stored entry) and against central finite differences;
the stated deviations of the loss; the argument checks of the Python layer; the new signatures against the header: everything
here runs without a device."""
import os
import re

import numpy as np
import pytest
import torch

import depth_training_ref as dr
from conftest import ROOT
from nano_vs_slam_amd import _lib, depth_training as dt, seg_training as st


@pytest.mark.parametrize("name", list(dr.LOSS_CASES))
def test_loss_oracle_equals_the_reference_fixture(name):
    z, gt = dr.make_loss_inputs(name)
    fx = dr.load_fixture(name)
    s = dr.depth_loss(z, gt)
    assert int(fx["max_stored"]) == dr.MAX_STORED and int(fx["seed"]) == dr.seed_of(name) and fx["dlogits"].size <= dr.MAX_STORED
    worst = max(np.abs(dr.stored(s["dz"]) - fx["dlogits"]).max(), abs(s["loss"] - float(fx["loss"])), abs(s["silog"] - float(fx["silog"])),
                abs(s["huber"] - float(fx["huber"])))
    print(f"case {name}: oracle vs fixture max|diff| {worst:.2e}")
    assert worst <= 1e-10
    assert s["valid"] == int(fx["valid"]) and s["stray"] == 0


@pytest.fixture(scope="module")
def steps():
    out = {}
    for name in dr.STEP_CASES:
        inp = dr.make_inputs(name)
        out[name] = (inp, dr.step_gradients(inp))
    return out


@pytest.mark.parametrize("name", list(dr.STEP_CASES))
def test_step_oracle_equals_the_reference_fixture(steps, name):
    inp, s = steps[name]
    fx = dr.load_fixture(name)
    assert int(fx["max_stored"]) == dr.MAX_STORED and int(fx["seed"]) == dr.seed_of(name)
    worst = 0.0
    for k in dr.MAPS + dr.DMAPS:
        assert fx[k].size <= dr.MAX_STORED
        worst = max(worst, np.abs(dr.stored(s[k]) - fx[k]).max())
    for i, g in enumerate(s["grads"]):
        assert np.asarray(g).size == inp["params"][i].size
        worst = max(worst, np.abs(dr.stored(g) - fx[f"g{i}"]).max())
    worst = max(worst, abs(s["loss"] - float(fx["loss"])), abs(s["silog"] - float(fx["silog"])), abs(s["huber"] - float(fx["huber"])))
    print(f"case {name}: oracle vs fixture max|diff| {worst:.2e}")
    assert worst <= 1e-10
    assert s["valid"] == int(fx["valid"]) and s["stray"] == 0


def test_cases_are_what_they_are_for(steps):
    for name in dr.LOSS_CASES:
        z, gt = dr.make_loss_inputs(name)
        s = dr.depth_loss(z, gt)
        assert np.abs(z).max() <= (20.01 if name == "L4" else dr.Z_MAX) and s["Dg"] >= 1e-3
        linear = (np.abs(s["d"][s["ok"]]) >= 1).mean()
        assert name == "L4" or 0.1 <= linear <= 0.9
    z, gt = dr.make_loss_inputs("L3")
    assert (gt[1] <= 0).all() and (gt[3] > 0).sum() == 1 and z.size > 10 * 1024
    assert not dr.depth_loss(z, gt)["dz"][1].any()
    z, gt = dr.make_loss_inputs("L4")
    g = dr.depth_loss(z, gt)
    gv = g["g"][g["ok"]]
    assert gv.mean() ** 2 / gv.var() > 1e8                  # a variance from raw fp32 moments has no digit left here
    for name, (N, c_in, c_hidden, d1, c_skip, h, w) in dr.STEP_CASES.items():
        inp, s = steps[name]
        assert s["logits"].shape == (N, 1, 2 * h, 2 * w) and np.abs(s["logits"]).max() <= dr.Z_MAX
        assert 0.1 <= (inp["gt"] <= 0).mean() <= 0.4
        linear = (np.abs(s["d"][inp["gt"] > 0]) >= 1).mean()
        assert 0.1 <= linear <= 0.9
    assert steps["B"][1]["pooled"].shape[2:] == (1, 1)
    assert {dr.STEP_CASES[n][1:5] for n in dr.STEP_CASES} == {c[1:5] for c in dr.sr.CASES.values()}


def test_oracle_against_finite_differences():
    """Central differences of the float64 loss: eight logits of L2 and of L4, and on case A three entries of every parameter.
    |fd - g| <= 1e-6 max|g| + 1e-10: truncation h^2 = 1e-10, rounding 1e-16 / h = 1e-11 (times the loss's size)."""
    rng = np.random.default_rng(11)
    h = 1e-5
    worst = 0.0
    for name in ("L2", "L4"):
        z, gt = dr.make_loss_inputs(name)
        z = z.astype(np.float64)
        s = dr.depth_loss(z, gt)
        valid = np.argwhere(s["ok"])
        for idx in valid[rng.integers(0, len(valid), 8)]:
            idx = tuple(idx)
            keep = z[idx]
            z[idx] = keep + h
            up = dr.depth_loss(z, gt)["loss"]
            z[idx] = keep - h
            dn = dr.depth_loss(z, gt)["loss"]
            z[idx] = keep
            err = abs((up - dn) / (2 * h) - s["dz"][idx]) / (1e-6 * np.abs(s["dz"]).max() + 1e-9)
            worst = max(worst, err)
            assert err <= 1.0, (name, idx, (up - dn) / (2 * h), s["dz"][idx])
    inp = dr.make_inputs("A")
    params = [p.astype(np.float64) for p in inp["params"]]
    s = dr.step_gradients(inp, params)
    for i, g in enumerate(s["grads"]):
        g = np.asarray(g).reshape(params[i].shape)
        for _ in range(3):
            idx = tuple(int(rng.integers(0, n)) for n in g.shape)
            keep = params[i][idx]
            params[i][idx] = keep + h
            up = dr.loss_from(inp, params)
            params[i][idx] = keep - h
            dn = dr.loss_from(inp, params)
            params[i][idx] = keep
            err = abs((up - dn) / (2 * h) - g[idx]) / (1e-6 * np.abs(g).max() + 1e-9)
            worst = max(worst, err)
            assert err <= 1.0, (dr.PARAMS[i], idx, (up - dn) / (2 * h), g[idx])
    print(f"finite differences: {worst:.3f} of the bound")


def test_loss_deviations_of_the_oracle():
    z, gt = dr.make_loss_inputs("L2")
    none = dr.depth_loss(z, np.zeros_like(gt))
    assert none["loss"] == 0.0 and none["valid"] == 0 and not none["dz"].any()
    one = np.zeros_like(gt)
    one[1, 4, 7] = 2.5
    s = dr.depth_loss(z, one)                                      # M = 1: Huber alone
    p = 1.0 / (1.0 + np.exp(-float(z[1, 4, 7])))
    assert s["valid"] == 1 and s["silog"] == 0.0 and abs(s["loss"] - ((2.5 - p) - 0.5)) <= 1e-15
    assert np.count_nonzero(s["dz"]) == 1 and abs(s["dz"][1, 4, 7] + p * (1 - p)) <= 1e-15
    flat = dr.depth_loss(np.zeros((2, 5, 7)), np.full((2, 5, 7), 0.5))      # Dg = 0: g = 0 at every pixel, and d = 0
    assert flat["Dg"] == 0.0 and flat["loss"] == 0.0 and not flat["dz"].any() and flat["valid"] == 70
    bad_gt, bad_z, base = gt.copy(), z.copy(), gt.copy()
    where = np.argwhere(gt > 0)[[0, 9, 33]]
    for i, v in zip(where, (np.nan, np.inf, -np.inf)):
        bad_gt[tuple(i)] = v
        base[tuple(i)] = 0.0
    bad_z[tuple(where[0])] = np.nan
    a, b, c = dr.depth_loss(z, bad_gt), dr.depth_loss(z, base), dr.depth_loss(bad_z, base)
    assert a["stray"] == 3 and b["stray"] == 0 and c["stray"] == 1 and a["valid"] == b["valid"] == c["valid"]
    assert a["loss"] == b["loss"] == c["loss"] and np.array_equal(a["dz"], b["dz"]) and np.array_equal(c["dz"], b["dz"])
    for big in (30.0, 200.0):                                      # saturation: finite where torch's log(sigmoid(z)) is not
        zz = np.where(np.arange(z.size).reshape(z.shape) % 2, big, -big)
        s = dr.depth_loss(zz, gt)
        assert np.isfinite(s["loss"]) and np.isfinite(s["dz"]).all() and s["loss"] > 10


def test_bounds_come_from_the_fixtures():
    b = dr.bounds()
    names = list(dr.LOSS_CASES) + list(dr.STEP_CASES)
    assert set(b) == set(dr.STEP_KEYS)
    for k, v in b.items():
        fx = [dr.load_fixture(n) for n in names]
        assert v == max(8.0 * max(float(f["err32_" + k]) for f in fx if "err32_" + k in f.files), dr.FLOOR)
        assert dr.FLOOR <= v < 1e-4, k                               # far below a missing term's 1e-2
    for k in dr.LOSS_KEYS:
        assert all("err32_" + k in dr.load_fixture(n).files for n in names)
    tb = dr.trajectory_bounds()
    assert set(tb) == {"loss_head", "loss_last", "p24_last", "p25_last"} | {f"p{i}_head" for i in range(26)}
    assert all(dr.FLOOR <= v < 1e-4 for v in tb.values())
    for n in names:                                                  # the recorded gaps: no branch flips between float32 and float64
        f = dr.load_fixture(n)
        assert float(f["huber_gap"]) > 100 * float(f["err32_d"])
        assert n in dr.LOSS_CASES or float(f["pre_gap"]) > 100 * float(f["err32_pre"])


def test_trajectory_falls():
    inp = dr.make_inputs(dr.TRAJECTORY_CASE)
    fx = dr.load_trajectory()
    for mode, trained in (("head", list(range(26))), ("last", [24, 25])):
        losses, after = dr.trajectory(inp, mode)
        assert np.abs(losses - fx[f"losses_{mode}"]).max() <= 1e-10
        assert (losses[1:] < losses[:-1]).all()
        for t, ps in enumerate(after):
            for i, p in zip(trained, ps):
                assert np.abs(dr.stored(p, dr.TRAJ_STORED) - fx[f"p{i}_{mode}"][t]).max() <= 1e-10, (mode, t, dr.PARAMS[i])


# ---- argument checks: nothing below may reach the library -------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(st._lib, "load", boom)


@pytest.fixture
def shapes_only(no_library, monkeypatch):
    monkeypatch.setattr("nano_vs_slam_amd.train_ops._is_device", lambda t: True)     # shapes, on a box without a device


def _depth_model(config="S", **kw):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import KP2DTinyV2, get_config
    return KP2DTinyV2(**get_config(config, **kw), nClasses=19, depth=True)


def test_depth_loss_refusals(shapes_only):
    z, gt = torch.zeros(2, 1, 4, 6), torch.zeros(2, 4, 6)
    for bad in ((z.double(), gt), (z, gt.double()), (z, gt.long()), (z, torch.zeros(2, 4, 5)), (z, torch.zeros(2, 8, 12)),
                (torch.zeros(2, 2, 4, 6), gt), (torch.zeros(4, 6), torch.zeros(4, 6)), (z[:0], gt[:0]), (z, None)):
        with pytest.raises(ValueError):
            dt.depth_loss(*bad)
    for kw in ({"silog_weight": -1.0}, {"huber_weight": float("inf")}, {"silog_weight": float("nan")}):
        with pytest.raises(ValueError, match="weights"):
            dt.depth_loss(z, gt, **kw)


def test_cpu_tensors_raise(no_library):
    with pytest.raises(ValueError, match="no CPU path"):
        dt.depth_loss(torch.zeros(2, 1, 4, 6), torch.zeros(2, 4, 6))
    trainer = dt.DepthHeadTrainer(_depth_model())
    with pytest.raises(ValueError, match="no CPU path"):
        trainer.step_features(torch.zeros(2, 64, 4, 6), torch.zeros(2, 64, 8, 12), torch.zeros(2, 8, 12))
    with pytest.raises(ValueError, match="no CPU path"):
        trainer.forward_features(torch.zeros(2, 64, 4, 6), torch.zeros(2, 64, 8, 12))
    with pytest.raises(ValueError, match="no CPU path"):
        trainer.step(torch.zeros(1, 3, 32, 32), torch.zeros(1, 16, 16))


def test_trainer_refusals(shapes_only):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import KP2DTinyV3, get_config, tiny_factory
    with pytest.raises(ValueError, match="DepthHeadTrainer: the model was built without depth=True"):
        dt.DepthHeadTrainer(tiny_factory("S", 28))
    for train in ("head", "last"):
        with pytest.raises(ValueError, match="DepthHeadTrainer: V3"):
            dt.DepthHeadTrainer(KP2DTinyV3(**get_config("S", v3=True), nClasses=19, depth=True), train=train)
        with pytest.raises(ValueError, match="DepthHeadTrainer: .*convtranspose"):
            dt.DepthHeadTrainer(_depth_model(to_mcu=True), train=train)
    with pytest.raises(ValueError, match="DepthHeadTrainer: .*attention"):
        dt.DepthHeadTrainer(_depth_model("S_A"), train="head")
    with pytest.raises(ValueError, match="DepthHeadTrainer: .*channel counts"):
        dt.DepthHeadTrainer(_depth_model("N"), train="head")            # the 72-channel concatenation
    with pytest.raises(ValueError, match="train must be"):
        dt.DepthHeadTrainer(_depth_model(), train="seg")
    model = _depth_model()
    for kw in ({"lr": -1.0}, {"betas": (1.0, 0.999)}, {"eps": -1e-8}, {"silog_weight": -0.5}, {"huber_weight": float("nan")}):
        with pytest.raises(ValueError):
            dt.DepthHeadTrainer(model, **kw)
    assert len(dt.DepthHeadTrainer(_depth_model("N"), train="last").parameters()) == 2
    attention = _depth_model("S_A")
    last = dt.DepthHeadTrainer(attention, train="last")                 # the attention head's last layer
    assert [id(p) for p in last.parameters()] == [id(attention.depth_head.convs[-1].weight), id(attention.depth_head.convs[-1].bias)]

    trainer = dt.DepthHeadTrainer(model)
    named = dict(model.depth_head.named_parameters())               # every parameter of the head, in registration order
    assert [id(p) for p in trainer.parameters()] == [id(named[n]) for n in dr.PARAMS] and len(named) == 26
    assert named["convs.8.weight"].shape == (1, 64, 3, 3)
    x, skip, gt = torch.zeros(2, 64, 4, 6), torch.zeros(2, 64, 8, 12), torch.zeros(2, 8, 12)
    with pytest.raises(ValueError, match="DepthHeadTrainer: .*even"):
        trainer.step_features(torch.zeros(2, 64, 5, 6), torch.zeros(2, 64, 10, 12), torch.zeros(2, 10, 12))
    with pytest.raises(ValueError, match="even"):
        trainer.forward_features(torch.zeros(2, 64, 4, 7), torch.zeros(2, 64, 8, 14))
    with pytest.raises(ValueError, match="logits' size"):
        trainer.step_features(x, skip, torch.zeros(2, 4, 6))                                     # gt at the backbone's size
    with pytest.raises(ValueError, match="logits' size"):
        trainer.step_features(x, skip, torch.zeros(2, 2, 8, 12))
    for bad in (gt.double(), gt.to(torch.uint8), gt.half()):
        with pytest.raises(ValueError, match="float32"):
            trainer.step_features(x, skip, bad)
    with pytest.raises(ValueError):
        trainer.step_features(x, torch.zeros(2, 32, 8, 12), gt)
    with pytest.raises(ValueError):
        trainer.step_features(x, None, gt)
    last = dt.DepthHeadTrainer(model, train="last")
    with pytest.raises(ValueError):
        last.step_features(x, skip, gt)                             # "last" mode takes the last layer's input alone
    with pytest.raises(ValueError, match="logits' size"):
        last.step_features(torch.zeros(2, 64, 8, 12), None, torch.zeros(2, 4, 6))
    w = model.depth_head.convs[8].weight
    w.data = w.data.permute(0, 1, 3, 2)                             # a non-contiguous parameter
    assert not w.is_contiguous()
    with pytest.raises(ValueError, match="DepthHeadTrainer: .*contiguous"):
        trainer.step_features(x, skip, gt)
    with pytest.raises(ValueError, match="contiguous"):
        last.step_features(torch.zeros(2, 64, 8, 12), None, gt[:, None])


def test_seg_trainer_on_a_depth_model_still_trains_seg_head():
    model = _depth_model()
    seg, depth = st.SegHeadTrainer(model), dt.DepthHeadTrainer(model)
    assert seg.convs[-1] is model.seg_head.convs[8] and depth.convs[-1] is model.depth_head.convs[8]
    assert not {id(p) for p in seg.parameters()} & {id(p) for p in depth.parameters()}       # the two heads share no parameter
    assert isinstance(seg, st._DenseHeadTrainer) and isinstance(depth, st._DenseHeadTrainer)
    assert type(seg).gradients is type(depth).gradients is st._DenseHeadTrainer.gradients   # one walk for both


# ---- the new signatures against the header ------------------------------------------------------------------------------------
NEW = ("kp2d_depth_loss_scratch_bytes", "kp2d_depth_loss")


def test_new_signatures_agree_with_the_header():
    import ctypes as C
    with open(os.path.join(ROOT, "include", "kp2d.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "size_t": C.c_size_t}
    for name in NEW:
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        assert res is kinds[m.group(1)], name
        decl = [a.strip() for a in m.group(2).split(",")]
        assert len(decl) == len(args), (name, len(decl), len(args))
        for d, a in zip(decl, args):
            if "*" in d:
                assert a is C.c_void_p, (name, d)
            else:
                assert a is kinds[d.split()[-2]], (name, d)
    for const, value in (("KP2D_SILOG_SCALE", dr.SILOG_SCALE), ("KP2D_SILOG_LAMBDA", dr.SILOG_LAMBDA), ("KP2D_HUBER_DELTA", dr.HUBER_DELTA)):
        assert float(re.search(r"#define\s+" + const + r"\s+(\S+)", raw).group(1)) == value
