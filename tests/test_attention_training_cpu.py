"""The float64 oracle of the attention head's training step (attention_training_ref) against the fixtures written from the
reference's SegFormerAttentionModule and SegmentationHeadATT (to 1e-10 on every stored entry) and against central finite
differences; the registration order; every refusal of the stage calls and of the two trainers; that the old trainers still
refuse; the new signatures against the header: everything here runs without a device."""
import os
import re

import numpy as np
import pytest
import torch

import attention_training_ref as ar
from conftest import ROOT
from nano_vs_slam_amd import _lib, attention_training as at, depth_training as dt, seg_training as st, train_ops as ops


@pytest.fixture(scope="module")
def module_steps():
    return {name: (inp, ar.module_step(inp)) for name, inp in ((n, ar.make_module_inputs(n)) for n in ar.MODULE_CASES)}


@pytest.fixture(scope="module")
def head_steps():
    return {name: (inp, ar.head_step(inp)) for name, inp in ((n, ar.make_head_inputs(n)) for n in ar.HEAD_CASES)}


@pytest.mark.parametrize("name", list(ar.MODULE_CASES))
def test_module_oracle_equals_the_reference_fixture(module_steps, name):
    inp, s = module_steps[name]
    fx = ar.load_fixture(name)
    assert int(fx["max_stored"]) == ar.sr.MAX_STORED and int(fx["seed"]) == ar.seed_of(name)
    worst = 0.0
    for k in ar.MODULE_MAPS + ar.MODULE_DMAPS:
        assert fx[k].size <= ar.sr.MAX_STORED
        worst = max(worst, np.abs(ar.stored(s[k]) - fx[k]).max())
    for i, g in enumerate(s["grads"]):
        assert np.asarray(g).shape == inp["params"][i].shape
        worst = max(worst, np.abs(ar.stored(g) - fx[f"g{i}"]).max())
    print(f"case {name}: oracle vs fixture max|diff| {worst:.2e}")
    assert worst <= 1e-10
    assert float(fx["min_s"]) > ar.MIN_S        # no pinned LayerNorm pixel is near sqrt(var) = 0


@pytest.mark.parametrize("name", list(ar.HEAD_CASES))
def test_head_oracle_equals_the_reference_fixture(head_steps, name):
    inp, s = head_steps[name]
    fx = ar.load_fixture(name)
    assert int(fx["seed"]) == ar.seed_of(name) and len(s["grads"]) == 47 == len(ar.HEAD_PARAMS)
    worst = abs(s["loss"] - float(fx["loss"]))
    for k in ar.HEAD_MAPS + ("dlogits",):
        worst = max(worst, np.abs(ar.stored(s[k]) - fx[k]).max())
    for i, g in enumerate(s["grads"]):
        assert np.asarray(g).size == inp["params"][i].size
        worst = max(worst, np.abs(ar.stored(g) - fx[f"g{i}"]).max())
    print(f"case {name}: oracle vs fixture max|diff| {worst:.2e}")
    assert worst <= 1e-10
    assert s["min_s"] > ar.MIN_S and float(fx["min_s"]) > ar.MIN_S


@pytest.mark.parametrize("name", ["seg", "depth", "pair"])
def test_trajectory_oracle_equals_the_reference_fixture(name):
    fx = ar.load_trajectory(name)
    if name == "pair":
        inp = ar.make_pair_inputs()
        assert aug_margin(inp) > ar.NEAREST_SAFE
        losses, after = ar.trajectory(inp, ar.PAIR_STEPS, step_fn=ar.pair_step)
    else:
        losses, after = ar.trajectory(ar.make_head_inputs(name))
    assert losses.shape == (ar.PAIR_STEPS if name == "pair" else ar.TRAJECTORY_STEPS,) and float(fx["lr"]) == ar.LR
    worst = np.abs(losses - fx["losses"]).max()
    for i in range(47):
        worst = max(worst, max(np.abs(ar.stored(a[i], ar.TRAJ_STORED) - fx[f"p{i}"][t]).max() for t, a in enumerate(after)))
    print(f"trajectory {name}: oracle vs fixture max|diff| {worst:.2e}; losses {losses}")
    assert worst <= 1e-10 and losses[-1] < losses[0]


def aug_margin(inp):
    import depth_pair_ref as pr
    return pr.nearest_margin(inp["homography"], 2 * inp["h"], 2 * inp["w"])


def test_cases_are_what_they_are_for(module_steps, head_steps):
    S = lambda n: ar.MODULE_CASES[n][2] * ar.MODULE_CASES[n][3]
    T = lambda n: (ar.MODULE_CASES[n][2] // 2) * (ar.MODULE_CASES[n][3] // 2)
    assert (S("A"), T("A")) == (24, 6) and (S("B"), T("B")) == (300, 70) and (S("C"), T("C")) == (468, 117)
    assert (S("D"), T("D")) == (4, 1) and (S("E"), T("E")) == (1700, 425)
    assert ar.MODULE_CASES["B"][2] % 2 == 1 and ar.MODULE_CASES["C"][1] // ar.HEADS == 12 and S("E") % 16 and T("E") % 16
    inp, s = module_steps["B"]      # the dropped line: no key reads the last row, the key/value branch sends nothing back to it
    _, _ = ar.patch2_backward(s["n1"], inp["params"][1], s["d_kv"])
    assert not ar.patch2_backward(s["n1"], inp["params"][1], s["d_kv"])[0][:, :, -1].any()
    inp, s = module_steps["D"]      # one key: the softmax is 1, dQ = dK = 0 exactly, dV = the sum of dO over the queries
    C = inp["C"]
    assert not s["d_q"].any() and not s["d_kv"][:, :C].any() and not np.asarray(s["grads"][0]).any()
    assert np.abs(s["d_kv"][:, C:, 0, 0] - s["d_o"].sum(axis=(2, 3))).max() <= 1e-12
    assert head_steps["odd"][1]["pooled"].shape[2:] == (5, 7)
    assert head_steps["depth"][1]["logits"].shape[1] == 1 and head_steps["seg"][1]["logits"].shape == (2, 28, 16, 24)


# ---- central finite differences -------------------------------------------------------------------------------------------------
def _fd(f, a, idx, h=1e-6):
    keep = a[idx]
    a[idx] = keep + h
    up = f()
    a[idx] = keep - h
    down = f()
    a[idx] = keep
    return (up - down) / (2 * h)


def test_layernorm_dx_formula_against_finite_differences_and_autograd():
    rng = np.random.default_rng(5)
    x, g, b, dy = rng.standard_normal((2, 48, 3, 4)), rng.uniform(0.5, 1.5, 48), rng.standard_normal(48), rng.standard_normal((2, 48, 3, 4))
    dx, dg, db = ar.layernorm_backward(x, g, dy)
    loss = lambda: float((ar.layernorm(x, g, b)[0] * dy).sum())
    for idx in ((0, 0, 0, 0), (1, 47, 2, 3), (0, 13, 1, 2)):
        assert abs(_fd(loss, x, idx) - dx[idx]) <= 1e-7
    for c in (0, 20, 47):
        assert abs(_fd(loss, g, c) - dg[c]) <= 1e-7 and abs(_fd(loss, b, c) - db[c]) <= 1e-7
    xt = torch.from_numpy(x).requires_grad_(True)       # the reference's own expression under autograd
    gt, bt = torch.from_numpy(g).view(1, -1, 1, 1), torch.from_numpy(b).view(1, -1, 1, 1)
    y = (xt - xt.mean(dim=1, keepdim=True)) / (torch.var(xt, dim=1, unbiased=False, keepdim=True).sqrt() + ar.LN_EPS) * gt + bt
    y.backward(torch.from_numpy(dy))
    assert np.abs(xt.grad.numpy() - dx).max() <= 1e-12
    flat = np.ones((1, 48, 1, 2))                       # a pixel with constant channels: the stated rule, finite where torch is NaN
    flat[0, :, 0, 1] = rng.standard_normal(48)
    d = ar.layernorm_backward(flat, g, np.ones((1, 48, 1, 2)))[0]
    assert np.isfinite(d).all() and np.abs(d[0, :, 0, 0] - (g - g.mean()) / ar.LN_EPS).max() <= 1e-6 * np.abs(g / ar.LN_EPS).max()


def test_module_against_finite_differences():
    inp = ar.make_module_inputs("A")
    p = [a.astype(np.float64) for a in inp["params"]]
    x = inp["x"].astype(np.float64)
    s = ar.module_forward(x, p)
    d, g = ar.module_backward(s, p, inp["dy"])
    loss = lambda: float((ar.module_forward(x, p)["y"] * inp["dy"]).sum())
    rng = np.random.default_rng(6)
    scale = max(np.abs(np.asarray(t)).max() for t in g)
    for i, a in enumerate(p):
        for _ in range(2):
            idx = tuple(int(rng.integers(0, n)) for n in a.shape)
            assert abs(_fd(loss, a, idx) - np.asarray(g[i]).reshape(a.shape)[idx]) <= 2e-7 * scale, (ar.MODULE_PARAMS[i], idx)
    for _ in range(4):
        idx = tuple(int(rng.integers(0, n)) for n in x.shape)
        assert abs(_fd(loss, x, idx) - d["dx"][idx]) <= 2e-7 * np.abs(d["dx"]).max()


# ---- registration order and refusals ----------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", boom)


@pytest.fixture
def shapes_only(no_library, monkeypatch):
    monkeypatch.setattr("nano_vs_slam_amd.train_ops._is_device", lambda t: True)     # shapes, on a box without a device


def _depth_model(config="S_A", **kw):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import KP2DTinyV2, get_config
    return KP2DTinyV2(**get_config(config, **kw), nClasses=19, depth=True)


def test_registration_order():
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    model = tiny_factory("S_A", 28)
    trainer = at.AttentionSegHeadTrainer(model)
    named = dict(model.seg_head.named_parameters())
    assert list(named) == list(ar.HEAD_PARAMS) and len(named) == 47
    assert [id(p) for p in trainer.parameters()] == [id(named[n]) for n in ar.HEAD_PARAMS]
    module = model.seg_head.convs[1]
    assert [id(p) for p in ops.attention_module_parameters(module)] == [id(p) for p in module.parameters()]
    assert [n for n, _ in module.named_parameters()] == list(ar.MODULE_PARAMS)
    last = at.AttentionSegHeadTrainer(model, train="last")
    assert [id(p) for p in last.parameters()] == [id(model.seg_head.convs[7].weight), id(model.seg_head.convs[7].bias)]
    depth = _depth_model()
    dtr = at.AttentionDepthHeadTrainer(depth)
    assert [id(p) for p in dtr.parameters()] == [id(p) for p in depth.depth_head.parameters()] and len(dtr.parameters()) == 47
    assert at.AttentionSegHeadTrainer(depth).convs[-1] is depth.seg_head.convs[7]        # never the depth head


def test_trainer_refusals(shapes_only):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import KP2DTinyV2, get_config, tiny_factory
    with pytest.raises(ValueError, match="no attention head.*SegHeadTrainer"):
        at.AttentionSegHeadTrainer(tiny_factory("S", 28))
    with pytest.raises(ValueError, match="no attention head.*DepthHeadTrainer"):
        at.AttentionDepthHeadTrainer(KP2DTinyV2(**get_config("S"), nClasses=19, depth=True))
    with pytest.raises(ValueError, match="V3"):
        at.AttentionSegHeadTrainer(tiny_factory("S_A", 28, v3=True))
    with pytest.raises(ValueError, match="convtranspose"):
        at.AttentionSegHeadTrainer(tiny_factory("S_A", 28, to_mcu=True))
    with pytest.raises(ValueError, match="channel counts"):
        at.AttentionSegHeadTrainer(tiny_factory("N_A", 28))             # the 72-channel concatenation
    with pytest.raises(ValueError, match="no depth_head"):
        at.AttentionDepthHeadTrainer(tiny_factory("S_A", 28))
    with pytest.raises(ValueError, match="train must be"):
        at.AttentionSegHeadTrainer(tiny_factory("S_A", 28), train="module")
    assert len(at.AttentionSegHeadTrainer(tiny_factory("N_A", 28), train="last").parameters()) == 2
    model = tiny_factory("S_A", 28)
    for kw in ({"lr": -1.0}, {"betas": (1.0, 0.999)}, {"ce_weight": -0.5}):
        with pytest.raises(ValueError):
            at.AttentionSegHeadTrainer(model, **kw)
    trainer = at.AttentionSegHeadTrainer(model)
    x, skip, lab = torch.zeros(2, 64, 4, 6), torch.zeros(2, 64, 8, 12), torch.zeros(2, 8, 12, dtype=torch.uint8)
    with pytest.raises(ValueError, match="even"):
        trainer.step_features(torch.zeros(2, 64, 5, 6), torch.zeros(2, 64, 10, 12), torch.zeros(2, 10, 12, dtype=torch.uint8))
    with pytest.raises(ValueError, match="at least 4 x 4"):
        trainer.step_features(torch.zeros(2, 64, 2, 6), torch.zeros(2, 64, 4, 12), torch.zeros(2, 4, 12, dtype=torch.uint8))
    with pytest.raises(ValueError, match="at least 4 x 4"):
        trainer.forward_features(torch.zeros(2, 64, 4, 2), torch.zeros(2, 64, 8, 4))
    with pytest.raises(ValueError, match="logits' size"):
        trainer.step_features(x, skip, torch.zeros(2, 4, 6, dtype=torch.uint8))
    with pytest.raises(ValueError):
        trainer.step_features(x, torch.zeros(2, 32, 8, 12), lab)
    with pytest.raises(ValueError):
        trainer.step_features(x, None, lab)
    w = model.seg_head.convs[1].att.fn.to_kv.weight
    w.data = w.data.permute(0, 1, 3, 2)                 # a non-contiguous parameter of a module
    assert not w.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        trainer.step_features(x, skip, lab)


def test_trainers_refuse_cpu_tensors(no_library):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    trainer = at.AttentionSegHeadTrainer(tiny_factory("S_A", 19))
    with pytest.raises(ValueError, match="no CPU path"):
        trainer.step_features(torch.zeros(2, 64, 4, 6), torch.zeros(2, 64, 8, 12), torch.zeros(2, 8, 12, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no CPU path"):
        trainer.forward_features(torch.zeros(2, 64, 4, 6), torch.zeros(2, 64, 8, 12))
    with pytest.raises(ValueError, match="no CPU path"):
        trainer.step(torch.zeros(1, 3, 32, 32), torch.zeros(1, 16, 16, dtype=torch.uint8))
    dtr = at.AttentionDepthHeadTrainer(_depth_model())
    with pytest.raises(ValueError, match="no CPU path"):
        dtr.step_features(torch.zeros(2, 64, 4, 6), torch.zeros(2, 64, 8, 12), torch.zeros(2, 8, 12))


def test_the_old_trainers_still_refuse():
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    with pytest.raises(ValueError, match="SegHeadTrainer: train='head' on an attention head is not supported.*AttentionSegHeadTrainer"):
        st.SegHeadTrainer(tiny_factory("S_A", 28), train="head")
    with pytest.raises(ValueError, match="DepthHeadTrainer: train='head' on an attention head.*AttentionDepthHeadTrainer"):
        dt.DepthHeadTrainer(_depth_model(), train="head")
    assert len(st.SegHeadTrainer(tiny_factory("S_A", 28), train="last").parameters()) == 2
    assert len(st.SegHeadTrainer(tiny_factory("S", 28)).parameters()) == 26


def _stage_calls():
    x, h = torch.zeros(2, 64, 5, 6), torch.zeros(2, 128, 5, 6)
    g, kv = torch.zeros(1, 64, 1, 1), torch.zeros(2, 128, 2, 3)
    w1, wkv, wd = torch.zeros(128, 64, 1, 1), torch.zeros(128, 64, 2, 2), torch.zeros(128, 1, 3, 3)
    m, lse = torch.zeros(2, 5, 6), torch.zeros(2, 2, 4, 30)
    return {
        "layernorm_forward": lambda **k: ops.layernorm_forward(k.get("x", x), k.get("g", g), g),
        "layernorm_backward": lambda **k: ops.layernorm_backward(k.get("x", x), g, k.get("m", m), m, k.get("dy", x)),
        "pointwise_forward": lambda **k: ops.pointwise_forward(k.get("x", x), k.get("w", w1), k.get("b", torch.zeros(128))),
        "pointwise_backward": lambda **k: ops.pointwise_backward(k.get("x", x), k.get("w", w1), k.get("dy", h), pre=k.get("pre")),
        "patch2_forward": lambda **k: ops.patch2_forward(k.get("x", x), k.get("w", wkv)),
        "patch2_backward": lambda **k: ops.patch2_backward(k.get("x", x), wkv, k.get("dy", kv)),
        "dwconv3_forward": lambda **k: ops.dwconv3_forward(k.get("x", h), k.get("w", wd), torch.zeros(128)),
        "dwconv3_backward": lambda **k: ops.dwconv3_backward(k.get("x", h), wd, k.get("dy", h)),
        "attention_forward": lambda **k: ops.attention_forward(k.get("x", x), k.get("kv", kv)),
        "attention_backward": lambda **k: ops.attention_backward(k.get("x", x), k.get("kv", kv), x, k.get("lse", lse), k.get("dy", x)),
    }


def test_stage_calls_refuse_cpu_tensors(no_library):
    for name, call in _stage_calls().items():
        with pytest.raises(ValueError, match="no CPU path"):
            call()


def test_stage_calls_refuse_bad_arguments(shapes_only):
    calls = _stage_calls()
    for name, call in calls.items():
        wide = name.startswith("dwconv3")
        good = torch.zeros(2, 128 if wide else 64, 5, 6)
        for bad in (good.double(), good[0], torch.zeros(2, 40, 5, 6), good.permute(0, 1, 3, 2)):       # dtype, rank, channels, layout
            with pytest.raises(ValueError):
                call(x=bad)
        with pytest.raises(AssertionError, match="the library was reached"):      # and the good arguments pass every check
            call()
    for name in ("layernorm_backward", "pointwise_backward", "patch2_backward", "dwconv3_backward", "attention_backward"):
        with pytest.raises(ValueError):
            calls[name](dy=torch.zeros(2, 64, 4, 6))
    with pytest.raises(ValueError):
        calls["layernorm_forward"](g=torch.zeros(48))
    with pytest.raises(ValueError):
        calls["layernorm_backward"](m=torch.zeros(2, 5, 5))
    with pytest.raises(ValueError):
        calls["pointwise_forward"](w=torch.zeros(128, 48, 1, 1))
    with pytest.raises(ValueError):
        calls["pointwise_forward"](w=torch.zeros(100, 64, 1, 1))
    with pytest.raises(ValueError):
        calls["pointwise_forward"](b=torch.zeros(64))
    with pytest.raises(ValueError):
        calls["pointwise_backward"](pre=torch.zeros(2, 128, 5, 5))
    with pytest.raises(ValueError):
        calls["patch2_forward"](w=torch.zeros(128, 64, 3, 3))
    with pytest.raises(ValueError):
        calls["patch2_forward"](x=torch.zeros(2, 64, 1, 6))                # no 2 x 2 patch
    with pytest.raises(ValueError):
        calls["attention_forward"](kv=torch.zeros(2, 128, 3, 3))
    with pytest.raises(ValueError):
        calls["attention_forward"](x=torch.zeros(2, 128, 5, 6), kv=torch.zeros(2, 256, 2, 3))       # head dimension 32
    with pytest.raises(ValueError):
        calls["attention_backward"](lse=torch.zeros(2, 4, 30))
    with pytest.raises(ValueError):
        calls["dwconv3_forward"](w=torch.zeros(128, 1, 1, 3))


# ---- the new signatures against the header ------------------------------------------------------------------------------------
NEW = ("kp2d_att_train_scratch_bytes", "kp2d_layernorm_forward_train", "kp2d_layernorm_backward", "kp2d_pointwise_forward_train",
       "kp2d_gelu_backward", "kp2d_pointwise_backward", "kp2d_patch2_forward_train", "kp2d_patch2_backward", "kp2d_dwconv3_forward_train",
       "kp2d_dwconv3_backward", "kp2d_attention_forward_train", "kp2d_attention_backward")


def test_new_signatures_agree_with_the_header():
    import ctypes as C
    with open(os.path.join(ROOT, "include", "kp2d.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
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
