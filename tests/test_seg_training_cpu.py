"""The float64 oracle of the segmentation head's training step (seg_training_ref) against the fixtures written from the
reference's SegmentationHead (to 1e-10 on every stored entry), against central finite differences and against a plain torch
restatement of the Dice loss; the argument checks of the Python layer; the new signatures against the header: everything
here runs without a device."""
import os
import re

import numpy as np
import pytest
import torch

import seg_training_ref as sr
from conftest import ROOT
from nano_vs_slam_amd import _lib, seg_training as st


@pytest.fixture(scope="module")
def steps():
    out = {}
    for name in sr.CASES:
        inp = sr.make_inputs(name)
        out[name] = (inp, sr.step_gradients(inp))
    return out


@pytest.mark.parametrize("name", list(sr.CASES))
def test_oracle_equals_the_reference_fixture(steps, name):
    inp, s = steps[name]
    fx = sr.load_fixture(name)
    assert int(fx["max_stored"]) == sr.MAX_STORED and int(fx["seed"]) == sr.seed_of(name)
    worst = 0.0
    for k in sr.MAPS + sr.DMAPS:
        assert fx[k].size <= sr.MAX_STORED
        worst = max(worst, np.abs(sr.stored(s[k]) - fx[k]).max())
    for i, g in enumerate(s["grads"]):
        assert np.asarray(g).size == inp["params"][i].size
        worst = max(worst, np.abs(sr.stored(g) - fx[f"g{i}"]).max())
    worst = max(worst, abs(s["loss"] - float(fx["loss"])), abs(s["ce"] - float(fx["ce"])), abs(s["dice"] - float(fx["dice"])))
    print(f"case {name}: oracle vs fixture max|diff| {worst:.2e}")
    assert worst <= 1e-10
    assert s["valid"] == int(fx["valid"]) and s["stray"] == 0


def test_cases_are_what_they_are_for(steps):
    for name, (N, c_in, c_hidden, d1, c_skip, classes, h, w, weights, src) in sr.CASES.items():
        inp, s = steps[name]
        assert c_in % 16 == 0 and c_hidden % 16 == 0 and d1 % 16 == 0 and (c_hidden + d1 // 4) % 16 == 0 and (d1 // 4 + c_skip) % 16 == 0
        lab = inp["labels"][:-1] if src == "B" else inp["labels"]
        assert (lab != sr.IGNORE).mean() >= 0.5
        assert s["logits"].shape == (N, classes, 2 * h, 2 * w)
    assert sr.CASES["A"][5] < 16 < sr.CASES["B"][5] < 32 and sr.CASES["D"][6:8] == (2, 2)
    inp, s = steps["A"]
    assert 0.03 < (inp["labels"] == sr.IGNORE).mean() < 0.2
    inp, s = steps["B"]
    assert (inp["labels"][-1] == sr.IGNORE).all() and not s["dlogits"][-1].any()       # the ignored frame: zero gradient
    assert not (inp["labels"] == 18).any()                                               # the absent class stays in the divisor
    assert s["pooled"].shape[2:] == (5, 9)
    assert sr.CASES["Bce"][8] == (1.0, 0.0) and abs(steps["Bce"][1]["loss"] - s["ce"]) <= 1e-14
    assert sr.CASES["C"][1:5] == (64, 64, 128, 64)


def test_oracle_against_finite_differences():
    """Central differences of the float64 loss on case A: three entries of every parameter, and eight logits of the loss
    alone.  |fd - g| <= 1e-6 max|g| + 1e-10: truncation h^2 = 1e-10, rounding 1e-16 / h = 1e-11."""
    inp = sr.make_inputs("A")
    params = [p.astype(np.float64) for p in inp["params"]]
    s = sr.step_gradients(inp, params)
    rng = np.random.default_rng(7)
    h = 1e-5
    worst = 0.0
    for i, g in enumerate(s["grads"]):
        g = np.asarray(g).reshape(params[i].shape)
        for _ in range(3):
            idx = tuple(int(rng.integers(0, n)) for n in g.shape)
            keep = params[i][idx]
            params[i][idx] = keep + h
            up = sr.loss_from(inp, params)
            params[i][idx] = keep - h
            dn = sr.loss_from(inp, params)
            params[i][idx] = keep
            err = abs((up - dn) / (2 * h) - g[idx]) / (1e-6 * np.abs(g).max() + 1e-10)
            worst = max(worst, err)
            assert err <= 1.0, (sr.PARAMS[i], idx, (up - dn) / (2 * h), g[idx])
    z = np.array(s["logits"], np.float64)
    g = s["dlogits"]
    for _ in range(8):
        idx = tuple(int(rng.integers(0, n)) for n in z.shape)
        keep = z[idx]
        z[idx] = keep + h
        up = sr.seg_loss(z, inp["labels"], inp["weights"])["loss"]
        z[idx] = keep - h
        dn = sr.seg_loss(z, inp["labels"], inp["weights"])["loss"]
        z[idx] = keep
        err = abs((up - dn) / (2 * h) - g[idx]) / (1e-6 * np.abs(g).max() + 1e-10)
        worst = max(worst, err)
        assert err <= 1.0, ("dlogits", idx)
    print(f"finite differences: {worst:.3f} of the bound")


def _torch_loss(z, labels, weights, ignore=sr.IGNORE, eps=1e-7):
    """CrossEntropyLoss(ignore_index) and the Dice loss written out in plain torch, under autograd."""
    z = torch.from_numpy(np.asarray(z, np.float64)).requires_grad_(True)
    y = torch.from_numpy(np.asarray(labels).astype(np.int64))
    C = z.shape[1]
    ce = torch.nn.functional.cross_entropy(z, y, ignore_index=ignore)
    mask = (y != ignore)
    p = torch.softmax(z, dim=1) * mask[:, None]
    t = torch.nn.functional.one_hot(torch.where(mask, y, 0), C).permute(0, 3, 1, 2).double() * mask[:, None]
    inter, card = (p * t).sum(dim=(0, 2, 3)), (p + t).sum(dim=(0, 2, 3))
    dice = (((1 - 2 * inter / card.clamp_min(eps)) * (t.sum(dim=(0, 2, 3)) > 0)).sum()) / C
    loss = weights[0] * ce + weights[1] * dice
    loss.backward()
    return float(loss.detach()), float(ce.detach()), float(dice.detach()), z.grad.numpy()


@pytest.mark.parametrize("name", list(sr.CASES))
def test_loss_matches_a_plain_torch_restatement(steps, name):
    inp, s = steps[name]
    loss, ce, dice, dz = _torch_loss(s["logits"], inp["labels"], inp["weights"])
    assert abs(loss - s["loss"]) <= 1e-12 and abs(ce - s["ce"]) <= 1e-12 and abs(dice - s["dice"]) <= 1e-12
    assert np.abs(dz - s["dlogits"]).max() <= 1e-12


def test_loss_deviations_of_the_oracle():
    inp = sr.make_inputs("A")
    z = sr.step_gradients(inp)["logits"]
    none = sr.seg_loss(z, np.full(inp["labels"].shape, sr.IGNORE, np.uint8))
    assert none["loss"] == 0.0 and none["valid"] == 0 and not none["dz"].any()
    lab = inp["labels"].copy()
    where = np.argwhere(lab != sr.IGNORE)[:3]
    base = lab.copy()
    for i in where:
        lab[tuple(i)] = 77                       # outside [0, 5), not the ignore index: stray
        base[tuple(i)] = sr.IGNORE
    a, b = sr.seg_loss(z, lab), sr.seg_loss(z, base)
    assert a["stray"] == 3 and b["stray"] == 0 and a["valid"] == b["valid"]
    assert a["loss"] == b["loss"] and np.array_equal(a["dz"], b["dz"])


def test_pool_rule_and_shuffle_against_torch():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 3, (2, 3, 5, 7)).astype(np.float64)      # ties in most windows, an odd last row and column
    t = torch.from_numpy(x).requires_grad_(True)
    y = torch.nn.functional.max_pool2d(t, 2, 2)
    dy = rng.standard_normal(tuple(y.shape))
    y.backward(torch.from_numpy(dy))
    assert np.array_equal(sr.maxpool2(x)[0], y.detach().numpy())
    assert np.array_equal(sr.maxpool2_backward(x, dy), t.grad.numpy())
    a, b = rng.standard_normal((2, 8, 3, 5)), rng.standard_normal((2, 3, 6, 10))
    ta = torch.from_numpy(a).requires_grad_(True)
    out = torch.cat([torch.nn.functional.pixel_shuffle(ta, 2), torch.from_numpy(b)], dim=1)
    d = rng.standard_normal(tuple(out.shape))
    out.backward(torch.from_numpy(d))
    assert np.array_equal(sr.shuffle_cat(a, b), out.detach().numpy())
    assert np.array_equal(sr.shuffle_cat_backward(d, 2), ta.grad.numpy())


def test_bounds_come_from_the_fixtures():
    b = sr.bounds()
    for k, v in b.items():
        assert v == max(8.0 * max(float(sr.load_fixture(n)["err32_" + k]) for n in sr.CASES), sr.FLOOR)
        assert sr.FLOOR <= v < 1e-4, k                               # far below a missing term's 1e-2
    tb = sr.trajectory_bounds()
    assert set(tb) == {"loss_head", "loss_last", "p24_last", "p25_last"} | {f"p{i}_head" for i in range(26)}
    assert all(sr.FLOOR <= v < 1e-4 for v in tb.values())


def test_trajectory_falls():
    inp = sr.make_inputs(sr.TRAJECTORY_CASE)
    fx = sr.load_trajectory()
    for mode, trained in (("head", list(range(26))), ("last", [24, 25])):
        losses, after = sr.trajectory(inp, mode)
        assert np.abs(losses - fx[f"losses_{mode}"]).max() <= 1e-10
        assert (losses[1:] < losses[:-1]).all()
        for t, ps in enumerate(after):
            for i, p in zip(trained, ps):
                assert np.abs(sr.stored(p, sr.TRAJ_STORED) - fx[f"p{i}_{mode}"][t]).max() <= 1e-10, (mode, t, sr.PARAMS[i])


# ---- argument checks: nothing below may reach the library -------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(st._lib, "load", boom)


@pytest.fixture
def shapes_only(no_library, monkeypatch):
    monkeypatch.setattr("nano_vs_slam_amd.train_ops._is_device", lambda t: True)     # shapes, on a box without a device


def test_cpu_tensors_raise(no_library):
    x, w, b = torch.zeros(2, 16, 4, 6), torch.zeros(5, 16, 3, 3), torch.zeros(5)
    z, lab = torch.zeros(2, 5, 4, 6), torch.zeros(2, 4, 6, dtype=torch.uint8)
    for call in (lambda: st.conv_bias_forward(x, w, b), lambda: st.conv_bias_backward(x, w, z), lambda: st.segmentation_loss(z, lab),
                 lambda: st.maxpool2_forward(x), lambda: st.maxpool2_backward(x, torch.zeros(2, 16, 2, 3)),
                 lambda: st.shuffle_cat_forward(x, torch.zeros(2, 3, 8, 12)), lambda: st.shuffle_cat_backward(torch.zeros(2, 7, 8, 12), 4)):
        with pytest.raises(ValueError, match="no CPU path"):
            call()


def test_bad_shapes_raise(shapes_only):
    x, w, b = torch.zeros(2, 16, 4, 6), torch.zeros(5, 16, 3, 3), torch.zeros(5)
    for bad in ((x[0], w, b), (x.double(), w, b), (x, w[:, :8], b), (x, w[:, :, :2], b), (x, w, b[:4]), (x, w, b.double()), (x, w, None),
                (x[:0], w, b), (x[:, :, :0], w, b), (x, torch.zeros(0, 16, 3, 3), torch.zeros(0)),
                (torch.zeros(2, 24, 4, 6), torch.zeros(5, 24, 3, 3), b),                             # Cin % 16
                (torch.zeros(1, 144, 2, 2), torch.zeros(5, 144, 3, 3), b),                           # Cin > 128
                (x, torch.zeros(129, 16, 3, 3), torch.zeros(129))):                                  # Cout > 128
        with pytest.raises(ValueError):
            st.conv_bias_forward(*bad)
    for dy in (torch.zeros(2, 5, 4, 5), torch.zeros(2, 16, 4, 6), torch.zeros(2, 5, 4, 6).double()):
        with pytest.raises(ValueError):
            st.conv_bias_backward(x, w, dy)
    z = torch.zeros(2, 5, 4, 6)
    for lab in (torch.zeros(2, 4, 5, dtype=torch.uint8), torch.zeros(2, 8, 12, dtype=torch.uint8), torch.zeros(2, 4, 6, dtype=torch.int16),
                torch.zeros(2, 4, 6), torch.zeros(2, 1, 4, 6, dtype=torch.int64)):
        with pytest.raises(ValueError):
            st.segmentation_loss(z, lab)
    lab = torch.zeros(2, 4, 6, dtype=torch.int64)
    for kw in ({"ce_weight": -1.0}, {"dice_weight": float("inf")}, {"ce_weight": float("nan")}, {"ignore_index": 2 ** 63}):
        with pytest.raises(ValueError):
            st.segmentation_loss(z, lab, **kw)
    with pytest.raises(ValueError):
        st.segmentation_loss(torch.zeros(2, 129, 4, 6), lab)
    for bad in (x[0], x.double(), torch.zeros(2, 16, 1, 6)):
        with pytest.raises(ValueError):
            st.maxpool2_forward(bad)
    with pytest.raises(ValueError):
        st.maxpool2_backward(x, torch.zeros(2, 16, 2, 2))
    for a, b2 in ((x, torch.zeros(2, 3, 8, 11)), (torch.zeros(2, 6, 4, 6), torch.zeros(2, 3, 8, 12)), (x, torch.zeros(1, 3, 8, 12)),
                  (x, torch.zeros(2, 3, 9, 13))):
        with pytest.raises(ValueError):
            st.shuffle_cat_forward(a, b2)
    for d, C in ((torch.zeros(2, 7, 8, 12), 8), (torch.zeros(2, 7, 7, 12), 4), (torch.zeros(2, 7, 8, 12), 0)):
        with pytest.raises(ValueError):
            st.shuffle_cat_backward(d, C)


def test_trainer_refusals(shapes_only):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import KP2DTinyV2, get_config, tiny_factory
    with pytest.raises(ValueError, match="V3"):
        st.SegHeadTrainer(tiny_factory("S", 28, v3=True))
    with pytest.raises(ValueError, match="V3"):
        st.SegHeadTrainer(tiny_factory("S", 28, v3=True), train="last")
    with pytest.raises(ValueError, match="attention"):
        st.SegHeadTrainer(tiny_factory("S_A", 28), train="head")
    with pytest.raises(ValueError, match="convtranspose"):
        st.SegHeadTrainer(tiny_factory("S", 28, to_mcu=True))
    with pytest.raises(ValueError, match="convtranspose"):
        st.SegHeadTrainer(tiny_factory("S", 28, to_mcu=True), train="last")
    with pytest.raises(ValueError, match="channel counts"):
        st.SegHeadTrainer(tiny_factory("N", 28), train="head")        # the 72-channel concatenation
    with pytest.raises(ValueError, match="train must be"):
        st.SegHeadTrainer(tiny_factory("S", 28), train="depth")
    with pytest.raises(ValueError, match="channel counts"):
        st.SegHeadTrainer(tiny_factory("S", 200), train="last")        # more than 128 classes
    model = tiny_factory("S", 19)
    for kw in ({"lr": -1.0}, {"betas": (1.0, 0.999)}, {"eps": -1e-8}, {"ce_weight": -0.5}, {"dice_weight": float("nan")}):
        with pytest.raises(ValueError):
            st.SegHeadTrainer(model, **kw)
    assert len(st.SegHeadTrainer(tiny_factory("N", 28), train="last").parameters()) == 2
    assert len(st.SegHeadTrainer(tiny_factory("S_A", 28), train="last").parameters()) == 2       # the attention head's last layer
    depth = KP2DTinyV2(**get_config("S"), nClasses=19, depth=True)
    assert st.SegHeadTrainer(depth).convs[-1] is depth.seg_head.convs[8]                          # never the depth head

    trainer = st.SegHeadTrainer(model)
    named = dict(model.seg_head.named_parameters())               # every parameter of the head, in registration order
    assert [id(p) for p in trainer.parameters()] == [id(named[n]) for n in sr.PARAMS] and len(named) == 26
    x, skip = torch.zeros(2, 64, 4, 6), torch.zeros(2, 64, 8, 12)
    lab = torch.zeros(2, 8, 12, dtype=torch.uint8)
    with pytest.raises(ValueError, match="even"):
        trainer.step_features(torch.zeros(2, 64, 5, 6), torch.zeros(2, 64, 10, 12), torch.zeros(2, 10, 12, dtype=torch.uint8))
    with pytest.raises(ValueError, match="even"):
        trainer.forward_features(torch.zeros(2, 64, 4, 7), torch.zeros(2, 64, 8, 14))
    with pytest.raises(ValueError, match="logits' size"):
        trainer.step_features(x, skip, torch.zeros(2, 4, 6, dtype=torch.uint8))                   # labels at the backbone's size
    with pytest.raises(ValueError):
        trainer.step_features(x, skip, lab.float())
    with pytest.raises(ValueError):
        trainer.step_features(x, torch.zeros(2, 32, 8, 12), lab)
    with pytest.raises(ValueError):
        trainer.step_features(x, None, lab)
    with pytest.raises(ValueError):
        trainer.step_features(x[:, :32], skip, lab)
    last = st.SegHeadTrainer(model, train="last")
    with pytest.raises(ValueError):
        last.step_features(x, skip, lab)                           # "last" mode takes the last layer's input alone
    with pytest.raises(ValueError, match="logits' size"):
        last.step_features(torch.zeros(2, 64, 8, 12), None, torch.zeros(2, 4, 6, dtype=torch.uint8))
    w = model.seg_head.convs[8].weight
    w.data = w.data.permute(0, 1, 3, 2)                            # a non-contiguous parameter
    assert not w.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        trainer.step_features(x, skip, lab)
    with pytest.raises(ValueError, match="contiguous"):
        last.step_features(torch.zeros(2, 64, 8, 12), None, lab)


def test_trainer_refuses_cpu_tensors(no_library):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    trainer = st.SegHeadTrainer(tiny_factory("S", 19))
    with pytest.raises(ValueError, match="no CPU path"):
        trainer.step_features(torch.zeros(2, 64, 4, 6), torch.zeros(2, 64, 8, 12), torch.zeros(2, 8, 12, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no CPU path"):
        trainer.forward_features(torch.zeros(2, 64, 4, 6), torch.zeros(2, 64, 8, 12))
    with pytest.raises(ValueError, match="no CPU path"):
        trainer.step(torch.zeros(1, 3, 32, 32), torch.zeros(1, 16, 16, dtype=torch.uint8))


# ---- the new signatures against the header ------------------------------------------------------------------------------------
NEW = ("kp2d_conv_bias_scratch_bytes", "kp2d_conv_bias_forward_train", "kp2d_conv_bias_backward", "kp2d_seg_loss_scratch_bytes",
       "kp2d_seg_loss", "kp2d_maxpool2_forward_train", "kp2d_maxpool2_backward", "kp2d_shuffle_cat_forward", "kp2d_shuffle_cat_backward")


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
