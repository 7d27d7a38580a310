"""The NetVLAD training step without a GPU: the numpy float64 oracle (vlad_training_ref) against the fixtures that
tools/make_vlad_training_golden.py wrote from the reference's NetVLAD module with torch autograd, TripletMarginLoss and
Adam; the conditions on the inputs under which tests/test_gpu_vlad_training.py compares the device; and the argument
checks of nano_vs_slam_amd.vlad_training, which fire before any library call."""
import numpy as np
import pytest
import torch

import vlad_training_ref as vr
from nano_vs_slam_amd import vlad_training as vt


@pytest.fixture(scope="module")
def steps():
    out = {}
    for name in vr.CASES:
        inp = vr.make_inputs(name)
        out[name] = (inp, vr.step_gradients(inp["x"], inp["W"], inp["cent"], inp["B"], inp["counts"]), vr.load_fixture(name))
    return out


@pytest.fixture(scope="module")
def traj():
    return vr.trajectory(vr.make_inputs(vr.TRAJECTORY_CASE))


@pytest.mark.parametrize("name", list(vr.CASES))
def test_oracle_reproduces_the_reference(steps, name):
    inp, s, fx = steps[name]
    assert s["vlad"].shape == (2 * inp["B"] + sum(inp["counts"]), inp["K"] * inp["C"])
    st = int(fx["col_stride"])
    assert st == vr.COL_STRIDE and fx["vlad_cols"].shape == fx["dvlad_cols"].shape == s["vlad"][:, ::st].shape
    assert np.abs(s["vlad"][:, ::st] - fx["vlad_cols"]).max() <= 1e-10
    assert abs(s["loss"] - float(fx["loss"])) <= 1e-10
    assert np.abs(s["dvlad"][:, ::st] - fx["dvlad_cols"]).max() <= 1e-10
    for k in ("dW", "dcent"):
        assert np.abs(s[k] - fx[k]).max() <= 1e-10 and vr.rel_err(s[k], fx[k]) <= 1e-10, k
    assert s["n_active"] == int(fx["n_active"]) and float(fx["margin"]) == vr.MARGIN


def test_oracle_reproduces_the_reference_trajectory(traj):
    fx = vr.load_fixture(vr.TRAJECTORY_CASE)
    losses, W3, c3, _ = traj
    assert float(fx["lr"]) == vr.LR and len(fx["losses"]) == vr.TRAJECTORY_STEPS
    assert np.abs(losses - fx["losses"]).max() <= 1e-10
    assert np.abs(W3 - fx["W_after"]).max() <= 1e-10 and np.abs(c3 - fx["cent_after"]).max() <= 1e-10


def test_input_conditions(steps):
    """Every hinge argument is at least 1e-3 away from 0 (no triplet's activity can depend on rounding), one case has
    inactive triplets, and the zero-negative query of case B is there."""
    inactive = 0
    for name, (inp, s, _) in steps.items():
        assert len(s["hinge"]) == sum(inp["counts"]) and np.abs(s["hinge"]).min() >= 1e-3, name
        inactive += len(s["hinge"]) - s["n_active"]
        print(name, "active", s["n_active"], "of", len(s["hinge"]), "min |hinge| %.3e" % np.abs(s["hinge"]).min())
    assert inactive > 0
    inp, s, _ = steps["B"]
    assert inp["counts"][1] == 0 and 0 < s["n_active"] < len(s["hinge"])
    assert not s["dvlad"][1].any() and not s["dvlad"][inp["B"] + 1].any()


def test_bounds_come_from_the_fixtures():
    b = vr.bounds()
    print("bounds", b)
    for k in ("loss", "dW", "dcent"):
        assert b[k] == 8.0 * max(float(vr.load_fixture(n)["err32_" + k]) for n in vr.CASES)
    assert 0 < b["loss"] < 1e-5 and 0 < b["grad"] <= min(b["dW"], b["dcent"]) < 1e-3       # far below a missing term's 1e-2
    assert vr.loss_bound(0.25, b) >= 16 * 2.0 ** -25


def test_trajectory_falls_and_sign_driven_share(traj):
    b = vr.bounds()
    losses, _, _, grads = traj
    fx = vr.load_fixture(vr.TRAJECTORY_CASE)
    drop = losses[:-1] - losses[1:]
    print("loss drop per step", drop, "loss bound", vr.loss_bound(losses[0], b))
    assert (drop >= 10.0 * vr.loss_bound(losses[0], b)).all()
    assert float(fx["err32_losses"]) <= 1e-6                    # the reference's float32 and float64 runs agree
    mw, mc = vr.sign_driven(grads, b)
    share = (mw.sum() + mc.sum()) / (mw.size + mc.size)
    print("sign-driven share", share)
    assert share <= 0.01


# ---- argument checks: nothing below may reach the library -------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(vt._lib, "load", boom)


def test_cpu_tensors_raise(no_library):
    x, W, c = torch.zeros(3, 16, 4, 3), torch.zeros(8, 16, 1, 1), torch.zeros(8, 16)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        vt.netvlad_forward(x, W, c)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        vt.netvlad_backward(x, W, c, torch.zeros(3, 8 * 16 + 20), torch.zeros(3, 128))
    with pytest.raises(RuntimeError, match="CPU tensors"):
        vt.triplet_margin_loss(torch.zeros(3, 128), 1, [1])
    with pytest.raises(RuntimeError, match="CPU tensors"):
        vt.adam_step(*(torch.zeros(4) for _ in range(4)), 1)


def test_bad_shapes_raise(no_library, monkeypatch):
    monkeypatch.setattr(vt._dev, "require_device", lambda name, t, hint="": t)       # shapes, on a box without a device
    x, W, c = torch.zeros(3, 16, 4, 3), torch.zeros(8, 16, 1, 1), torch.zeros(8, 16)
    for bad in ((x[:, :12], W, c), (x, W[:4], c), (x.double(), W, c), (x[:0], W, c), (x[:, :, :0], W, c),
                (torch.zeros(3, 18, 4, 3), torch.zeros(8, 18, 1, 1), torch.zeros(8, 18)),            # C % 4
                (torch.zeros(3, 16, 4, 3), torch.zeros(6, 16, 1, 1), torch.zeros(6, 16)),            # K % 4
                (torch.zeros(1, 256, 2, 2), torch.zeros(64, 256, 1, 1), torch.zeros(64, 256))):      # K C > 8192
        with pytest.raises(ValueError):
            vt.netvlad_forward(*bad)
    with pytest.raises(ValueError):
        vt.netvlad_backward(x, W, c, torch.zeros(3, 8 * 16 + 19), torch.zeros(3, 128))
    with pytest.raises(ValueError):
        vt.netvlad_backward(x, W, c, torch.zeros(3, 8 * 16 + 20), torch.zeros(2, 128))
    v = torch.zeros(5, 128)
    for B, counts in ((0, []), (3, [0, 0, 0]), (2, [1]), (2, [1, 1]), (1, [-1]), (2, torch.tensor([1.0, 0.0])),
                      (2, torch.tensor([-1, 2]))):
        with pytest.raises(ValueError):
            vt.triplet_margin_loss(v, B, counts)
    with pytest.raises(ValueError):
        vt.triplet_margin_loss(v, 2, [1, 0], margin=-1.0)
    with pytest.raises(ValueError):
        vt.adam_step(torch.zeros(4), torch.zeros(5), torch.zeros(4), torch.zeros(4), 1)
    with pytest.raises(ValueError):
        vt.adam_step(*(torch.zeros(4) for _ in range(4)), 0)


@pytest.mark.parametrize("config,kw", [("GEM_N", {}), ("CONVAP_S_A", {}), ("S", {"to_export": True})])
def test_trainer_refuses_other_poolers(no_library, config, kw):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    with pytest.raises(ValueError, match="NetVLAD|remove_netvlad"):
        vt.NetVLADTrainer(tiny_factory(config, 28, **kw))


def test_trainer_checks_its_settings_and_frames(no_library):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    model = tiny_factory("S", 28)
    with pytest.raises(ValueError):
        vt.NetVLADTrainer(model, betas=(0.9, 1.0))
    trainer = vt.NetVLADTrainer(model)
    f = torch.zeros(2, 3, 32, 32)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        trainer.step(f, f, f, [1, 1])
    with pytest.raises(RuntimeError, match="CPU tensors"):
        trainer.step_encoded(torch.zeros(6, 64, 4, 4), 2, [1, 1])
    assert trainer.steps == 0
