"""The float64 oracle of the head training step (vpr_head_training_ref) against the fixtures written from the reference's
VPRHead (to 1e-10 on every stored entry), against central finite differences, and the argument checks of the Python layer:
everything here runs without a device."""
import numpy as np
import pytest
import torch

import vpr_head_training_ref as hr
from nano_vs_slam_amd import vpr_head_training as ht


@pytest.fixture(scope="module")
def steps():
    out = {}
    for name in hr.CASES:
        inp = hr.make_inputs(name)
        out[name] = (inp, hr.step_gradients(inp["feat"], inp["params"], inp["stats"], inp["B"], inp["counts"], inp["slope"]))
    return out


@pytest.mark.parametrize("name", list(hr.CASES))
def test_oracle_equals_the_reference_fixture(steps, name):
    inp, s = steps[name]
    fx = hr.load_fixture(name)
    assert int(fx["max_stored"]) == hr.MAX_STORED
    worst = 0.0
    for k in hr.MAPS + ("vlad", "dvlad"):
        assert fx[k].size <= hr.MAX_STORED
        worst = max(worst, np.abs(hr.stored(s[k]) - fx[k]).max())
    for i, g in enumerate(s["grads"]):
        worst = max(worst, np.abs(hr.stored(g) - fx[f"g{i}"]).max())
    worst = max(worst, abs(s["loss"] - float(fx["loss"])))
    print(f"case {name}: oracle vs fixture max|diff| {worst:.2e}")
    assert worst <= 1e-10
    assert s["n_active"] == int(fx["n_active"])
    assert np.abs(s["hinge"]).min() >= 1e-4


def test_cases_are_what_they_are_for(steps):
    active = sum(s["n_active"] for _, s in steps.values())
    total = sum(len(s["hinge"]) for _, s in steps.values())
    assert active >= 1 and total - active >= 1
    inp, s = steps["B"]                       # the query without negatives: two frames with exactly zero gradients
    B = inp["B"]
    for k in ("dvlad", "dx_netvlad", "dx3", "dx2"):
        assert not s[k][1].any() and not s[k][B + 1].any(), k
        assert s[k][0].any()
    inp, s = steps["E"]                       # ReLU, and one channel per layer whose gamma is 0 but whose dgamma is not
    assert inp["slope"] == 0.0
    for i in range(3):
        zero = np.flatnonzero(inp["params"][3 * i + 1] == 0)
        assert zero.size == 1 and s["grads"][3 * i + 1][zero[0]] != 0
    for name, (Cin, C, K, H, W, *_) in hr.CASES.items():
        assert Cin % 16 == 0 and C % 16 == 0 and K % 4 == 0


def test_oracle_against_finite_differences():
    """Central differences of the float64 loss on case A: six entries of every parameter and of the three inputs dx is
    formed for.  |fd - g| <= 1e-6 max|g| + 1e-10: the truncation error of h = 1e-5 on a loss of order 1 is about
    h^2 = 1e-10 and the rounding error 1e-16 / h = 1e-11."""
    inp = hr.make_inputs("A")
    params = [p.astype(np.float64) for p in inp["params"]]
    args = (inp["stats"], inp["B"], inp["counts"], inp["slope"])
    s = hr.step_gradients(inp["feat"], params, *args)
    rng = np.random.default_rng(5)
    h = 1e-5
    worst = 0.0
    for i, g in enumerate(s["grads"]):
        g = np.asarray(g).reshape(params[i].shape)
        for _ in range(6):
            idx = tuple(int(rng.integers(0, n)) for n in g.shape)
            keep = params[i][idx]
            params[i][idx] = keep + h
            up = hr.loss_from(inp["feat"], 0, params, *args)
            params[i][idx] = keep - h
            dn = hr.loss_from(inp["feat"], 0, params, *args)
            params[i][idx] = keep
            err = abs((up - dn) / (2 * h) - g[idx]) / (1e-6 * np.abs(g).max() + 1e-10)
            worst = max(worst, err)
            assert err <= 1.0, (hr.PARAMS[i], idx, (up - dn) / (2 * h), g[idx])
    for key, start in (("dx2", 1), ("dx3", 2), ("dx_netvlad", 3)):
        x = np.array(s[f"y{start}"], np.float64)
        g = s[key]
        for _ in range(6):
            idx = tuple(int(rng.integers(0, n)) for n in g.shape)
            keep = x[idx]
            x[idx] = keep + h
            up = hr.loss_from(x, start, params, *args)
            x[idx] = keep - h
            dn = hr.loss_from(x, start, params, *args)
            x[idx] = keep
            err = abs((up - dn) / (2 * h) - g[idx]) / (1e-6 * np.abs(g).max() + 1e-10)
            worst = max(worst, err)
            assert err <= 1.0, (key, idx, (up - dn) / (2 * h), g[idx])
    print(f"finite differences: {worst:.3f} of the bound")


def test_bounds_come_from_the_fixtures():
    b = hr.bounds()
    print("bounds", b)
    for k in ("loss",) + tuple(hr.GROUPS) + hr.MAPS:
        assert b[k] == 8.0 * max(float(hr.load_fixture(n)["err32_" + k]) for n in hr.CASES)
        assert 0 < b[k] < 1e-3                                  # far below a missing term's 1e-2
    assert hr.loss_bound(0.25, b) >= 16 * 2.0 ** -25


def test_trajectory_falls():
    inp = hr.make_inputs(hr.TRAJECTORY_CASE)
    fx = hr.load_fixture(hr.TRAJECTORY_CASE)
    losses, kept, _ = hr.trajectory(inp)
    assert np.abs(losses - fx["losses"]).max() <= 1e-10
    assert (losses[1:] < losses[:-1]).all()
    for i, p in enumerate(kept):
        assert np.abs(hr.stored(p) - fx[f"p{i}_after"]).max() <= 1e-10, hr.PARAMS[i]
    assert float(fx["err32_losses"]) <= 1e-5                    # the reference's float32 and float64 runs agree


# ---- argument checks: nothing below may reach the library -------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ht._lib, "load", boom)


def _layer(N=2, Cin=16, Cout=32, H=3, W=4):
    return (torch.zeros(N, Cin, H, W), torch.zeros(Cout, Cin, 3, 3), torch.zeros(Cout), torch.zeros(Cout), torch.zeros(Cout),
            torch.zeros(N, Cout, H, W))


def test_cpu_tensors_raise(no_library):
    x, w, v0, v1, v2, m = _layer()
    with pytest.raises(RuntimeError, match="CPU tensors"):
        ht.cbr_forward(x, w, v0, v1)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        ht.cbr_backward(x, w, v0, v1, v2, m, m, m)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        ht.netvlad_backward_input(torch.zeros(3, 16, 4, 3), torch.zeros(8, 16, 1, 1), torch.zeros(8, 16), torch.zeros(3, 148), torch.zeros(3, 128))


def test_bad_shapes_raise(no_library, monkeypatch):
    monkeypatch.setattr(ht._dev, "require_device", lambda name, t, hint="": t)       # shapes, on a box without a device
    x, w, v0, v1, v2, m = _layer()
    for bad in ((x[0], w, v0, v1), (x.double(), w, v0, v1), (x, w[:, :8], v0, v1), (x, w[:, :, :2], v0, v1), (x, w, v0[:16], v1),
                (x, w, v0, v1.double()), (x[:0], w, v0, v1), (x[:, :, :0], w, v0, v1),
                (torch.zeros(2, 24, 3, 4), torch.zeros(32, 24, 3, 3), v0, v1),                                # Cin % 16
                (x, torch.zeros(40, 16, 3, 3), torch.zeros(40), torch.zeros(40)),                            # Cout % 16
                (torch.zeros(1, 144, 2, 2), torch.zeros(32, 144, 3, 3), v0, v1)):                            # Cin > 128
        with pytest.raises(ValueError):
            ht.cbr_forward(*bad)
    for slope in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            ht.cbr_forward(x, w, v0, v1, slope)
    for bad in ((x, w, v0, v1, v2, m[:1], m, m), (x, w, v0, v1, v2, m, m[:, :16], m), (x, w, v0, v1, v2, m, m, m.double()),
                (x, w, v0, v1, v2[:8], m, m, m)):
        with pytest.raises(ValueError):
            ht.cbr_backward(*bad)
    e, W, c = torch.zeros(3, 16, 4, 3), torch.zeros(8, 16, 1, 1), torch.zeros(8, 16)
    with pytest.raises(ValueError):
        ht.netvlad_backward_input(e, W, c, torch.zeros(3, 8 * 16 + 19), torch.zeros(3, 128))
    with pytest.raises(ValueError):
        ht.netvlad_backward_input(e, W, c, torch.zeros(3, 8 * 16 + 20), torch.zeros(2, 128))
    with pytest.raises(ValueError):      # C above the input gradient's 128
        ht.netvlad_backward_input(torch.zeros(1, 256, 2, 2), torch.zeros(8, 256, 1, 1), torch.zeros(8, 256), torch.zeros(1, 8 * 256 + 20),
                                  torch.zeros(1, 8 * 256))


def test_trainer_refuses_other_poolers_and_bad_settings(no_library):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    for config in ("GEM_N", "CONVAP_S_A"):
        with pytest.raises(ValueError, match="NetVLAD pooler"):
            ht.VPRHeadTrainer(tiny_factory(config, 28))
    with pytest.raises(ValueError, match="remove_netvlad"):
        ht.VPRHeadTrainer(tiny_factory("S", 28, to_export=True))
    model = tiny_factory("S", 28)
    for kw in ({"lr": -1.0}, {"margin": -0.1}, {"betas": (1.0, 0.999)}, {"eps": -1e-8}):
        with pytest.raises(ValueError):
            ht.VPRHeadTrainer(model, **kw)
    trainer = ht.VPRHeadTrainer(tiny_factory("S_A", 28, v3=True))       # V3 attention configs: the head is the same
    named = dict(trainer.model.vlad_head.named_parameters())      # every parameter of the head, and nothing else
    assert [id(p) for p in trainer.parameters()] == [id(named[n]) for n in hr.PARAMS]
    assert len(named) == 11 and trainer.slope == 0.01
    with pytest.raises(RuntimeError, match="CPU tensors"):
        trainer.step_features(torch.zeros(3, 64, 4, 4), 1, [1])
    with pytest.raises(RuntimeError, match="CPU tensors"):
        trainer.step(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32), [1])
