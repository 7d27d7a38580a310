"""The float64 oracle of the head training step on batch statistics with Dropout2d (vpr_head_bn_ref) against the fixtures
written from the reference's VPRHead in .train() (to 1e-10 on every stored entry), against central finite differences
(which is what proves the two terms through the batch mean and variance), the Python restatement of the dropout draw, and
the argument checks of the Python layer: everything here runs without a device."""
import numpy as np
import pytest
import torch

import vpr_head_bn_ref as br
from nano_vs_slam_amd import vpr_head_training as ht

hr = br.hr


@pytest.fixture(scope="module")
def steps():
    out = {}
    for name, (case, p, seed) in br.FIXTURES.items():
        inp = hr.make_inputs(case)
        fx = br.load_fixture(name)
        out[name] = (inp, fx, br.step_gradients(inp["feat"], inp["params"], inp["stats"], inp["B"], inp["counts"], inp["slope"], fx["mask"]))
    return out


@pytest.mark.parametrize("name", list(br.FIXTURES))
def test_oracle_equals_the_reference_fixture(steps, name):
    inp, fx, s = steps[name]
    case, p, seed = br.FIXTURES[name]
    assert int(fx["max_stored"]) == hr.MAX_STORED and float(fx["p"]) == p and int(fx["torch_seed"]) == seed
    assert float(fx["momentum"]) == br.MOMENTUM
    mask = fx["mask"]
    assert mask.shape == (inp["N"], inp["C"]) and mask.dtype == np.float32
    kept = np.float32(1.0 / (1.0 - p))
    assert ((mask == 0) | (mask == kept)).all() and ((mask == 0).any() == (p > 0))
    worst = 0.0
    for k in hr.MAPS + ("vlad", "dvlad") + br.STATS:
        assert fx[k].size <= hr.MAX_STORED
        worst = max(worst, np.abs(hr.stored(s[k]) - fx[k]).max())
    for i, g in enumerate(s["grads"]):
        worst = max(worst, np.abs(hr.stored(g) - fx[f"g{i}"]).max())
    worst = max(worst, abs(s["loss"] - float(fx["loss"])))
    print(f"{name}: oracle vs fixture max|diff| {worst:.2e}")
    assert worst <= 1e-10
    assert s["n_active"] == int(fx["n_active"])
    assert np.abs(s["hinge"]).min() >= 1e-4


def test_fixtures_are_what_they_are_for(steps):
    active = sum(s["n_active"] for _, _, s in steps.values())
    total = sum(len(s["hinge"]) for _, _, s in steps.values())
    assert active >= 1 and total - active >= 1
    inp, fx, s = steps["E_p20"]               # ReLU, one channel per layer whose gamma is 0 but whose dgamma is not, M = 18
    assert inp["slope"] == 0.0 and inp["N"] * inp["H"] * inp["W"] == 18
    for i in range(3):
        zero = np.flatnonzero(inp["params"][3 * i + 1] == 0)
        assert zero.size == 1 and s["grads"][3 * i + 1][zero[0]] != 0
    for name, (inp, fx, s) in steps.items():   # dc sums to zero against 1 and against xhat: the two batch terms
        for i in (1, 2, 3):
            dc = s[f"dc{i}"]
            assert np.abs(dc.sum(axis=(0, 2, 3))).max() <= 1e-12 * max(np.abs(dc).max(), 1e-30) * dc[:, 0].size, (name, i)
        if float(fx["p"]) > 0:                 # a dropped plane of a channel kept in another frame: exact zeros in y1,
            mask = fx["mask"]                  # while its dc is not zero
            n, c = np.argwhere((mask == 0) & mask.any(axis=0)[None])[0]
            assert not s["y1"][n, c].any() and s["dc1"][n, c].any()
    inp, fx, s = steps["B_p20"]                # in batch mode the frames of a query without negatives still get gradients
    assert not s["dvlad"][1].any() and s["dx3"][1].any()


@pytest.mark.parametrize("name", ["A_p20", "E_p20"])
def test_oracle_against_finite_differences(name):
    """Central differences of the float64 loss: six entries of every parameter and of the three inputs dx is formed for,
    with the fixture's mask held fixed.  |fd - g| <= 1e-6 max|g| + 1e-10: the truncation error of h = 1e-5 on a loss of
    order 1 is about h^2 = 1e-10 and the rounding error 1e-16 / h = 1e-11.  Without the terms through the batch mean and
    variance the gradients of the conv weights are off by more than 1e-2 of their largest entry (asserted below, so that
    this test is known to see them)."""
    case = br.FIXTURES[name][0]
    inp = hr.make_inputs(case)
    drop = br.load_fixture(name)["mask"]
    params = [p.astype(np.float64) for p in inp["params"]]
    args = (inp["B"], inp["counts"], inp["slope"], drop)
    s = br.step_gradients(inp["feat"], params, inp["stats"], *args)
    rng = np.random.default_rng(5)
    h = 1e-5
    worst = 0.0
    for i, g in enumerate(s["grads"]):
        g = np.asarray(g).reshape(params[i].shape)
        for _ in range(6):
            idx = tuple(int(rng.integers(0, n)) for n in g.shape)
            keep = params[i][idx]
            params[i][idx] = keep + h
            up = br.loss_from(inp["feat"], 0, params, *args)
            params[i][idx] = keep - h
            dn = br.loss_from(inp["feat"], 0, params, *args)
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
            up = br.loss_from(x, start, params, *args[:3], None)       # (the mask acts inside layer 0 only)
            x[idx] = keep - h
            dn = br.loss_from(x, start, params, *args[:3], None)
            x[idx] = keep
            err = abs((up - dn) / (2 * h) - g[idx]) / (1e-6 * np.abs(g).max() + 1e-10)
            worst = max(worst, err)
            assert err <= 1.0, (key, idx, (up - dn) / (2 * h), g[idx])
    print(f"{name}: finite differences {worst:.3f} of the bound")
    # the same dy through the frozen-statistics backward (no mean / variance terms) is a different gradient
    x, y, c, mean, var, invstd = br.head_forward(inp["feat"], params, inp["slope"], drop)["acts"][2]
    frozen = hr.cbr_backward(x, params[6], params[7] * invstd, mean, invstd, inp["slope"], y, c, s["dx_netvlad"], need_dx=False)[0]
    assert hr.rel_err(frozen, s["grads"][6]) > 1e-2


def test_running_statistics_use_the_unbiased_variance(steps):
    inp, fx, s = steps["E_p20"]
    M = 18
    for i in (1, 2, 3):
        rm0, rv0 = (np.asarray(t, np.float64) for t in inp["stats"][i - 1])
        assert np.abs(s[f"rmean{i}"] - (0.9 * rm0 + 0.1 * s[f"mean{i}"])).max() <= 1e-15
        assert np.abs(s[f"rvar{i}"] - (0.9 * rv0 + 0.1 * s[f"var{i}"] * M / (M - 1))).max() <= 1e-15
        biased = 0.9 * rv0 + 0.1 * s[f"var{i}"]
        assert np.abs(hr.stored(biased) - fx[f"rvar{i}"]).max() > 1e-4        # M = 18: the two differ by 1 / 17 of 0.1 var


def test_bounds_come_from_the_fixtures():
    b = br.bounds()
    print("bounds", b)
    for k in br.QUANTITIES:
        e = max(float(br.load_fixture(n)["err32_" + k]) for n in br.FIXTURES)
        assert np.isfinite(e) and e > 0
        assert b[k] == max(8.0 * e, 16.0 * 2.0 ** -24)
        assert b[k] < 1e-3                                      # far below a missing term's 1e-2
    assert br.loss_bound(0.25, b) >= 16 * 2.0 ** -25


def test_trajectory_matches_the_fixture():
    name = br.TRAJECTORY
    inp = hr.make_inputs(br.FIXTURES[name][0])
    fx = br.load_fixture(name)
    drops = fx["masks"]
    assert drops.shape == (hr.TRAJECTORY_STEPS, inp["N"], inp["C"]) and np.array_equal(drops[0], fx["mask"])
    assert any(not np.array_equal(drops[0], d) for d in drops[1:])            # a fresh mask per step
    losses, kept, kept_stats, _ = br.trajectory(inp, drops)
    assert np.abs(losses - fx["losses"]).max() <= 1e-10
    for i, p in enumerate(kept):
        assert np.abs(hr.stored(p) - fx[f"p{i}_after"]).max() <= 1e-10, hr.PARAMS[i]
    for i, (m, v) in enumerate(kept_stats, 1):
        assert np.abs(hr.stored(m) - fx[f"rmean{i}_after"]).max() <= 1e-10
        assert np.abs(hr.stored(v) - fx[f"rvar{i}_after"]).max() <= 1e-10
    assert float(fx["err32_losses"]) <= 1e-5 and float(fx["err32_rstats_after"]) <= 1e-5


# ---- the draw ----------------------------------------------------------------------------------------------------------
def test_draw_restatement_is_self_consistent():
    assert br.mix(0) == 0 and br.mix(1) == 0x5692161D100B05E5         # splitmix64's finaliser: fixed point 0, and of 1
    a = br.dropout_scale(6, 16, 0.2, 7, 3, 1)
    assert np.array_equal(a, br.dropout_scale(6, 16, 0.2, 7, 3, 1))
    assert set(np.unique(a)) <= {np.float32(0), np.float32(1.25)} and a.dtype == np.float32
    for other in ((8, 3, 1), (7, 4, 1), (7, 3, 2)):                   # every counter enters
        assert not np.array_equal(a, br.dropout_scale(6, 16, 0.2, *other))
    assert np.array_equal(br.dropout_scale(8, 16, 0.2, 7, 3, 1)[:6], a)      # a (frame, channel)'s draw is its own
    assert (br.dropout_scale(4, 16, 0.0, 7, 3, 1) == 1).all()         # p = 0 keeps everything, unscaled
    # the threshold in integers is the comparison u >= p in double
    for p in (0.2, 0.5, 1e-3, 0.999):
        t = p * 2.0 ** 53
        thr = int(t) if t == int(t) else int(t) + 1
        assert thr * 2.0 ** -53 >= p > (thr - 1) * 2.0 ** -53
    share = float((br.dropout_scale(64, 128, 0.2, 11, 1, 1) == 0).mean())
    assert abs(share - 0.2) <= 5 * np.sqrt(0.2 * 0.8 / (64 * 128)), share


# ---- argument checks: nothing below may reach the library -------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ht._lib, "load", boom)


def _layer(N=2, Cin=16, Cout=32, H=3, W=4):
    return (torch.zeros(N, Cin, H, W), torch.zeros(Cout, Cin, 3, 3), torch.zeros(Cout), torch.zeros(N, Cout, H, W), torch.zeros(N, Cout))


def test_cpu_tensors_raise(no_library):
    x, w, v, m, d = _layer()
    with pytest.raises(RuntimeError, match="CPU tensors"):
        ht.cbr_forward_batch(x, w, v, v)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        ht.cbr_backward_batch(x, w, v, v, v, m, m, m)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ht.dropout2d_scale(2, 16, 0.2, 0, 1, 1, "cpu")


def test_bad_arguments_raise(no_library, monkeypatch):
    monkeypatch.setattr(ht._dev, "require_device", lambda name, t, hint="": t)       # shapes, on a box without a device
    x, w, v, m, d = _layer()
    one = torch.zeros(1, 16, 1, 1)
    for bad in ((x, w, v[:16], v), (x, w, v, v.double()), (x[0], w, v, v), (torch.zeros(2, 24, 3, 4), torch.zeros(32, 24, 3, 3), v, v),
                (one, w, v, v)):                                                      # M = 1
        with pytest.raises(ValueError):
            ht.cbr_forward_batch(*bad)
    for kw in ({"eps": -1.0}, {"eps": float("nan")}, {"momentum": 1.5}, {"momentum": -0.1}, {"slope": 1.0}, {"drop": d[:1]},
               {"drop": d.double()}, {"running": (v[:16], v)}, {"running": (v, v.double())},
               {"running": (torch.zeros(64)[::2], v)}):
        with pytest.raises(ValueError):
            ht.cbr_forward_batch(x, w, v, v, **kw)
    for bad in ((x, w, v, v, v, m[:1], m, m), (x, w, v[:8], v, v, m, m, m), (x, w, v, v, v, m, m, m.double()),
                (one, w, v, v, v, torch.zeros(1, 32, 1, 1), torch.zeros(1, 32, 1, 1), torch.zeros(1, 32, 1, 1))):
        with pytest.raises(ValueError):
            ht.cbr_backward_batch(*bad)
    with pytest.raises(ValueError):
        ht.cbr_backward_batch(x, w, v, v, v, m, m, m, drop=d[:, :16])
    for bad in ((0, 16, 0.2, 0, 1, 1), (2, 0, 0.2, 0, 1, 1), (2, 16, 1.0, 0, 1, 1), (2, 16, -0.1, 0, 1, 1), (2, 16, 0.2, -1, 1, 1),
                (2, 16, 0.2, 0, -1, 1), (2, 16, 0.2, 0, 2 ** 32, 1), (2, 16, 0.2, 0, 1, -1), (2, 16, 0.2, 2 ** 64, 1, 1)):
        with pytest.raises(ValueError):
            ht.dropout2d_scale(*bad, "cuda:0")


def test_trainer_settings(no_library):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    model = tiny_factory("S", 28)
    t = ht.VPRHeadTrainer(model)
    assert (t.bn, t.dropout, t.seed) == ("running", 0.0, 0)
    t = ht.VPRHeadTrainer(model, bn="batch", dropout=0.2, seed=5)
    assert (t.bn, t.dropout, t.seed) == ("batch", 0.2, 5)
    assert ht.VPRHeadTrainer(model, dropout=0.2).bn == "running"          # the other half of the reference's mode alone
    for kw in ({"bn": "eval"}, {"dropout": 1.0}, {"dropout": -0.1}, {"seed": -1}):
        with pytest.raises(ValueError):
            ht.VPRHeadTrainer(model, **kw)
    model.vlad_head.convlad2.bn.momentum = None
    ht.VPRHeadTrainer(model)                                              # running statistics: momentum is not read
    with pytest.raises(ValueError, match="momentum"):
        ht.VPRHeadTrainer(model, bn="batch")
    model.vlad_head.convlad2.bn.momentum = 0.1
    model.with_drop = False
    ht.VPRHeadTrainer(model, bn="batch")
    with pytest.raises(ValueError, match="with_drop"):
        ht.VPRHeadTrainer(model, bn="batch", dropout=0.2)
