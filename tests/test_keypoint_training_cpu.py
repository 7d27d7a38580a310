"""The float64 oracle of the keypoint heads' training step (keypoint_training_ref) against the fixtures written from the
reference's own KeypointNetwithIOLoss.forward and heads (to 1e-10 on every stored entry, 2^-23 relative on the total, which the
reference rounds to float32) and against central finite differences; what the cases are for; the argument checks of the
Python layer; the new signatures against the header: everything here runs without a device."""
import os
import re

import numpy as np
import pytest
import torch

import keypoint_training_ref as kr
from conftest import ROOT
from nano_vs_slam_amd import _lib, keypoint_training as kt, seg_training as st


def _oracle(inp, **kw):
    return kr.keypoint_loss(inp["tgt"], inp["src"], inp["hom"], inp["H"], inp["W"], inp["cell"], inp["weights"], **kw)


@pytest.fixture(scope="module")
def losses():
    return {name: (kr.make_loss_inputs(name), _oracle(kr.make_loss_inputs(name))) for name in kr.LOSS_CASES}


@pytest.mark.parametrize("name", list(kr.LOSS_CASES))
def test_loss_oracle_equals_the_reference_fixture(losses, name):
    inp, s = losses[name]
    fx = kr.load_fixture(name)
    lw, dw, sw, kw = inp["weights"]
    assert int(fx["max_stored"]) == kr.MAX_STORED and int(fx["seed"]) == kr.seed_of(name) and np.array_equal(fx["weights"], inp["weights"])
    worst = max(abs(lw * s["loc"] - float(fx["loc_loss"])), abs(s["metric"] - float(fx["metric_loss"])), abs(sw * s["usp"] - float(fx["usp_loss"])),
                abs(s["con"] - float(fx["con"])), abs(s["recall"] - float(fx["recall"])), abs(s["usp_abs"] - float(fx["usp_abs"])))
    for k in kr.GRADS:
        assert fx[k].size <= kr.MAX_STORED
        worst = max(worst, np.abs(kr.stored(s[k]) - fx[k]).max())
    print(f"case {name}: oracle vs fixture max|diff| {worst:.2e}; total {abs(s['loss'] - float(fx['total'])) / abs(float(fx['total'])):.2e}")
    assert worst <= 1e-10
    assert abs(s["loss"] - float(fx["total"])) <= 2.0 ** -23 * abs(float(fx["total"]))       # the reference's total is a float32
    assert (s["M"], s["n"], s["hits"]) == (int(fx["M"]), int(fx["n"]), int(fx["hits"]))


def test_cases_are_what_they_are_for(losses):
    n_of = {name: (c[1] - 2) * (c[2] - 2) for name, c in kr.LOSS_CASES.items()}
    assert (n_of["A"], n_of["B"], n_of["C"], n_of["D"]) == (20, 35, 234, 16)
    assert losses["A"][1]["n"] == 20 and losses["A"][1]["metric"] > 0                  # n = 20 is NOT skipped
    d = losses["D"][1]
    assert d["n"] == 0 and d["metric"] == 0.0 and not d["dfeat_t"].any() and not d["dfeat_s"].any()
    assert d["loc"] > 0 and d["usp"] != 0 and d["con"] > 0 and d["dshift_s"].any() and d["dscore_t"].any()
    c = losses["C"][1]
    outside = (np.abs(c["q"]["wn"]) > 1).any(axis=0)
    assert outside[1].sum() >= 50 and (c["d"][1] >= kr.VALID_DIST).sum() >= 50        # the strong homography of frame 1
    assert np.isfinite(c["dfeat_t"]).all() and c["M"] > 300
    assert kr.LOSS_CASES["E"][7] != kr.WEIGHTS and kr.LOSS_CASES["E"][7][3] == 0.5
    for name, (inp, s) in losses.items():
        if s["n"]:                                                                     # active and inactive hinges, real negatives
            on = np.concatenate(s["q"]["harg"]) > 0
            assert on.any() and not on.all(), name
        assert 0 < s["M"] <= inp["tgt"]["score"].shape[0] * n_of[name]
        for b in range(inp["hom"].shape[0]):
            if not (name == "C" and b == 1):
                assert np.abs(inp["hom"][b] - np.eye(3)).max() <= 0.05 + 1e-6


def test_recorded_margins():
    """The generator's conditions, as recorded: every fixture's float32 errors are small, and the oracle in float32 takes
    the float64 oracle's decisions."""
    b = kr.bounds()
    assert set(b) == set(kr.LOSS_KEYS) and all(kr.FLOOR <= v < 1e-3 for v in b.values())
    tb = kr.trainer_bounds()
    assert set(tb) == {"losses", "score", "coord", "feat"} | {f"g{i}" for i in range(20)} | {f"p{i}" for i in range(20)}
    assert all(kr.FLOOR <= v < 1e-3 for v in tb.values())
    for name in kr.LOSS_CASES:
        inp = kr.make_loss_inputs(name)
        s64, s32 = _oracle(inp, grads=False), _oracle(inp, dtype=np.float32, grads=False)
        assert (s64["M"], s64["hits"]) == (s32["M"], s32["hits"]) and np.array_equal(s64["a"][s64["valid"]], s32["a"][s64["valid"]])


def test_oracle_against_finite_differences():
    """Central differences of the float64 loss on case B (three entries of each of the six maps) and, through the heads, on
    the trainer case (one entry of every parameter).  |fd - g| <= 1e-6 max|g| + 1e-9: truncation h^2 = 1e-10, rounding
    1e-16 / h = 1e-11 (times the loss's size).  The sampling grids are held fixed, as the reference detaches them.  The loss is
    piecewise smooth; the fixtures' margins keep h = 1e-5 inside a piece."""
    rng = np.random.default_rng(17)
    h = 1e-5
    worst = 0.0
    inp = kr.make_loss_inputs("B")
    inp = {**inp, "tgt": {k: v.astype(np.float64) for k, v in inp["tgt"].items()}, "src": {k: v.astype(np.float64) for k, v in inp["src"].items()}}
    s = _oracle(inp)
    for view, tag in (("tgt", "t"), ("src", "s")):
        for key in ("score", "shift", "feat"):
            g = s[f"d{key}_{tag}"]
            nz = np.argwhere(g != 0)
            for idx in nz[rng.integers(0, len(nz), 3)]:
                idx = tuple(idx)
                keep = inp[view][key][idx]
                inp[view][key][idx] = keep + h
                up = _oracle(inp, grads=False, grids=s["grids"])["loss"]
                inp[view][key][idx] = keep - h
                dn = _oracle(inp, grads=False, grids=s["grids"])["loss"]
                inp[view][key][idx] = keep
                err = abs((up - dn) / (2 * h) - g[idx]) / (1e-6 * np.abs(g).max() + 1e-9)
                worst = max(worst, err)
                assert err <= 1.0, (view, key, idx, (up - dn) / (2 * h), g[idx])
    tinp = kr.make_trainer_inputs()
    params = [p.astype(np.float64) for p in tinp["params"]]
    s = kr.step_gradients(tinp, params)
    for i, g in enumerate(s["grads"]):
        g = np.asarray(g).reshape(params[i].shape)
        for _ in range(1):
            idx = tuple(int(rng.integers(0, n)) for n in g.shape)
            keep = params[i][idx]
            params[i][idx] = keep + h
            up = kr.loss_from(tinp, params, s["grids"])
            params[i][idx] = keep - h
            dn = kr.loss_from(tinp, params, s["grids"])
            params[i][idx] = keep
            err = abs((up - dn) / (2 * h) - g[idx]) / (1e-6 * np.abs(g).max() + 1e-9)
            worst = max(worst, err)
            assert err <= 1.0, (kr.PARAMS[i], idx, (up - dn) / (2 * h), g[idx])
    print(f"finite differences: {worst:.3f} of the bound")


def test_trainer_oracle_equals_the_reference_fixture():
    inp, fx = kr.make_trainer_inputs(), kr.load_trainer()
    assert int(fx["seed"]) == kr.seed_of("T") and float(fx["lr"]) == kr.LR
    s = kr.step_gradients(inp)
    worst = max(np.abs(kr.stored(s[o]) - fx[k]).max() for k, o in (("score", "score"), ("coord", "shift"), ("feat", "feat")))
    for i, g in enumerate(s["grads"]):
        assert np.asarray(g).size == inp["params"][i].size
        worst = max(worst, np.abs(kr.stored(g) - fx[f"g{i}"]).max())
    losses, after = kr.trajectory(inp)
    for t, ps in enumerate(after):
        for i, p in enumerate(ps):
            worst = max(worst, np.abs(kr.stored(p, kr.TRAJ_STORED) - fx[f"p{i}"][t]).max())
    print(f"trainer: oracle vs fixture max|diff| {worst:.2e}")
    assert worst <= 1e-10 and abs(s["recall"] - float(fx["recall"])) <= 1e-12
    assert np.abs(losses - fx["losses"]).max() <= 2.0 ** -23 * np.abs(fx["losses"]).max()
    assert (losses[1:] < losses[:-1]).all() and s["n"] == 60
    part = kr.step_gradients(inp, train=("score", "loc"))
    assert all(g is None for g in part["grads"][10:]) and all(np.array_equal(a, b) for a, b in zip(part["grads"][:10], s["grads"][:10]))


def test_loss_deviations_of_the_oracle():
    inp = kr.make_loss_inputs("B")
    far = {**inp, "hom": inp["hom"].copy()}
    far["hom"][:, 0, 2] += 3.0
    s = _oracle(far)                                                                    # M = 0: no NaN, loc and usp 0
    assert s["M"] == 0 and s["loc"] == 0.0 and s["usp"] == 0.0 and np.isfinite(s["loss"])
    assert all(np.isfinite(s[k]).all() for k in kr.GRADS) and not s["dshift_t"].any() and not s["dshift_s"].any()
    wide = _oracle(inp, relax=1000.0)                                                   # no admissible negative: the overall nearest
    base = _oracle(inp)
    assert wide["hits"] == base["hits"] and wide["metric"] != base["metric"] and np.isfinite(wide["dfeat_t"]).all()


# ---- argument checks: nothing below may reach the library -------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(st._lib, "load", boom)


@pytest.fixture
def shapes_only(no_library, monkeypatch):
    monkeypatch.setattr("nano_vs_slam_amd.train_ops._is_device", lambda t: True)     # shapes, on a box without a device


def _model(config="S", **kw):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import KP2DTinyV2, get_config
    return KP2DTinyV2(**get_config(config, **kw), nClasses=19)


def _views(B=2, Hc=6, Wc=7, C=16):
    mk = lambda: {"score": torch.zeros(B, 1, Hc, Wc), "coord": torch.zeros(B, 2, Hc, Wc), "feat": torch.zeros(B, C, Hc, Wc)}
    return mk(), mk(), torch.eye(3).repeat(B, 1, 1)


def test_keypoint_loss_refusals(shapes_only):
    out, aug, hom = _views()
    size = (48, 56)
    for bad in (hom.double(), hom[:1], hom[:, :2], hom.reshape(2, 9), None):
        with pytest.raises(ValueError, match="homography"):
            kt.keypoint_loss(out, aug, bad, size, 8)
    with pytest.raises(ValueError):
        kt.keypoint_loss({**out, "score": out["score"].double()}, aug, hom, size, 8)
    with pytest.raises(ValueError):
        kt.keypoint_loss({k: v for k, v in out.items() if k != "feat"}, aug, hom, size, 8)
    with pytest.raises(ValueError):
        kt.keypoint_loss(out, {**aug, "coord": aug["coord"][:, :1]}, hom, size, 8)
    for C in (8, 24, 272):
        o, a, _ = _views(C=C)
        with pytest.raises(ValueError, match="multiple of 16"):
            kt.keypoint_loss(o, a, hom, size, 8)
    o, a, _ = _views(Hc=300, Wc=300)
    with pytest.raises(ValueError, match="65536"):
        kt.keypoint_loss(o, a, hom, size, 8)
    for kw in ({"loc_weight": -1.0}, {"score_weight": float("inf")}, {"keypoint_weight": float("nan")}, {"relax_field": -1}):
        with pytest.raises(ValueError, match="weights"):
            kt.keypoint_loss(out, aug, hom, size, 8, **kw)
    with pytest.raises(ValueError):
        kt.keypoint_loss(out, aug, hom, (1, 56), 8)


def test_cpu_tensors_raise(no_library):
    out, aug, hom = _views()
    with pytest.raises(ValueError, match="no CPU path"):
        kt.keypoint_loss(out, aug, hom, (48, 56), 8)
    trainer = kt.KeypointHeadTrainer(_model())
    maps = (torch.zeros(2, 64, 4, 6), torch.zeros(2, 64, 8, 12))
    with pytest.raises(ValueError, match="no CPU path"):
        trainer.step_features(maps, maps, hom, (16, 24))
    with pytest.raises(ValueError, match="no CPU path"):
        trainer.forward_features(*maps)
    with pytest.raises(ValueError, match="no CPU path"):
        trainer.step(torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32), hom)


def test_trainer_refusals(shapes_only):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import KP2DTinyV3, get_config
    with pytest.raises(ValueError, match="KeypointHeadTrainer: V3"):
        kt.KeypointHeadTrainer(KP2DTinyV3(**get_config("S", v3=True), nClasses=19))
    with pytest.raises(ValueError, match="KeypointHeadTrainer: .*convtranspose"):
        kt.KeypointHeadTrainer(_model(to_mcu=True))
    with pytest.raises(ValueError, match="KeypointHeadTrainer: desc_head.confAa .*72"):
        kt.KeypointHeadTrainer(_model("N"))                                              # the 72-channel concatenation
    with pytest.raises(ValueError, match="KeypointHeadTrainer: desc_head"):
        kt.KeypointHeadTrainer(_model("N"), train="desc")
    assert len(kt.KeypointHeadTrainer(_model("N"), train=("score", "loc")).parameters()) == 10
    model = _model()
    for train in ((), ("score", "seg"), ("loc", "loc"), "head"):
        with pytest.raises(ValueError, match="train must be"):
            kt.KeypointHeadTrainer(model, train=train)
    for kw in ({"lr": -1.0}, {"betas": (1.0, 0.999)}, {"eps": -1e-8}, {"score_weight": -0.5}, {"descriptor_weight": float("nan")}):
        with pytest.raises(ValueError):
            kt.KeypointHeadTrainer(model, **kw)
    trainer = kt.KeypointHeadTrainer(model)
    named = dict(model.named_parameters())                          # the three heads' parameters, in registration order
    assert [id(p) for p in trainer.parameters()] == [id(named[n]) for n in kr.PARAMS]
    assert sum(len(list(getattr(model, h).parameters())) for h in ("score_head", "loc_head", "desc_head")) == 20
    assert kt.KeypointHeadTrainer(model, train=("desc", "score")).train == ("score", "desc")
    assert len(kt.KeypointHeadTrainer(model, train="loc").parameters()) == 5
    x, skip, hom = torch.zeros(2, 64, 4, 6), torch.zeros(2, 64, 8, 12), torch.eye(3).repeat(2, 1, 1)
    for bad in (hom.double(), hom[:1], hom.reshape(2, 9)):
        with pytest.raises(ValueError, match="homography"):
            trainer.step_features((x, skip), (x, skip), bad, (16, 24))
    with pytest.raises(ValueError):
        trainer.step_features((x, torch.zeros(2, 64, 4, 6)), (x, skip), hom, (16, 24))
    with pytest.raises(ValueError):
        trainer.step_features((x, skip), (x[:1], skip[:1]), hom, (16, 24))
    with pytest.raises(ValueError):
        trainer.step_features(x, skip, hom, (16, 24))
    with pytest.raises(ValueError):
        trainer.forward_features(torch.zeros(2, 32, 4, 6), skip)
    w = model.desc_head.convB.weight
    w.data = w.data.permute(0, 1, 3, 2)                             # a non-contiguous parameter
    assert not w.is_contiguous()
    with pytest.raises(ValueError, match="KeypointHeadTrainer: .*contiguous"):
        trainer.step_features((x, skip), (x, skip), hom, (16, 24))


def test_normalized_homography():
    H, W = 32, 48
    hom = torch.tensor([[[1.1, 0.05, 3.0], [-0.04, 0.95, -2.0], [1e-3, -2e-3, 1.0]]], dtype=torch.float64)
    for invert in (False, True):
        hn = kt.normalized_homography(hom, H, W, invert=invert).double()
        assert hn.dtype == torch.float64 and float(hn[0, 2, 2]) == 1.0
        m = torch.linalg.inv(hom[0]) if invert else hom[0]
        p = torch.tensor([10.0, 20.0, 1.0], dtype=torch.float64)
        q = m @ p
        q = q / q[2]
        pn = torch.tensor([10.0 / ((W - 1) / 2) - 1, 20.0 / ((H - 1) / 2) - 1, 1.0], dtype=torch.float64)
        qn = hn[0] @ pn
        qn = qn / qn[2]
        assert abs(float((qn[0] + 1) * (W - 1) / 2 - q[0])) <= 1e-4 and abs(float((qn[1] + 1) * (H - 1) / 2 - q[1])) <= 1e-4


# ---- the new signatures against the header ------------------------------------------------------------------------------------
NEW = ("kp2d_keypoint_loss_scratch_bytes", "kp2d_keypoint_loss")


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
    for const, value in (("KP2D_KEYPOINT_VALID_DIST", kr.VALID_DIST), ("KP2D_KEYPOINT_MARGIN", kr.MARGIN), ("KP2D_KEYPOINT_MIN_ANCHORS", kr.MIN_ANCHORS)):
        assert float(re.search(r"#define\s+" + const + r"\s+(\S+)", raw).group(1)) == value
    with open(os.path.join(ROOT, "nano-vs-slam_amd", "csrc", "build.py")) as f:
        assert '"keypoint_train.hip"' in f.read()
