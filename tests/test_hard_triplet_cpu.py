"""The batch-hard triplet loss and the trainers' view step without a GPU: the float64 numpy oracle (hard_triplet_ref) against
the reference's fixtures (tests/golden/hard_triplet/, written by tools/make_hard_triplet_golden.py), against central
differences and against a plain torch restatement of the formulas; the margin quirk; and the argument checks of the C call
(refused on the host before any launch, so they run here on made-up addresses) and of the Python wrappers.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import hard_triplet_ref as tr
from nano_vs_slam_amd import _lib, vlad_training as vt, vpr_head_training as ht

LOSS_FIXTURES = [(n, m) for n in tr.LOSS_CASES for m in tr.MODES]


def _margin(mode):
    return tr.QUIRK_MARGIN if mode == "hardest" else tr.BATCH_ALL_MARGIN


# ---- 1. the oracle against the reference's fixtures ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", LOSS_FIXTURES)
def test_oracle_equals_the_reference_fixture(name, mode):
    fx = tr.load_fixture(f"loss_{name}_{mode}")
    M, dim, _, noise, seed, squared = tr.LOSS_CASES[name]
    assert int(fx["max_stored"]) == tr.MAX_STORED and int(fx["seed"]) == seed and float(fx["noise"]) == noise and bool(fx["squared"]) == squared
    assert float(fx["margin"]) == _margin(mode)
    emb, labels = tr.make_loss_inputs(name)
    assert emb.shape == (M, dim) and emb.dtype == np.float32
    assert np.abs(np.linalg.norm(emb.astype(np.float64), axis=1) - 1).max() < 1e-6
    r = tr.hard_triplet(emb, labels, _margin(mode), mode == "hardest", squared)
    assert abs(r["loss"] - float(fx["loss"])) <= 1e-10
    assert np.abs(tr.stored(r["demb"]) - fx["demb"]).max() <= 1e-10
    assert np.array_equal(r["stats"], fx["stats"])


def test_fixtures_are_what_they_are_for():
    for name in ("B", "C", "D"):
        emb, labels = tr.make_loss_inputs(name)
        r = tr.hard_triplet(emb, labels)
        M = emb.shape[0]
        assert M / 4 <= r["stats"][0] <= 3 * M / 4, (name, r["stats"])
        for hardest in (True, False):
            r = tr.hard_triplet(emb, labels, 0.1, hardest)
            own = tr.own_error(emb)
            assert tr.hinge_gap(r) >= 100 * own and tr.hardest_gaps(emb, labels) >= 100 * own
    emb, labels = tr.make_loss_inputs("E")
    r = tr.hard_triplet(emb, labels)
    assert r["stats"][1] == 1 and list(labels).count(2) == 1
    emb, labels = tr.make_loss_inputs("F")
    assert np.array_equal(emb[0].view(np.uint32), emb[1].view(np.uint32))
    r = tr.hard_triplet(emb, labels)
    assert r["stats"][3] == 2 and r["d"][0, 1] == 0 and r["d"][1, 0] == 0
    emb, labels = tr.make_loss_inputs("G")
    r = tr.hard_triplet(emb, labels)
    assert r["loss"] == 0.1 and not r["demb"].any() and list(r["stats"]) == [2, 0, 2, 0]       # plus and minus cancel
    r = tr.hard_triplet(emb, labels, 0.1, False)
    assert r["loss"] == 0.0 and not r["demb"].any() and list(r["stats"]) == [0, 0, 2, 0]


@pytest.mark.parametrize("case", list(tr.TRAINER_CASES))
@pytest.mark.parametrize("batch", [False, True])
def test_head_view_step_oracle_equals_the_reference_fixture(case, batch):
    fx = tr.load_fixture(f"head_{case}_{'batch' if batch else 'running'}")
    inp = tr.make_trainer_inputs(case)
    drops = [tuple(m) for m in fx["masks"]] if batch else None
    s = tr.head_views_gradients(inp["feat"], inp["feat_aug"], inp["params"], inp["stats"], inp["slope"], batch, drops[0] if batch else None)
    assert abs(s["loss"] - float(fx["loss"])) <= 1e-10 and np.array_equal(s["stats"], fx["stats"])
    for k in ("vlad", "dvlad", "y3"):
        assert np.abs(tr.stored(s[k]) - fx[k]).max() <= 1e-10, k
    for i, g in enumerate(s["grads"]):
        assert np.abs(tr.stored(g) - fx[f"g{i}"]).max() <= 1e-10, tr.hr.PARAMS[i]
    steps = tr.BATCH_STEPS if batch else tr.RUNNING_STEPS
    losses, params, stats, _ = tr.head_views_trajectory(inp, steps, batch, drops)
    assert np.abs(losses - fx["losses"]).max() <= 1e-10
    for i, p in enumerate(params):
        assert np.abs(tr.stored(p) - fx[f"p{i}_after"]).max() <= 1e-10, tr.hr.PARAMS[i]
    if batch:
        assert fx["masks"].shape == (steps, 2, tr.PAIRS, inp["C"])
        assert not np.array_equal(fx["masks"][0, 0], fx["masks"][0, 1])         # each view drew its own mask
        for i, (m, v) in enumerate(s["rstats"], 1):
            assert np.abs(m - fx[f"rstats_mean{i}"]).max() <= 1e-10 and np.abs(v - fx[f"rstats_var{i}"]).max() <= 1e-10
        for i, (m, v) in enumerate(stats, 1):
            assert np.abs(m - fx[f"rstats_after_mean{i}"]).max() <= 1e-10 and np.abs(v - fx[f"rstats_after_var{i}"]).max() <= 1e-10
        # the running statistics moved twice, plain view first: one move by either view alone is another number
        once = tr.br.step_gradients(inp["feat"], inp["params"], inp["stats"], 1, (1,), inp["slope"], drops[0][0])
        assert np.abs(once["rmean1"] - fx["rstats_mean1"]).max() > 1e-4


@pytest.mark.parametrize("case", list(tr.TRAINER_CASES))
def test_netvlad_view_step_oracle_equals_the_reference_fixture(case):
    fx = tr.load_fixture(f"netvlad_{case}")
    inp = tr.make_trainer_inputs(case)
    K, Cc = inp["K"], inp["C"]
    s = tr.netvlad_views_gradients(inp["enc"], inp["enc_aug"], inp["params"][9].reshape(K, Cc), inp["params"][10])
    assert abs(s["loss"] - float(fx["loss"])) <= 1e-10 and np.array_equal(s["stats"], fx["stats"])
    for k in ("vlad", "dvlad", "dW", "dcent"):
        assert np.abs(tr.stored(s[k]) - fx[k]).max() <= 1e-10, k
    losses, W, cent, _ = tr.netvlad_views_trajectory(inp, tr.RUNNING_STEPS)
    assert np.abs(losses - fx["losses"]).max() <= 1e-10
    assert np.abs(tr.stored(W) - fx["W_after"]).max() <= 1e-10 and np.abs(tr.stored(cent) - fx["cent_after"]).max() <= 1e-10


# ---- 2. the oracle against central differences and against torch ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "E", "H"])
@pytest.mark.parametrize("hardest", [True, False])
def test_oracle_against_central_differences(name, hardest):
    """Eight entries of emb, away from ties (the fixtures' gaps are >= 1e-4, the step moves a distance by <= 1e-6):
    |fd - g| <= 1e-6 max|g| + 1e-9; the truncation error of h = 1e-6 on a loss of order 0.1 is below 1e-10."""
    emb, labels = tr.make_loss_inputs(name)
    squared = tr.LOSS_CASES[name][5]
    x = emb.astype(np.float64)
    r = tr.hard_triplet(x, labels, 0.1, hardest, squared, weight=0.7)
    rng = np.random.default_rng(5)
    h = 1e-6
    for _ in range(8):
        i, k = int(rng.integers(0, x.shape[0])), int(rng.integers(0, x.shape[1]))
        up, dn = x.copy(), x.copy()
        up[i, k] += h
        dn[i, k] -= h
        fd = (tr.hard_triplet(up, labels, 0.1, hardest, squared, weight=0.7)["loss"] - tr.hard_triplet(dn, labels, 0.1, hardest, squared, weight=0.7)["loss"]) / (2 * h)
        assert abs(fd - r["demb"][i, k]) <= 1e-6 * np.abs(r["demb"]).max() + 1e-9, (i, k, fd, r["demb"][i, k])


@pytest.mark.parametrize("name", list(tr.LOSS_CASES))
@pytest.mark.parametrize("hardest", [True, False])
def test_oracle_against_a_plain_torch_restatement(name, hardest):
    emb, labels = tr.make_loss_inputs(name)
    squared = tr.LOSS_CASES[name][5]
    x = torch.from_numpy(emb).double().requires_grad_(True)
    loss = tr.torch_hard_triplet(x, torch.from_numpy(labels), 0.25, hardest, squared, weight=1.5)
    loss.backward()
    r = tr.hard_triplet(emb, labels, 0.25, hardest, squared, weight=1.5)
    assert abs(float(loss.detach()) - r["loss"]) <= 1e-10
    assert np.abs(x.grad.numpy() - r["demb"]).max() <= 1e-9


def test_ties_take_the_lowest_index_and_single_rows():
    # two negatives at exactly the same distance from anchor 0: column 2 wins over column 3
    x = np.zeros((4, 4))
    x[0], x[1], x[2], x[3] = (1, 0, 0, 0), (-0.6, 0, 0, 0.8), (0, 1, 0, 0), (0, 0, 1, 0)
    r = tr.hard_triplet(x, [0, 0, 1, 2], 1.0)
    assert r["d"][0, 2] == r["d"][0, 3] and r["picks"][0][1] == 2 and r["w"][0, 2] < 0 and r["w"][0, 3] == 0
    r = tr.hard_triplet(np.ones((1, 5)), [7], 0.3, weight=2.0)
    assert r["loss"] == pytest.approx(0.6) and not r["demb"].any() and list(r["stats"]) == [1, 1, 1, 0]
    r = tr.hard_triplet(x, [0, 0, 1, 2], 1.0, weight=0.0)
    assert r["loss"] == 0 and not r["demb"].any()


# ---- 3. the margin quirk ------------------------------------------------------------------------------------------------------------
def test_the_class_reproduces_the_margin_quirk(monkeypatch):
    """HardTripletLoss(margin=0.5, hardest=True) equals margin=0.9: the hardest branch uses 0.1 whatever margin says; the
    batch-all branch reads its margin."""
    seen = []

    def fake(emb, labels, margin=0.1, hardest=True, squared=False, weight=1.0, scratch=None):
        seen.append((margin, hardest, squared, weight))
        r = tr.hard_triplet(emb.numpy(), labels.numpy(), margin, hardest, squared, weight)
        return torch.tensor(r["loss"], dtype=torch.float64), torch.from_numpy(r["demb"]), torch.from_numpy(r["stats"])

    from nano_vs_slam_amd import train_ops
    assert vt.HardTripletLoss is train_ops.HardTripletLoss and vt.hard_triplet_loss is train_ops.hard_triplet_loss
    monkeypatch.setattr(train_ops, "hard_triplet_loss", fake)      # where the class looks its call up
    emb, labels = (torch.from_numpy(a) for a in tr.make_loss_inputs("B"))
    a, b = vt.HardTripletLoss(margin=0.5, hardest=True), vt.HardTripletLoss(margin=0.9, hardest=True)
    la, lb = a(emb, labels), b(emb, labels)
    assert float(la) == float(lb) == pytest.approx(float(tr.load_fixture("loss_B_hardest")["loss"]), abs=1e-12)
    assert torch.equal(a.grad, b.grad) and a.stats is not None and a.margin == 0.5 and b.margin == 0.9
    c, d = vt.HardTripletLoss(margin=0.5), vt.HardTripletLoss(margin=0.9)
    assert float(c(emb, labels)) != float(d.forward(emb, labels))
    assert seen == [(0.1, True, False, 1.0)] * 2 + [(0.5, False, False, 1.0), (0.9, False, False, 1.0)]
    assert vt.HardTripletLoss().hardest is False and vt.HardTripletLoss().margin == 0.1        # the reference's defaults


# ---- 4. the argument checks ---------------------------------------------------------------------------------------------------------
ARG, UNSUPPORTED = -1, -2


def test_c_call_refuses_before_launching():
    lib = _lib.load()
    p, null, odd = C.c_void_p(4096), None, C.c_void_p(4096 + 2)      # never dereferenced: every call below is refused
    fn, size = lib.kp2d_hard_triplet_loss, lib.kp2d_hard_triplet_scratch_bytes

    def f(M=12, dim=64, margin=0.1, flags=1, weight=1.0, emb=p, labels=p, loss=p, demb=p, stats=p, scratch=p, nbytes=1 << 24):
        return fn(emb, labels, M, dim, margin, flags, weight, loss, demb, stats, scratch, nbytes, null)

    assert f(M=0) == ARG and f(M=-3) == ARG and f(dim=0) == ARG
    assert f(M=513) == UNSUPPORTED and b"512" in lib.kp2d_last_error()
    assert f(margin=-0.1) == ARG and f(margin=float("nan")) == ARG and f(margin=float("inf")) == ARG
    assert f(weight=float("nan")) == ARG and f(weight=float("-inf")) == ARG
    assert f(flags=4) == ARG and f(flags=7) == ARG
    for k in ("emb", "labels", "loss", "demb", "stats", "scratch"):
        assert f(**{k: null}) == ARG and b"null" in lib.kp2d_last_error(), k
    for k in ("emb", "labels", "loss", "demb", "stats", "scratch"):
        assert f(**{k: odd}) == ARG and b"aligned" in lib.kp2d_last_error(), k
    assert f(stats=C.c_void_p(4096 + 4)) == ARG and f(scratch=C.c_void_p(4096 + 8)) == ARG
    assert size(0, 8) == 0 and size(4, 0) == 0 and size(513, 8) == 0
    for M in (1, 2, 130, 512):
        need = size(M, 4096)
        assert need >= 8 * M * M + 28 * M and need % 256 == 0
        assert f(M=M, nbytes=need - 1) == ARG and b"scratch" in lib.kp2d_last_error()
    assert size(12, 8) == size(12, 4096)


def test_wrapper_refuses_bad_arguments(monkeypatch):
    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(vt._lib, "load", boom)
    emb, labels = torch.zeros(6, 8), torch.arange(6)
    with pytest.raises(ValueError, match="device tensor"):
        vt.hard_triplet_loss(emb, labels)

    class OnDevice(torch.Tensor):          # shapes and types, on a box without a device
        @property
        def device(self):
            return torch.device("cuda:0")

    dev = lambda t: t.as_subclass(OnDevice)      # noqa: E731
    with pytest.raises(ValueError, match="device tensor"):
        vt.hard_triplet_loss(dev(emb), labels)
    for bad in (torch.zeros(6, 8, dtype=torch.float64), torch.zeros(6), torch.zeros(2, 3, 8), torch.zeros(0, 8), torch.zeros(6, 0)):
        with pytest.raises(ValueError, match=r"float32 \[M, dim\]"):
            vt.hard_triplet_loss(dev(bad), dev(labels))
    for bad in (torch.zeros(6), torch.arange(5), torch.zeros(6, 1, dtype=torch.int64), torch.zeros(6, dtype=torch.bool)):
        with pytest.raises(ValueError, match="integer tensor of length 6"):
            vt.hard_triplet_loss(dev(emb), dev(bad))
    with pytest.raises(ValueError, match="at most 512"):
        vt.hard_triplet_loss(dev(torch.zeros(513, 4)), dev(torch.arange(513)))
    for kw in ({"margin": -1.0}, {"margin": float("nan")}, {"weight": float("inf")}):
        with pytest.raises(ValueError, match="margin must be finite"):
            vt.hard_triplet_loss(dev(emb), dev(labels), **kw)


def test_view_labels():
    got = vt.view_labels(4, "cpu")
    assert got.dtype == torch.int32 and got.tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
    assert np.array_equal(tr.view_labels(4), got.numpy())


def test_trainers_refuse_bad_views(monkeypatch):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory

    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(vt._lib, "load", boom)
    model = tiny_factory("S", 28)
    head, layer = ht.VPRHeadTrainer(model), vt.NetVLADTrainer(model)
    assert head.ht_stats is None and layer.ht_stats is None
    f = torch.zeros(3, 64, 6, 8)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        head.step_views_features(f, f)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        layer.step_views_encoded(f, f)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        head.step_views(torch.zeros(2, 3, 64, 96), torch.zeros(2, 3, 64, 96))
    monkeypatch.setattr(vt._dev, "require_device", lambda name, t, hint="": t)
    with pytest.raises(ValueError, match="one shape"):
        head.step_views_features(f, f[:2])
    with pytest.raises(ValueError, match="feat_aug must be float32"):
        head.step_views_features(f, f.double())
    with pytest.raises(ValueError, match="at most 256 pairs"):
        head.step_views_features(torch.zeros(257, 64, 1, 1), torch.zeros(257, 64, 1, 1))
    with pytest.raises(ValueError, match=r"drop must be \(mask, mask_aug\)"):
        head.step_views_features(f, f, drop=(torch.ones(3, 64),))
    with pytest.raises(ValueError, match="both be float32"):
        layer.step_views_encoded(f, f[:2])
    with pytest.raises(ValueError, match="both be"):
        layer.step_views(torch.zeros(2, 3, 64, 96), torch.zeros(3, 3, 64, 96))
