"""The head training step on batch statistics with Dropout2d on the device (nano_vs_slam_amd.vpr_head_training:
cbr_forward_batch, cbr_backward_batch, dropout2d_scale, VPRHeadTrainer(bn="batch", dropout=p); csrc/vpr_head_train.hip)
against the float64 outputs of the reference's VPRHead in .train() under torch autograd (tests/golden/vpr_head_bn/, written
by tools/make_vpr_head_bn_golden.py; inputs regenerated from seeds, the reference's dropout mask read from the fixture).  The
fixtures keep a stated stride of every larger array, so the numpy float64 oracle (vpr_head_bn_ref), held to the stored
entries to 1e-10, stands in for the whole arrays.

Error measure: for an array G, E(G) = max|G - G64| / max|G64|; for the loss |loss - loss64|.
Bound: max(8 x the reference's own float32 error of that quantity, 16 x 2^-24), the error being that of the same module run
in float32 on the CPU against its float64 run under the same mask, the maximum over the seven fixtures, per gradient group
and per map as in test_gpu_vpr_head_training.py, and for the batch mean, the biased variance and the two running statistics
(vpr_head_bn_ref.bounds); the loss has a floor of 16 ulp in fp32.  The biased variance is read as 1 / invstd^2 - eps from
the invstd the call returns.  Every test prints the fraction of its bound it used.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import vpr_head_bn_ref as br
from conftest import product_model

hr = br.hr
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAP_TOL = 2e-4        # what test_gpu_parity.py applies to fp32-mode taps (its TOL)
OUTPUTS = ("y1", "y2", "y3", "vlad", "loss", "dvlad", "n_active", "dx_netvlad", "dx3", "dx2") + br.STATS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _run_step(inp, mask):
    """forward, loss, backward on the device as a training step chains them -> dict of device tensors."""
    from nano_vs_slam_amd import vlad_training as vt, vpr_head_training as ht
    K, Cc = inp["K"], inp["C"]
    x = _dev(inp["feat"])
    drop = _dev(mask)
    r, acts = {}, []
    for i in range(3):
        w, gamma, beta = (_dev(inp["params"][3 * i + j]) for j in range(3))
        running = (_dev(inp["stats"][i][0]), _dev(inp["stats"][i][1]))
        d = drop if i == 0 else None
        y, c, mean, invstd = ht.cbr_forward_batch(x, w, gamma, beta, hr.BN_EPS, inp["slope"], d, running, br.MOMENTUM)
        acts.append((x, w, gamma, mean, invstd, y, c, d))
        r[f"y{i + 1}"], r[f"mean{i + 1}"], r[f"var{i + 1}"] = y, mean, 1.0 / (invstd.double() ** 2) - hr.BN_EPS
        r[f"rmean{i + 1}"], r[f"rvar{i + 1}"] = running
        x = y
    W, cent = _dev(inp["params"][9]).view(K, Cc, 1, 1), _dev(inp["params"][10])
    vlad, saved = vt.netvlad_forward(x, W, cent)
    loss, dvlad, n_active = vt.triplet_margin_loss(vlad, inp["B"], inp["counts"], hr.MARGIN)
    dW, dcent = vt.netvlad_backward(x, W, cent, saved, dvlad)
    dy = ht.netvlad_backward_input(x, W, cent, saved, dvlad)
    r.update(vlad=vlad, loss=loss, dvlad=dvlad, n_active=n_active, dx_netvlad=dy, acts=acts)
    grads = [None] * 9 + [dW, dcent]
    for i in (2, 1, 0):
        lx, w, gamma, mean, invstd, y, c, d = acts[i]
        r[f"dy{i + 1}"] = dy
        dw, dgamma, dbeta, dy = ht.cbr_backward_batch(lx, w, gamma, mean, invstd, y, c, dy, inp["slope"], d, need_dx=i > 0)
        grads[3 * i:3 * i + 3] = [dw, dgamma, dbeta]
        if dy is not None:
            r[f"dx{i + 1}"] = dy
    r["grads"] = grads
    return r


@pytest.fixture(scope="module")
def bounds():
    return br.bounds()


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name, (case, p, seed) in br.FIXTURES.items():
        inp = hr.make_inputs(case)
        fx = br.load_fixture(name)
        ref = br.step_gradients(inp["feat"], inp["params"], inp["stats"], inp["B"], inp["counts"], inp["slope"], fx["mask"])
        for k in hr.MAPS + ("vlad", "dvlad") + br.STATS:      # the oracle stands in for the whole arrays: held to the fixture here
            assert np.abs(hr.stored(ref[k]) - fx[k]).max() <= 1e-10, k
        for i, g in enumerate(ref["grads"]):
            assert np.abs(hr.stored(g) - fx[f"g{i}"]).max() <= 1e-10, hr.PARAMS[i]
        assert abs(ref["loss"] - float(fx["loss"])) <= 1e-10 and ref["n_active"] == int(fx["n_active"])
        out[name] = (inp, fx, _run_step(inp, fx["mask"]), ref)
    torch.cuda.synchronize()
    return out


# ---- 1. the chained step against the fixtures ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(br.FIXTURES))
def test_batch_and_running_statistics(runs, bounds, name):
    inp, fx, r, ref = runs[name]
    for k in br.STATS:
        group = k[:-1]
        assert r[k].shape == ref[k].shape
        e = hr.rel_err(_np(r[k]), ref[k])
        print(f"{name}: E({k}) {e:.3e} = {e / bounds[group]:.3f} of {bounds[group]:.3e}")
        assert e <= bounds[group], k


@pytest.mark.parametrize("name", list(br.FIXTURES))
def test_forward_maps(runs, bounds, name):
    inp, fx, r, ref = runs[name]
    for k in ("y1", "y2", "y3"):
        assert r[k].shape == ref[k].shape
        e = hr.rel_err(_np(r[k]), ref[k])
        print(f"{name}: E({k}) {e:.3e} = {e / bounds[k]:.3f} of {bounds[k]:.3e}")
        assert e <= bounds[k]


@pytest.mark.parametrize("name", list(br.FIXTURES))
def test_loss_and_active_count(runs, bounds, name):
    inp, fx, r, ref = runs[name]
    lb = br.loss_bound(ref["loss"], bounds)
    err = abs(float(r["loss"]) - ref["loss"])
    print(f"{name}: loss err {err:.3e} = {err / lb:.3f} of {lb:.3e}; n_active {int(r['n_active'])}")
    assert err <= lb
    assert int(r["n_active"]) == ref["n_active"]


@pytest.mark.parametrize("name", list(br.FIXTURES))
def test_gradients(runs, bounds, name):
    inp, fx, r, ref = runs[name]
    for group, members in hr.GROUPS.items():
        for i in members:
            want = np.asarray(ref["grads"][i])
            got = _np(r["grads"][i]).reshape(want.shape)
            assert r["grads"][i].numel() == inp["params"][i].size
            e = hr.rel_err(got, want)
            print(f"{name}: E(d {hr.PARAMS[i]}) {e:.3e} = {e / bounds[group]:.3f} of {bounds[group]:.3e}")
            assert e <= bounds[group], hr.PARAMS[i]


@pytest.mark.parametrize("name", list(br.FIXTURES))
def test_input_gradients(runs, bounds, name):
    inp, fx, r, ref = runs[name]
    assert "dx1" not in r
    for k in ("dx_netvlad", "dx3", "dx2"):
        assert r[k].shape == ref[k].shape
        e = hr.rel_err(_np(r[k]), ref[k])
        print(f"{name}: E({k}) {e:.3e} = {e / bounds[k]:.3f} of {bounds[k]:.3e}")
        assert e <= bounds[k]


# ---- 2. determinism, dx = NULL, gamma = 0, dropped planes, the two sums of dc ----------------------------------------------
@pytest.mark.parametrize("name", list(br.FIXTURES))
def test_bit_reproducible(runs, name):
    inp, fx, r, _ = runs[name]
    again = _run_step(inp, fx["mask"])
    for k in OUTPUTS:
        assert torch.equal(again[k], r[k]), k
    for i, (a, b) in enumerate(zip(again["grads"], r["grads"])):
        assert torch.equal(a, b), hr.PARAMS[i]


@pytest.mark.parametrize("name", ["B_p20", "C_p0"])
def test_backward_without_dx_has_the_same_bits(runs, name):
    from nano_vs_slam_amd import vpr_head_training as ht
    inp, fx, r, _ = runs[name]
    for i in range(3):
        lx, w, gamma, mean, invstd, y, c, d = r["acts"][i]
        dy = r[f"dy{i + 1}"]
        with_dx = ht.cbr_backward_batch(lx, w, gamma, mean, invstd, y, c, dy, inp["slope"], d, need_dx=True)
        without = ht.cbr_backward_batch(lx, w, gamma, mean, invstd, y, c, dy, inp["slope"], d, need_dx=False)
        assert without[3] is None and with_dx[3].shape == lx.shape
        for a, b, g in zip(with_dx[:3], without[:3], r["grads"][3 * i:3 * i + 3]):
            assert torch.equal(a, b) and torch.equal(a, g)
        if i > 0:
            assert torch.equal(with_dx[3], r[f"dx{i + 1}"])


def test_gamma_zero_channels(runs, bounds):
    """Case E: one channel per layer has gamma = 0 (y constant, dc zero): its dgamma comes from c itself and is held to the
    BatchNorm bound like every other entry; its rows of dw are exactly zero."""
    inp, fx, r, ref = runs["E_p20"]
    for i in range(3):
        ch = int(np.flatnonzero(inp["params"][3 * i + 1] == 0)[0])
        want = ref["grads"][3 * i + 1]
        got = _np(r["grads"][3 * i + 1])
        assert want[ch] != 0
        e = abs(got[ch] - want[ch]) / np.abs(want).max()
        print(f"layer {i + 1} channel {ch}: dgamma {got[ch]:.6e} vs {want[ch]:.6e}, {e / bounds['bn']:.3f} of {bounds['bn']:.3e}")
        assert e <= bounds["bn"]
        assert not r["grads"][3 * i][ch].any()


@pytest.mark.parametrize("name", ["A_p20", "B_p20", "C_p20", "D_p20", "E_p20"])
def test_dropped_planes_are_exact_zeros(runs, name):
    inp, fx, r, _ = runs[name]
    dropped = _dev(fx["mask"]) == 0
    assert dropped.any()
    assert not r["y1"][dropped].any()
    assert r["y1"][~dropped].any()


@pytest.mark.parametrize("shape", [(3, 5, 7, 0.01), (3, 2, 3, 0.0), (2, 9, 13, 0.01)])
def test_dc_sums_vanish_and_a_dropped_channel_has_zero_g(shape):
    """A layer call with identity weights (c = x, and dx = dc exactly: every other product is a multiplication by 0).
    Per channel sum dc vanishes to rounding, and so does sum dc xhat once the one term that is not rounding is taken out: with
    sum xhat^2 = M var / (var + eps) < M the formulas give sum dc xhat = gamma invstd dgamma (1 - sum xhat^2 / M) exactly, about
    eps / var of dgamma (torch's own gradient has it too); it is formed here in float64 and subtracted.  |sum| <= 64 x 2^-24 x A, A = sum |gamma invstd| (|g| + |dbeta| / M +
    |xhat dgamma| / M), the sum of the magnitudes that enter; 64 covers the roundings of one element (a handful), the strided
    fp32 sums behind dbeta and dgamma, and the fp32 error of mean and invstd, which moves sum xhat off zero by a few
    2^-24 M |mean| invstd (|mean| invstd < 2 here).  Without either batch term the sums are of the order of A / 4.
    Channel 3 is dropped in every frame: its g is zero everywhere, so dbeta, dgamma and dw are exact zeros there."""
    from nano_vs_slam_amd import vpr_head_training as ht
    N, H, W, slope = shape
    Cn = 16
    rng = np.random.default_rng(23)
    x = _dev((rng.standard_normal((N, Cn, H, W)) + 0.3 * rng.standard_normal((1, Cn, 1, 1))).astype(np.float32))
    w = torch.zeros(Cn, Cn, 3, 3, device=DEV)
    w[torch.arange(Cn), torch.arange(Cn), 1, 1] = 1.0
    gamma = _dev(rng.uniform(0.5, 1.5, Cn).astype(np.float32))
    beta = _dev((0.2 * rng.standard_normal(Cn)).astype(np.float32))
    mask = np.where(rng.random((N, Cn)) < 0.2, 0.0, 1.25).astype(np.float32)
    mask[:, 3] = 0.0
    mask[:, 5] = 1.25
    mask[0, 5] = 0.0
    drop = _dev(mask)
    dy = _dev(rng.standard_normal((N, Cn, H, W)).astype(np.float32))
    y, c, mean, invstd = ht.cbr_forward_batch(x, w, gamma, beta, hr.BN_EPS, slope, drop)
    assert torch.equal(c, x)
    dw, dgamma, dbeta, dc = ht.cbr_backward_batch(x, w, gamma, mean, invstd, y, c, dy, slope, drop)
    assert not y[:, 3].any() and not y[0, 5].any() and y[1:, 5].any()
    assert float(dbeta[3]) == 0 and float(dgamma[3]) == 0 and not dw[3].any() and not dc[:, 3].any()
    assert dc[0, 5].any()                      # a dropped plane of a channel that lives in other frames
    M = N * H * W
    c64, dc64 = _np(c), _np(dc)
    xh = (c64 - _np(mean)[None, :, None, None]) * _np(invstd)[None, :, None, None]
    d = _np(dy) * mask.astype(np.float64)[:, :, None, None]
    g = np.where(_np(y) > 0, d, slope * d)
    sc = np.abs(_np(gamma) * _np(invstd))
    A = sc * (np.abs(g) + np.abs(_np(dbeta))[None, :, None, None] / M + np.abs(xh * _np(dgamma)[None, :, None, None]) / M).sum(axis=(0, 2, 3))
    tol = 64 * 2.0 ** -24 * A
    eps_term = _np(gamma) * _np(invstd) * _np(dgamma) * (1.0 - (xh * xh).sum(axis=(0, 2, 3)) / M)
    s0, s1 = np.abs(dc64.sum(axis=(0, 2, 3))), np.abs((dc64 * xh).sum(axis=(0, 2, 3)) - eps_term)
    live = A > 0
    print(f"{shape}: sum dc {np.max(s0[live] / tol[live]):.3f}, sum dc xhat {np.max(s1[live] / tol[live]):.3f} of 64 x 2^-24 x A; "
          f"|mean| invstd <= {np.abs(_np(mean) * _np(invstd)).max():.2f}")
    assert np.abs(_np(mean) * _np(invstd)).max() < 2
    assert (s0 <= tol).all() and (s1 <= tol).all()


# ---- 3. the draw -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,step", [(0, 1), (0xFEDCBA9876543210, 4000000000)])
def test_device_mask_equals_the_python_restatement(seed, step):
    from nano_vs_slam_amd import vpr_head_training as ht
    got = ht.dropout2d_scale(5, 48, 0.2, seed, step, 1, DEV)
    assert got.dtype == torch.float32 and got.shape == (5, 48)
    want = br.dropout_scale(5, 48, 0.2, seed, step, 1)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert torch.equal(got, ht.dropout2d_scale(5, 48, 0.2, seed, step, 1, DEV))
    assert not torch.equal(got, ht.dropout2d_scale(5, 48, 0.2, seed, step, 2, DEV))
    assert (ht.dropout2d_scale(5, 48, 0.0, seed, step, 1, DEV) == 1).all()


def test_dropped_share():
    from nano_vs_slam_amd import vpr_head_training as ht
    m = ht.dropout2d_scale(64, 128, 0.2, 11, 1, 1, DEV)
    share = float((m == 0).float().mean())
    sd = np.sqrt(0.2 * 0.8 / (64 * 128))
    print(f"dropped share {share:.4f}: {abs(share - 0.2) / sd:.2f} standard deviations from 0.2")
    assert abs(share - 0.2) <= 5 * sd
    assert ((m == 0) | (m == 1.25)).all()


# ---- 4. the trainer --------------------------------------------------------------------------------------------------------
def _model_with(inp):
    """A config-S model (64 -> 64, K = 64) whose vlad_head holds the case's parameters and statistics, in fp32 mode."""
    model, _ = product_model("S", False, 28, DEV)
    head = model.vlad_head
    with torch.no_grad():
        for i, layer in enumerate((head.convlad1, head.convlad2, head.convlad3)):
            layer.conv.weight.copy_(_dev(inp["params"][3 * i]))
            layer.bn.weight.copy_(_dev(inp["params"][3 * i + 1]))
            layer.bn.bias.copy_(_dev(inp["params"][3 * i + 2]))
            layer.bn.running_mean.copy_(_dev(inp["stats"][i][0]))
            layer.bn.running_var.copy_(_dev(inp["stats"][i][1]))
            assert layer.bn.eps == hr.BN_EPS and layer.bn.momentum == br.MOMENTUM
        head.netvlad.conv.weight.copy_(_dev(inp["params"][9]).view(inp["K"], inp["C"], 1, 1))
        head.netvlad.centroids.copy_(_dev(inp["params"][10]))
    return model.set_precision("fp32")


def test_trainer_follows_the_reference_trajectory(bounds):
    """bn="batch", dropout=0.2, each step under the mask the reference's Dropout2d drew at that step: the ten losses, and
    the parameters and running statistics after three steps (the sign-driven exemption of
    test_gpu_vpr_head_training.py's trajectory test, by the same rule)."""
    from nano_vs_slam_amd import vpr_head_training as ht
    name = br.TRAJECTORY
    inp = hr.make_inputs(br.FIXTURES[name][0])
    fx = br.load_fixture(name)
    model = _model_with(inp)
    trainer = ht.VPRHeadTrainer(model, lr=hr.LR, margin=hr.MARGIN, bn="batch", dropout=br.P_DROP)
    feat = _dev(inp["feat"])
    drops = fx["masks"]
    tracked0 = [int(l.bn.num_batches_tracked) for l in trainer.layers]
    losses, kept, kept_stats = [], None, None
    for t in range(hr.TRAJECTORY_STEPS):
        buffers = [b for l in trainer.layers for b in (l.bn.running_mean, l.bn.running_var, l.bn.num_batches_tracked)]
        versions = [p._version for p in trainer.parameters() + buffers]
        losses.append(trainer.step_features(feat, inp["B"], inp["counts"], drop=_dev(drops[t])))
        assert all(p._version > v for p, v in zip(trainer.parameters() + buffers, versions))
        if t + 1 == hr.PARAM_STEPS:
            kept = [p.detach().clone() for p in trainer.parameters()]
            kept_stats = [(l.bn.running_mean.clone(), l.bn.running_var.clone()) for l in trainer.layers]
    assert [int(l.bn.num_batches_tracked) for l in trainer.layers] == [n + hr.TRAJECTORY_STEPS for n in tracked0]
    losses = np.asarray([float(l) for l in losses])
    used = [abs(l - l64) / br.loss_bound(l64, bounds) for l, l64 in zip(losses, fx["losses"])]
    print("trainer losses", losses, "fractions of the loss bound", np.round(used, 3))
    assert max(used) <= 1.0
    _, want, want_stats, grads = br.trajectory(inp, drops[:hr.PARAM_STEPS])
    sb = max(8.0 * float(fx["err32_rstats_after"]), br.FLOOR)
    for i, ((m, v), (m64, v64)) in enumerate(zip(kept_stats, want_stats), 1):
        assert np.abs(hr.stored(m64) - fx[f"rmean{i}_after"]).max() <= 1e-10 and np.abs(hr.stored(v64) - fx[f"rvar{i}_after"]).max() <= 1e-10
        em, ev = hr.rel_err(_np(m), m64), hr.rel_err(_np(v), v64)
        print(f"running statistics of layer {i} after {hr.PARAM_STEPS} steps: mean {em / sb:.3f}, var {ev / sb:.3f} of {sb:.3e}")
        assert em <= sb and ev <= sb
    group_of = {i: g for g, members in hr.GROUPS.items() for i in members}
    tol = 1e-2 * hr.LR * hr.PARAM_STEPS
    for i, got in enumerate(kept):
        assert np.abs(hr.stored(want[i]) - fx[f"p{i}_after"]).max() <= 1e-10
        skip = np.zeros(want[i].shape, bool)
        for g in grads:
            skip |= np.abs(g[i]) < bounds[group_of[i]] * np.abs(g[i]).max()
        diff = np.abs(_np(got).reshape(want[i].shape) - want[i])
        print(f"{hr.PARAMS[i]} after {hr.PARAM_STEPS} steps: max|diff| {diff[~skip].max():.3e} = {diff[~skip].max() / tol:.3f} of {tol:.1e}; "
              f"sign-driven elements {int(skip.sum())} of {skip.size}")
        assert diff[~skip].max() <= tol, hr.PARAMS[i]
        assert diff.max() <= 2.5 * hr.LR * hr.PARAM_STEPS, hr.PARAMS[i]


def test_trainer_draws_its_own_mask_per_step():
    """Without an injected mask the step's mask is dropout2d_scale(N, C, p, seed, step, 1): the loss of step 1 equals a
    step under that mask bit for bit, and the steps are reproducible from the seed."""
    from nano_vs_slam_amd import vpr_head_training as ht
    inp = hr.make_inputs("C")
    feat = _dev(inp["feat"])
    out = []
    for injected in (False, True, False):
        trainer = ht.VPRHeadTrainer(_model_with(inp), lr=hr.LR, bn="batch", dropout=0.2, seed=9)
        drop = ht.dropout2d_scale(inp["N"], inp["C"], 0.2, 9, 1, 1, DEV) if injected else None
        first = trainer.step_features(feat, inp["B"], inp["counts"], drop=drop)
        out.append((first, trainer.step_features(feat, inp["B"], inp["counts"])))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][0], out[2][0]) and torch.equal(out[0][1], out[2][1])
    other = ht.VPRHeadTrainer(_model_with(inp), lr=hr.LR, bn="batch", dropout=0.2, seed=10).step_features(feat, inp["B"], inp["counts"])
    assert not torch.equal(other, out[0][0])
    # dropout on running statistics: the other half of the reference's mode alone
    t = ht.VPRHeadTrainer(_model_with(inp), lr=hr.LR, dropout=0.2, seed=9)
    stats0 = [(l.bn.running_mean.clone(), l.bn.running_var.clone()) for l in t.layers]
    plain = ht.VPRHeadTrainer(_model_with(inp), lr=hr.LR).step_features(feat, inp["B"], inp["counts"])
    assert not torch.equal(t.step_features(feat, inp["B"], inp["counts"]), plain)
    for l, (m0, v0) in zip(t.layers, stats0):
        assert torch.equal(l.bn.running_mean, m0) and torch.equal(l.bn.running_var, v0)


def test_engine_refolds_the_updated_running_statistics():
    """After a batch-mode step over frames the engine's only_encoder in fp32 mode equals the training forward run on the NEW
    running statistics: the engine re-packed from the updated buffers.  num_batches_tracked rose by one."""
    from nano_vs_slam_amd import vpr_head_training as ht
    from oracle.weights import synthetic_frames
    model, _ = product_model("S", False, 28, DEV)
    model.set_precision("fp32")
    H, W = 64, 96
    f = _dev(synthetic_frames(3, H, W, seed=31))
    query, positives = f[0:1], f[1:2]
    negatives = torch.stack([0.9 * f[0] + 0.1 * f[2], f[2]])
    x = torch.cat([query, positives, negatives])
    trainer = ht.VPRHeadTrainer(model, lr=1e-3, margin=hr.MARGIN, bn="batch", dropout=0.2, seed=3)
    frozen = ht.VPRHeadTrainer(model)

    def both():
        with torch.no_grad():
            own = model.only_encoder(x).clone()
            y3 = frozen.forward_features(model.backbone_features(x))[-1][1]
            return own, torch.nn.functional.normalize(y3, p=2.0, dim=1)

    own0, mine0 = both()
    stats0 = [(l.bn.running_mean.clone(), l.bn.running_var.clone(), int(l.bn.num_batches_tracked)) for l in trainer.layers]
    loss = trainer.step(query, positives, negatives, torch.tensor([2]))
    assert float(loss) > 0 and trainer.steps == 1
    for l, (m0, v0, n0) in zip(trainer.layers, stats0):
        assert not torch.equal(l.bn.running_mean, m0) and not torch.equal(l.bn.running_var, v0)
        assert int(l.bn.num_batches_tracked) == n0 + 1
    # the same step with the parameters alone moved: what the engine would show had it kept the old statistics
    own1, mine1 = both()
    err0, err1 = float((own0 - mine0).abs().max()), float((own1 - mine1).abs().max())
    with torch.no_grad():
        saved = [(l.bn.running_mean.clone(), l.bn.running_var.clone()) for l in trainer.layers]
        for l, (m0, v0, _) in zip(trainer.layers, stats0):
            l.bn.running_mean.copy_(m0)
            l.bn.running_var.copy_(v0)
        stale = frozen.forward_features(model.backbone_features(x))[-1][1]
        stale = torch.nn.functional.normalize(stale, p=2.0, dim=1)
        for l, (m, v) in zip(trainer.layers, saved):
            l.bn.running_mean.copy_(m)
            l.bn.running_var.copy_(v)
    moved = float((own1 - stale).abs().max())
    print(f"training forward on running statistics vs only_encoder: before {err0:.3e} = {err0 / TAP_TOL:.3f}, after {err1:.3e} = "
          f"{err1 / TAP_TOL:.3f} of {TAP_TOL}; the statistics alone moved the map by {moved:.3e}")
    assert err0 <= TAP_TOL and err1 <= TAP_TOL
    assert moved > TAP_TOL


def test_default_trainer_is_the_chain_of_the_running_statistics_calls():
    """VPRHeadTrainer(model) with its defaults: the same bits as cbr_forward / cbr_backward chained by hand with Adam."""
    from nano_vs_slam_amd import vlad_training as vt, vpr_head_training as ht
    inp = hr.make_inputs("C")
    feat = _dev(inp["feat"])
    model = _model_with(inp)
    trainer = ht.VPRHeadTrainer(model, lr=hr.LR, margin=hr.MARGIN)
    assert trainer.bn == "running" and trainer.dropout == 0.0
    stats0 = [(l.bn.running_mean.clone(), l.bn.running_var.clone(), int(l.bn.num_batches_tracked)) for l in trainer.layers]
    # by hand, on copies
    params = [p.detach().clone() for p in trainer.parameters()]
    acts, x = [], feat
    for i, layer in enumerate(trainer.layers):
        vec = ht.bn_vectors(layer.bn)
        y, c = ht.cbr_forward(x, params[3 * i], vec[0], vec[1], trainer.slope)
        acts.append((x, y, c, vec))
        x = y
    W, cent = params[9], params[10]
    vlad, saved = vt.netvlad_forward(x, W, cent)
    loss, dvlad, n_active = vt.triplet_margin_loss(vlad, inp["B"], inp["counts"], hr.MARGIN)
    grads = [None] * 9 + list(vt.netvlad_backward(x, W, cent, saved, dvlad))
    dy = ht.netvlad_backward_input(x, W, cent, saved, dvlad)
    for i in (2, 1, 0):
        lx, ly, lc, (scale, _, mean, invstd) = acts[i]
        dw, dgamma, dbeta, dy = ht.cbr_backward(lx, params[3 * i], scale, mean, invstd, ly, lc, dy, trainer.slope, need_dx=i > 0)
        grads[3 * i:3 * i + 3] = [dw, dgamma, dbeta]
    for p, g in zip(params, grads):
        vt.adam_step(p, g.view(p.shape), torch.zeros_like(p), torch.zeros_like(p), 1, hr.LR)
    got = trainer.step_features(feat, inp["B"], inp["counts"])
    assert torch.equal(got, loss) and torch.equal(trainer.n_active, n_active)
    for name, p, q in zip(hr.PARAMS, trainer.parameters(), params):
        assert torch.equal(p.detach(), q), name
    for l, (m0, v0, n0) in zip(trainer.layers, stats0):
        assert torch.equal(l.bn.running_mean, m0) and torch.equal(l.bn.running_var, v0) and int(l.bn.num_batches_tracked) == n0


# ---- 5. the C ABI refuses before launching -----------------------------------------------------------------------------------
def test_c_abi_refuses_before_launching():
    from nano_vs_slam_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    p, null = C.c_void_p(buf.data_ptr()), None
    odd = C.c_void_p(buf.data_ptr() + 2)
    big = 1 << 18
    fwd, bwd, mask = lib.kp2d_cbr_forward_batchnorm, lib.kp2d_cbr_backward_batchnorm, lib.kp2d_dropout2d_mask

    def f(N=2, H=5, W=7, ci=16, co=16, x=p, drop=null, rm=null, rv=null, mean=p, eps=1e-5, slope=0.01, mom=0.1, nbytes=big):
        return fwd(x, p, p, p, eps, slope, drop, mom, rm, rv, N, H, W, ci, co, p, p, mean, p, p, nbytes, null)

    def b(N=2, H=5, W=7, ci=16, co=16, dy=p, drop=null, dx=null, slope=0.01, nbytes=big):
        return bwd(p, p, p, p, p, slope, drop, p, p, dy, N, H, W, ci, co, p, p, p, dx, p, nbytes, null)

    assert f(N=1, H=1, W=1) == -1 and b"N * H * W >= 2" in lib.kp2d_last_error()       # M < 2: KP2D_ERR_ARG
    assert b(N=1, H=1, W=1) == -1 and b"N * H * W >= 2" in lib.kp2d_last_error()
    assert f(N=0) == -1 and b(N=0) == -1 and f(H=0) == -1 and b(W=0) == -1
    assert f(ci=24) == -2 and f(co=8) == -2 and f(co=144) == -2 and b(ci=24) == -2 and b(co=160) == -2      # KP2D_ERR_UNSUPPORTED
    assert f(x=null) == -1 and b"null" in lib.kp2d_last_error()
    assert f(mean=null) == -1 and b"null" in lib.kp2d_last_error()
    assert b(dy=null) == -1 and b"null" in lib.kp2d_last_error()
    assert f(nbytes=16) == -1 and b"scratch" in lib.kp2d_last_error()
    assert b(nbytes=16) == -1 and b"scratch" in lib.kp2d_last_error()
    assert f(slope=1.5) == -1 and b(slope=-0.1) == -1 and f(eps=-1.0) == -1 and f(eps=float("nan")) == -1
    assert f(mom=1.5) == -1 and f(mom=-0.5) == -1
    assert f(drop=odd) == -1 and f(rm=odd) == -1 and f(rv=odd) == -1 and b(drop=odd) == -1 and b(dx=odd) == -1
    assert mask(p, 4, 16, 1.0, 0, 1, 1, null) == -1 and b"outside [0, 1)" in lib.kp2d_last_error()          # p >= 1
    assert mask(p, 4, 16, -0.1, 0, 1, 1, null) == -1 and mask(p, 4, 16, float("nan"), 0, 1, 1, null) == -1
    assert mask(null, 4, 16, 0.2, 0, 1, 1, null) == -1 and b"null" in lib.kp2d_last_error()
    assert mask(p, 0, 16, 0.2, 0, 1, 1, null) == -1 and mask(p, 4, 0, 0.2, 0, 1, 1, null) == -1 and mask(p, 65536, 65536, 0.2, 0, 1, 1, null) == -1
    assert mask(p, 4, 16, 0.2, 0, -1, 1, null) == -1 and mask(p, 4, 16, 0.2, 0, 1 << 32, 1, null) == -1 and mask(p, 4, 16, 0.2, 0, 1, -1, null) == -1
    torch.cuda.synchronize()
    assert not buf.any()
