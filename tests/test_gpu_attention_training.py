"""The attention head's training step on the device (nano_vs_slam_amd.attention_training, train_ops' stage calls,
csrc/attention_train.hip) against the float64 outputs of the reference's SegFormerAttentionModule and SegmentationHeadATT in
.eval() under torch autograd (tests/golden/attention_training/, written by tools/make_attention_training_golden.py; inputs
regenerated from seeds by attention_training_ref).  The fixtures keep a stated stride of every larger array, so the numpy
float64 oracle, held to the stored entries to 1e-10, stands in for the whole arrays.

Error measure: for an array G, E(G) = max|G - G64| / max|G64|; for the loss |loss - loss64| / |loss64|.
Bound per quantity and case: max(8 x the reference modules' own float32 error of that quantity (the same modules run in float32
on the CPU against their float64 run), 16 x 2^-24), read from the case's fixture.  The unpinned cases (a LayerNorm pixel with
constant channels, logits beyond +-60) are held to the float64 oracle alone, on the same float32 inputs, with 16 x 2^-24.
Every test prints each figure before it asserts and the largest share of a bound it used; profiles/attention_training_fp64.txt
holds the lines of one run on an MI355X, and the README section repeats the shares.
"""
import types

import numpy as np
import pytest
import torch

import attention_training_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4        # the project's inference contract in fp32 mode (test_gpu_parity.py)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _f32(a):
    return _dev(np.asarray(a, np.float32))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


class Check:
    """E(G) against its bound: prints every figure, keeps the largest share, and ``done`` asserts that none was over."""

    def __init__(self, what):
        self.what, self.worst, self.over = what, (0.0, ""), []

    def __call__(self, key, got, ref, bound, mask=None):
        ref = np.asarray(ref, np.float64)
        got = np.asarray(got, np.float64).reshape(ref.shape)
        e = ar.rel_err(got, ref) if mask is None else float(np.abs(got - ref)[mask].max(initial=0.0) / np.abs(ref).max())
        print(f"{self.what}: E({key}) {e:.3e} of {bound:.3e}")
        if e / bound >= self.worst[0]:
            self.worst = (e / bound, key)
        if not e <= bound:
            self.over.append((key, e, bound))

    def done(self):
        print(f"{self.what}: largest share of a bound {self.worst[0]:.3f} ({self.worst[1]})")
        assert not self.over, (self.what, self.over)


def _lse_pair(lse64):
    """The float64 log-sum-exp as the device keeps it: its float32 rounding and what that dropped."""
    hi = np.asarray(lse64, np.float32)
    return _dev(np.stack([hi, (np.asarray(lse64, np.float64) - hi).astype(np.float32)]))


def _ops():
    from nano_vs_slam_amd import train_ops
    return train_ops


def _module(params, C):
    """The project's holder of a SegFormerAttentionModule(C) with the case's parameters."""
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import _AttentionModule
    m = _AttentionModule(C).to(DEV)
    with torch.no_grad():
        for t, a in zip(_ops().attention_module_parameters(m), params):
            t.copy_(_dev(a))
    return m


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in ar.MODULE_CASES:
        inp, fx = ar.make_module_inputs(name), ar.load_fixture(name)
        ref = ar.module_step(inp)
        for k in ar.MODULE_MAPS + ar.MODULE_DMAPS:      # the oracle stands in for the whole arrays: held to the fixture here
            assert np.abs(ar.stored(ref[k]) - fx[k]).max() <= 1e-10, k
        for i, g in enumerate(ref["grads"]):
            assert np.abs(ar.stored(g) - fx[f"g{i}"]).max() <= 1e-10, i
        out[name] = (inp, ref, fx)
    return out


# ---- 1. every stage alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ar.MODULE_CASES))
def test_stages_alone(cases, name):
    """Each stage call on the float32 rounding of the oracle's own input of that stage."""
    ops = _ops()
    inp, ref, fx = cases[name]
    p = [_dev(a) for a in inp["params"]]
    r = {k: _f32(v) for k, v in ref.items() if isinstance(v, np.ndarray)}
    chk = Check(f"case {name} stages")
    b = lambda k: ar.bound(fx, k)
    n1, mean1, rinv1 = ops.layernorm_forward(r["x"], p[3], p[4])
    chk("n1", _np(n1), ref["n1"], b("n1"))
    chk("mean1", _np(mean1), ref["mean1"], ar.FLOOR)
    chk("rinv1", _np(rinv1), ref["rinv1"], ar.FLOOR)
    chk("q", _np(ops.pointwise_forward(r["n1"], p[0])[0]), ref["q"], b("q"))
    chk("kv", _np(ops.patch2_forward(r["n1"], p[1])), ref["kv"], b("kv"))
    o, lse = ops.attention_forward(r["q"], r["kv"])
    chk("o", _np(o), ref["o"], b("o"))
    chk("lse", _np(lse[0]), ref["lse"], b("lse"))
    chk("a", _np(ops.pointwise_forward(r["o"], p[2])[0]), ref["a"], b("a"))
    n2, mean2, rinv2 = ops.layernorm_forward(r["a"], p[13], p[14])
    chk("n2", _np(n2), ref["n2"], b("n2"))
    chk("h0", _np(ops.pointwise_forward(r["n2"], p[5], p[6])[0]), ref["h0"], b("h0"))
    chk("h1", _np(ops.dwconv3_forward(r["h0"], p[7], p[8])), ref["h1"], b("h1"))
    h2, pre = ops.pointwise_forward(r["h1"], p[9], p[10], gelu=True)
    chk("pre", _np(pre), ref["pre"], b("pre"))
    chk("h2", _np(h2), ref["h2"], b("h2"))
    chk("y", _np(ops.pointwise_forward(r["h2"], p[11], p[12])[0]), ref["y"], b("y"))

    g = ref["grads"]
    d, dw, db = ops.pointwise_backward(r["h2"], p[11], _dev(inp["dy"]))
    chk("d_h2", _np(d), ref["d_h2"], b("d_h2")); chk("g11", _np(dw), g[11], b("g11")); chk("g12", _np(db), g[12], b("g12"))
    d, dw, db = ops.pointwise_backward(r["h1"], p[9], r["d_h2"], pre=r["pre"])
    chk("d_h1", _np(d), ref["d_h1"], b("d_h1")); chk("g9", _np(dw), g[9], b("g9")); chk("g10", _np(db), g[10], b("g10"))
    d, dw, db = ops.dwconv3_backward(r["h0"], p[7], r["d_h1"])
    chk("d_h0", _np(d), ref["d_h0"], b("d_h0")); chk("g7", _np(dw), g[7], b("g7")); chk("g8", _np(db), g[8], b("g8"))
    d, dw, db = ops.pointwise_backward(r["n2"], p[5], r["d_h0"])
    chk("d_n2", _np(d), ref["d_n2"], b("d_n2")); chk("g5", _np(dw), g[5], b("g5")); chk("g6", _np(db), g[6], b("g6"))
    d, dg, db = ops.layernorm_backward(r["a"], p[13], r["mean2"], r["rinv2"], r["d_n2"])
    chk("d_a", _np(d), ref["d_a"], b("d_a")); chk("g13", _np(dg), g[13], b("g13")); chk("g14", _np(db), g[14], b("g14"))
    d, dw, none = ops.pointwise_backward(r["o"], p[2], r["d_a"], need_dbias=False)
    assert none is None
    chk("d_o", _np(d), ref["d_o"], b("d_o")); chk("g2", _np(dw), g[2], b("g2"))
    dq, dkv = ops.attention_backward(r["q"], r["kv"], r["o"], _lse_pair(ref["lse"]), r["d_o"])
    chk("d_q", _np(dq), ref["d_q"], b("d_q")); chk("d_kv", _np(dkv), ref["d_kv"], b("d_kv"))
    dn_q, dw, _ = ops.pointwise_backward(r["n1"], p[0], r["d_q"], need_dbias=False)
    chk("g0", _np(dw), g[0], b("g0"))
    dn_kv, dw = ops.patch2_backward(r["n1"], p[1], r["d_kv"])
    chk("g1", _np(dw), g[1], b("g1"))
    chk("d_n1", _np(dn_q + dn_kv), ref["d_n1"], b("d_n1"))
    d, dg, db = ops.layernorm_backward(r["x"], p[3], r["mean1"], r["rinv1"], r["d_n1"])
    chk("dx", _np(d), ref["dx"], b("dx")); chk("g3", _np(dg), g[3], b("g3")); chk("g4", _np(db), g[4], b("g4"))
    assert ops.pointwise_backward(r["n1"], p[0], r["d_q"], need_dx=False)[0] is None
    chk.done()


# ---- 2. the whole module, twice ----------------------------------------------------------------------------------------------
def _run_module(inp, frames=slice(None)):
    ops = _ops()
    m = _module(inp["params"], inp["C"])
    y, saved = ops.attention_module_forward(m, _dev(inp["x"][frames]))
    grads, dx = ops.attention_module_backward(m, saved, _dev(inp["dy"][frames]))
    return y, saved, grads, dx


@pytest.mark.parametrize("name", list(ar.MODULE_CASES))
def test_whole_module(cases, name):
    inp, ref, fx = cases[name]
    y, saved, grads, dx = _run_module(inp)
    chk = Check(f"case {name} module")
    for k in ("n1", "q", "kv", "o", "lse", "a", "n2", "h0", "h1", "pre", "h2"):
        chk(k, _np(saved[k][0] if k == "lse" else saved[k]), ref[k], ar.bound(fx, k))
    chk("y", _np(y), ref["y"], ar.bound(fx, "y"))
    chk("dx", _np(dx), ref["dx"], ar.bound(fx, "dx"))
    for i, g in enumerate(grads):
        assert g.shape == tuple(inp["params"][i].shape)
        chk(f"g{i}", _np(g), ref["grads"][i], ar.bound(fx, f"g{i}"))
    chk.done()
    y2, saved2, grads2, dx2 = _run_module(inp)          # two runs agree bit for bit
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert all(torch.equal(saved[k], saved2[k]) for k in saved)
    m = _module(inp["params"], inp["C"])
    assert _ops().attention_module_backward(m, saved, _dev(inp["dy"]), need_dx=False)[1] is None


# ---- 3. the exact statements ----------------------------------------------------------------------------------------------------
def test_a_frame_alone_is_the_frame_in_the_batch(cases):
    """Case B: attention couples nothing across frames, and no per-frame result depends on the batch."""
    inp = cases["B"][0]
    y, saved, _, dx = _run_module(inp)
    for n in range(inp["N"]):
        y1, saved1, _, dx1 = _run_module(inp, slice(n, n + 1))
        assert torch.equal(y[n:n + 1], y1) and torch.equal(dx[n:n + 1], dx1)
        for k in ("n1", "q", "kv", "o", "a", "n2", "h0", "h1", "pre", "h2"):
            assert torch.equal(saved[k][n:n + 1], saved1[k]), k
        assert torch.equal(saved["lse"][:, n:n + 1], saved1["lse"])
    ops, ref = _ops(), cases["B"][1]
    t = {k: _f32(ref[k]) for k in ("q", "kv", "o", "d_o")}
    lse = _lse_pair(ref["lse"])
    dq, dkv = ops.attention_backward(t["q"], t["kv"], t["o"], lse, t["d_o"])
    dq1, dkv1 = ops.attention_backward(t["q"][1:2].contiguous(), t["kv"][1:2].contiguous(), t["o"][1:2].contiguous(), lse[:, 1:2].contiguous(),
                                       t["d_o"][1:2].contiguous())
    assert torch.equal(dq[1:2], dq1) and torch.equal(dkv[1:2], dkv1)


def test_the_dropped_line_gets_exact_zeros(cases):
    """Case B, 15 x 20: the last row is in no 2 x 2 patch; its dx from the key/value branch is written as zeros."""
    inp, ref, _ = cases["B"]
    ops = _ops()
    from nano_vs_slam_amd import _dev as dev, _lib
    n1, dkv, w = _f32(ref["n1"]), _f32(ref["d_kv"]), _dev(inp["params"][1])
    N, C, H, W = n1.shape
    lib = _lib.load()
    scratch = dev.scratch(int(lib.kp2d_att_train_scratch_bytes(N, H, W, C, 2 * C)), n1.device)
    dx, dw = torch.full_like(n1, float("nan")), torch.empty_like(w)      # a poisoned buffer: the zeros must be written
    _lib.check(lib.kp2d_patch2_backward(n1.data_ptr(), w.data_ptr(), dkv.data_ptr(), N, C, H, W, dx.data_ptr(), dw.data_ptr(),
                                        scratch.data_ptr(), scratch.numel(), dev.stream(n1.device)))
    assert torch.isfinite(dx).all()
    assert int(torch.count_nonzero(dx[:, :, -1])) == 0 and int(torch.count_nonzero(dx[:, :, :-1])) > 0
    out, dw2 = ops.patch2_backward(n1, w, dkv)
    assert torch.equal(out, dx) and torch.equal(dw, dw2)


def test_one_key(cases):
    """Case D, 2 x 2: one key, so the softmax is 1: dQ = dK = 0 exactly, dV = the sum of dO."""
    inp, ref, fx = cases["D"]
    ops = _ops()
    t = {k: _f32(ref[k]) for k in ("q", "kv", "d_o")}
    o, lse = ops.attention_forward(t["q"], t["kv"])
    C = inp["C"]
    assert torch.equal(o, t["kv"][:, C:].expand(-1, -1, 2, 2))          # O is V, bit for bit
    dq, dkv = ops.attention_backward(t["q"], t["kv"], o, lse, t["d_o"])
    assert int(torch.count_nonzero(dq)) == 0 and int(torch.count_nonzero(dkv[:, :C])) == 0
    chk = Check("case D one key")
    chk("dV", _np(dkv[:, C:, 0, 0]), np.asarray(ref["d_o"], np.float32).astype(np.float64).sum(axis=(2, 3)), ar.bound(fx, "d_kv"))
    chk.done()
    y, saved, grads, dx = _run_module(inp)
    assert int(torch.count_nonzero(grads[0])) == 0                      # to_q moves nothing with one key


# ---- 4. unpinned: against the float64 oracle alone ---------------------------------------------------------------------------
def test_saturated_logits(cases):
    """Case F: case B's q and k scaled until the logits reach about +-60 (measured span -55.65 ... 60.00); the oracle runs on
    the same float32 inputs; bound 16 x 2^-24 = 9.537e-07 on every tensor.

    Measured on an MI355X: E(o) 3.04e-07, E(lse) 3.24e-08, E(dq) 4.96e-07, E(dkv) 8.54e-07 (0.90 of the bound).  With float32
    logits this case missed the bound on dq (1.06 x) and dkv (1.30 x; 1.52 x before the log-sum-exp kept its rounding
    residual): near 60 an ulp of a float32 logit is 3.8e-6 and the backward forms every probability again from it, which is
    why the kernels form the logits, the running maximum and the log-sum-exp in float64 (csrc/attention_train.hip,
    logit_tile)."""
    inp, ref, _ = cases["B"]
    ops = _ops()
    C = inp["C"]
    rng = np.random.default_rng(77)
    q, kv = ref["q"].copy(), ref["kv"].copy()
    sim_max = max(np.abs(np.einsum("nhic,nhjc->nhij", ar._heads(q), ar._heads(kv[:, :C]))).max() * (C // ar.HEADS) ** -0.5, 1e-9)
    f = np.sqrt(60.0 / sim_max)
    q, kv[:, :C] = q * f, kv[:, :C] * f
    q, kv = q.astype(np.float32), kv.astype(np.float32)
    do = rng.standard_normal(q.shape).astype(np.float32)
    sim = np.einsum("nhic,nhjc->nhij", ar._heads(q.astype(np.float64)), ar._heads(kv[:, :C].astype(np.float64))) * (C // ar.HEADS) ** -0.5
    print(f"case F: logits in [{sim.min():.2f}, {sim.max():.2f}]")
    assert np.abs(sim).max() > 59 and sim.max() > 40 and sim.min() < -40
    o64, lse64 = ar.attention(q, kv)
    o, lse = ops.attention_forward(_dev(q), _dev(kv))
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    dq64, dkv64 = ar.attention_backward(q, kv, do)
    dq, dkv = ops.attention_backward(_dev(q), _dev(kv), o, lse, _dev(do))
    assert torch.isfinite(dq).all() and torch.isfinite(dkv).all()
    chk = Check("case F saturated")
    chk("o", _np(o), o64, ar.FLOOR); chk("lse", _np(lse[0]), lse64, ar.FLOOR)
    chk("dq", _np(dq), dq64, ar.FLOOR); chk("dkv", _np(dkv), dkv64, ar.FLOOR)
    chk.done()


def test_layernorm_pixel_with_constant_channels():
    """sqrt(var) = 0 at one pixel: the term through the deviation is taken as 0 (torch: NaN); the oracle states the same rule."""
    ops = _ops()
    rng = np.random.default_rng(78)
    x = rng.standard_normal((2, 64, 3, 5)).astype(np.float32)
    x[1, :, 2, 3] = 0.75
    g, b = rng.uniform(0.5, 1.5, (1, 64, 1, 1)).astype(np.float32), rng.standard_normal((1, 64, 1, 1)).astype(np.float32)
    dy = rng.standard_normal(x.shape).astype(np.float32)
    y, mean, rinv = ops.layernorm_forward(_dev(x), _dev(g), _dev(b))
    dx, dg, db = ops.layernorm_backward(_dev(x), _dev(g), mean, rinv, _dev(dy))
    assert all(torch.isfinite(t).all() for t in (y, mean, rinv, dx, dg, db))
    y64 = ar.layernorm(x, g, b)[0]
    dx64, dg64, db64 = ar.layernorm_backward(x, g, dy)
    assert torch.equal(y[1, :, 2, 3], _dev(b).flatten())               # (x - mean) = 0 exactly: y = b there
    chk = Check("layernorm s = 0")
    chk("y", _np(y), y64, ar.FLOOR); chk("dx", _np(dx), dx64, ar.FLOOR); chk("dg", _np(dg), dg64, ar.FLOOR); chk("db", _np(db), db64, ar.FLOOR)
    chk.done()


# ---- 5. the head --------------------------------------------------------------------------------------------------------------------
def _stand_in(inp):
    """A model-shaped holder of a V2 attention head with the case's channel counts, parameters and statistics."""
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import _SegHead
    head = _SegHead(inp["c_in"], inp["c_hidden"], inp["d1"] // 4 + inp["c_skip"], inp["classes"], inp["d1"], 0.1, True).to(DEV)
    named = dict(head.named_parameters())
    assert list(named) == list(ar.HEAD_PARAMS)
    with torch.no_grad():
        for n, a in zip(ar.HEAD_PARAMS, inp["params"]):
            named[n].copy_(_dev(a))
        for i, (mean, var) in inp["stats"].items():
            head.convs[i].bn.running_mean.copy_(_dev(mean))
            head.convs[i].bn.running_var.copy_(_dev(var))
            assert head.convs[i].bn.eps == ar.sr.BN_EPS
    attr = "depth_head" if inp["loss"] == "depth" else "seg_head"
    return types.SimpleNamespace(**{attr: head}, _version_id=2, upscale_method="pixelshuffle", use_attention=True, leaky_relu=True)


def _trainer(inp, **kw):
    from nano_vs_slam_amd import attention_training as at
    cls = at.AttentionDepthHeadTrainer if inp["loss"] == "depth" else at.AttentionSegHeadTrainer
    return cls(_stand_in(inp), lr=ar.LR, **kw)


@pytest.mark.parametrize("name", list(ar.HEAD_CASES))
def test_head_gradients(name):
    inp, fx = ar.make_head_inputs(name), ar.load_fixture(name)
    ref = ar.head_step(inp)
    for k in ar.HEAD_MAPS + ("dlogits",):
        assert np.abs(ar.stored(ref[k]) - fx[k]).max() <= 1e-10, k
    trainer = _trainer(inp)
    x, skip, target = _dev(inp["x"]), _dev(inp["skip"]), _dev(inp["target"])
    loss, logits, grads = trainer.gradients(x, skip, target)
    assert len(grads) == 47 == len(trainer.parameters())
    chk = Check(f"head {name}")
    chk("loss", float(loss), ref["loss"], ar.bound(fx, "loss"))
    chk("logits", _np(logits), ref["logits"], ar.bound(fx, "logits"))
    chk("logits (forward_features)", _np(trainer.forward_features(x, skip)), ref["logits"], ar.bound(fx, "logits"))
    for i, (g, p) in enumerate(zip(grads, trainer.parameters())):
        assert g.numel() == p.numel()
        chk(f"g{i} {ar.HEAD_PARAMS[i]}", _np(g), ref["grads"][i], ar.bound(fx, f"g{i}"))
    chk.done()
    loss2, logits2, grads2 = trainer.gradients(x, skip, target)        # two runs agree bit for bit
    assert torch.equal(loss, loss2) and torch.equal(logits, logits2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert int(trainer.stray) == 0 and int(trainer.valid) > 0


def _follow(name, inp, fx, case_fx, steps, step, step_fn=None):
    """``steps`` Adam steps: the loss of and all 47 parameters after every step against the oracle's trajectory, which is held
    to the fixture here.  A parameter's elements whose oracle gradient at a step so far lies below that gradient's own bound
    are sign-driven (attention_training_ref.sign_driven): Adam moves them by lr g / (|g| + eps), so a gradient within its
    bound moves them elsewhere; they are counted, held to 4 lr per step (what Adam can move an element), and must be few."""
    losses64, after64, grads64 = ar.trajectory(inp, steps, step_fn=step_fn, keep_grads=True)
    assert np.abs(losses64 - fx["losses"]).max() <= 1e-10
    trainer = _trainer(inp)
    versions = [p._version for p in trainer.parameters()]
    chk = Check(f"trajectory {name}")
    driven = total = 0
    for t in range(steps):
        loss = step(trainer)
        chk(f"loss step {t}", float(loss), losses64[t], ar.bound(fx, "loss"))
        for i, p in enumerate(trainer.parameters()):
            assert np.abs(ar.stored(after64[t][i], ar.TRAJ_STORED) - fx[f"p{i}"][t]).max() <= 1e-10
            mask = ar.sign_driven(grads64[:t + 1], i, ar.bound(case_fx, f"g{i}"))
            chk(f"p{i} step {t}", _np(p), after64[t][i], ar.bound(fx, f"p{i}"), mask=~mask)
            assert np.abs(_np(p) - after64[t][i])[mask].max(initial=0.0) <= 4.0 * ar.LR * (t + 1)
            if t == steps - 1:
                driven, total = driven + int(mask.sum()), total + mask.size
    print(f"trajectory {name}: {driven} of {total} elements are sign-driven")
    assert driven <= 0.01 * total
    chk.done()
    assert trainer.steps == steps and all(p._version > v for p, v in zip(trainer.parameters(), versions))
    return trainer


@pytest.mark.parametrize("name", ["seg", "depth"])
def test_trajectories(name):
    """Five Adam steps of train="head"."""
    inp = ar.make_head_inputs(name)
    x, skip, target = _dev(inp["x"]), _dev(inp["skip"]), _dev(inp["target"])
    _follow(name, inp, ar.load_trajectory(name), ar.load_fixture(name), ar.TRAJECTORY_STEPS, lambda tr: tr.step_features(x, skip, target))


def test_pair_trajectory():
    """Three steps of the depth trainer's ``step_pair_features`` on a view pair: the inherited cross-view step.  The gradient
    bounds are the depth case's (the same head and shapes)."""
    inp = ar.make_pair_inputs()
    t = {k: _dev(inp[k]) for k in ("x", "skip", "x_aug", "skip_aug", "gt", "gt_aug", "homography")}
    step = lambda tr: tr.step_pair_features((t["x"], t["skip"]), (t["x_aug"], t["skip_aug"]), t["gt"], t["gt_aug"], t["homography"],
                                            cross_weight=ar.CROSS_WEIGHT)
    trainer = _follow("pair", inp, ar.load_trajectory("pair"), ar.load_fixture("depth"), ar.PAIR_STEPS, step, step_fn=ar.pair_step)
    assert trainer.pair_parts.shape == (5,) and int(trainer.inside) > 0


# ---- 6. wiring ----------------------------------------------------------------------------------------------------------------------
def test_engine_follows_three_steps():
    """A config-S_A model at 64 x 96: after three steps the engine's own forward, which re-packs the updated weights, agrees
    with the training forward within the inference contract; the loss has fallen."""
    from conftest import product_model
    from nano_vs_slam_amd import attention_training as at
    from oracle.weights import synthetic_frames
    model, _ = product_model("S_A", False, 28, DEV)
    model.set_precision("fp32")
    frames = _dev(synthetic_frames(2, 64, 96, seed=41))
    rng = np.random.default_rng(41)
    labels = rng.integers(0, 28, (2, 32, 48)).astype(np.uint8)
    labels[rng.random(labels.shape) < 0.1] = 255
    labels = _dev(labels)
    with torch.no_grad():
        x, skip = model.backbone_maps(frames)
        trainer = at.AttentionSegHeadTrainer(model, lr=1e-3)
        assert len(trainer.parameters()) == 47
        seg0 = model(frames)["seg"].clone()
        err0 = float((seg0 - trainer.forward_features(x, skip)).abs().max())
        losses = [float(trainer.step(frames, labels)) for _ in range(3)]
        seg1 = model(frames)["seg"]
        err1 = float((seg1 - trainer.forward_features(x, skip)).abs().max())
    moved = float((seg1 - seg0).abs().max())
    print(f"training forward vs the engine: before {err0:.3e}, after {err1:.3e} of {TOL}; moved {moved:.3e}; losses {losses}")
    assert err0 <= TOL and err1 <= TOL and moved > TOL
    assert losses[2] < losses[0]
    last = at.AttentionSegHeadTrainer(model, lr=1e-3, train="last")
    l0, l1 = float(last.step(frames, labels)), float(last.step(frames, labels))
    assert l1 < l0


def test_c_abi_refuses_before_launching():
    """Bad shapes, null pointers and short scratch return an error code without touching the device."""
    import ctypes as C
    from nano_vs_slam_amd import _lib
    lib = _lib.load()
    x = torch.zeros(1, 64, 4, 6, device=DEV)
    p = x.data_ptr()
    assert lib.kp2d_att_train_scratch_bytes(1, 4, 6, 40, 64) == 0 and lib.kp2d_att_train_scratch_bytes(0, 4, 6, 64, 64) == 0
    assert lib.kp2d_att_train_scratch_bytes(1, 4, 6, 64, 64) > 0
    assert lib.kp2d_attention_forward_train(p, p, 1, 128, 4, 6, p, p, None) == -2          # head dimension 32: unsupported (nothing is written)
    assert lib.kp2d_attention_forward_train(p, p, 1, 64, 1, 6, p, p, None) == -1           # no 2 x 2 key patch
    assert lib.kp2d_attention_forward_train(p, None, 1, 64, 4, 6, p, p, None) == -1
    assert lib.kp2d_layernorm_forward_train(p, p, p, 1, 40, 4, 6, 1e-5, p, p, p, None) == -2
    assert lib.kp2d_pointwise_backward(p, p, p, 1, 4, 6, 64, 64, p, p, p, p, 16, None) == -1    # scratch too short
    assert lib.kp2d_patch2_forward_train(p, p, 1, 96, 4, 6, p, None) == -2
    assert lib.kp2d_dwconv3_backward(p, p, p, 1, 64, 4, 6, p, p, p, None, 0, None) == -1
    assert b"scratch" in lib.kp2d_last_error()
    torch.cuda.synchronize()
