"""The training layer ops on the device (nano_vs_slam_amd.train_ops; csrc/train_conv.h, csrc/vpr_head_train.hip,
csrc/seg_train.hip) at the shapes of train_ops_shapes_ref: more than one tile per weight-gradient slab with slabs that
straddle two frames and a short last slab (G1: 2 tiles per slab, G2: 3), more than one pass of every plane loop (G1: 703
pixels, G2: 3200), and on G3 every channel width NT = 1..8 as the output width of the forward, the weight gradient and the
data gradient, in the plain and in the padded (conv_bias) form, up to the largest LDS images.

1. Exact: on the dyadic inputs every product and partial sum is a float32 number (train_ops_shapes_ref.check_exact asserts
   the condition again here, before the comparison), so the device result equals the float64 result bit for bit: no tolerance,
   one dropped, doubled or misplaced term fails.
2. Float-valued, for batch-statistic BatchNorm with Dropout2d factors and the LeakyReLU epilogue: E(G) = max|G - G64| / max|G64|
   against torch's float64 graph on the CPU, bound max(8 x torch's own float32 error of that quantity, 16 x 2^-24), the
   maximum over the four float cases, formed from the reference alone (train_ops_shapes_ref.bounds); the factor 8 is for
   another summation order over tiles, slabs and frames, a missing batch term or a skipped pass gives E >= 1e-2.  The biased
   variance is read as 1 / invstd^2 - eps.  Every test prints the share of its bound it used.
"""
import numpy as np
import pytest
import torch

import train_ops_shapes_ref as sr

hr, br = sr.hr, sr.br
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _f32(t):
    return t.to(torch.float32).to(DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(what, got, want):
    """The device's float32 tensor holds the float64 reference's numbers exactly."""
    got = got.cpu().double()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    bad = got != want
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} entries differ, first at {tuple(bad.nonzero()[0].tolist())}, "
                           f"max|diff| {float((got - want).abs().max()):.6g}")


def _equal_runs(what, a, b):
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None and v is None) or torch.equal(u, v), f"{what}: output {i} differs"


# ---- 0. the library cuts the slabs as the restated geometry does ------------------------------------------------------------
@pytest.mark.parametrize("case", sr.CBR_CASES + sr.BIAS_CASES, ids=sr.case_id)
def test_scratch_size_holds_the_slab_count(case):
    """The scratch sizes are the walks of head_plan and bias_plan for geo_of's slab count: the pieces' bytes and nothing but
    the padding to 256 in front of each piece and at the end.  One slab more or less moves a size by more than that."""
    from nano_vs_slam_amd import _lib
    lib = _lib.load()
    shape, ci, co = case
    N, H, W = sr.SHAPES[shape]
    pieces = sr.conv_bias_pieces(N, H, W, ci, co)
    got = int(lib.kp2d_conv_bias_scratch_bytes(N, H, W, ci, co))
    assert got == sr.carve(pieces) and 4 * sum(pieces) <= got < 4 * sum(pieces) + sr.ALIGN * len(pieces)
    if co % 16 == 0:
        pieces = sr.cbr_pieces(N, H, W, ci, co)
        got = int(lib.kp2d_cbr_train_scratch_bytes(N, H, W, ci, co))
        assert got == sr.carve(pieces) and 4 * sum(pieces) <= got < 4 * sum(pieces) + sr.ALIGN * len(pieces)


# ---- 1. exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.CBR_CASES, ids=sr.case_id)
def test_cbr_is_exact_on_the_dyadic_grid(case):
    from nano_vs_slam_amd import train_ops as ops
    inp = sr.dyadic_inputs(case)
    ref, head, _ = sr.exact_cbr(inp)
    used = sr.check_exact(ref, head)
    print(f"{sr.case_id(case)}: share of 2^24 used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    x, w, dy, scale, shift, mean, invstd = (_f32(inp[k]) for k in ("x", "w", "dy", "scale", "shift", "mean", "invstd"))
    y, c = ops.cbr_forward(x, w, scale, shift, sr.EXACT_SLOPE)
    _equal_runs("cbr_forward twice", (y, c), ops.cbr_forward(x, w, scale, shift, sr.EXACT_SLOPE))
    _same("c", c, ref["c"])
    _same("y", y, ref["y"])
    out = ops.cbr_backward(x, w, scale, mean, invstd, y, c, dy, sr.EXACT_SLOPE)       # fed the device's own y and c
    _equal_runs("cbr_backward twice", out, ops.cbr_backward(x, w, scale, mean, invstd, y, c, dy, sr.EXACT_SLOPE))
    without = ops.cbr_backward(x, w, scale, mean, invstd, y, c, dy, sr.EXACT_SLOPE, need_dx=False)
    assert without[3] is None
    _equal_runs("cbr_backward without dx", out[:3], without[:3])
    for k, got in zip(("dweight", "dgamma", "dbeta", "dx"), out):
        _same(k, got, ref[k])


@pytest.mark.parametrize("case", sr.BIAS_CASES, ids=sr.case_id)
def test_conv_bias_is_exact_on_the_dyadic_grid(case):
    from nano_vs_slam_amd import train_ops as ops
    inp = sr.dyadic_inputs(case)
    ref, head = sr.exact_conv_bias(inp)
    used = sr.check_exact(ref, head)
    print(f"{sr.case_id(case)}: share of 2^24 used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    x, w, dy, bias = (_f32(inp[k]) for k in ("x", "w", "dy", "bias"))
    y = ops.conv_bias_forward(x, w, bias)
    assert torch.equal(y, ops.conv_bias_forward(x, w, bias))
    _same("y", y, ref["y"])
    out = ops.conv_bias_backward(x, w, dy)
    _equal_runs("conv_bias_backward twice", out, ops.conv_bias_backward(x, w, dy))
    without = ops.conv_bias_backward(x, w, dy, need_dx=False)
    assert without[2] is None
    _equal_runs("conv_bias_backward without dx", out[:2], without[:2])
    for k, got in zip(("dweight", "dbias", "dx"), out):
        _same(k, got, ref[k])


# ---- 2. float-valued -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bounds():
    return sr.bounds()


def _run_float(case):
    """One layer forward and backward on the device -> (dict of device tensors by quantity, what the backward took)."""
    from nano_vs_slam_amd import train_ops as ops
    inp = sr.float_inputs(case)
    x, w, gamma, beta, dy = (_dev(inp[k]) for k in ("x", "w", "gamma", "beta", "dy"))
    if case[0] == "batch":
        drop = _dev(inp["drop"])
        running = (_dev(inp["running_mean"]), _dev(inp["running_var"]))
        y, c, mean, invstd = ops.cbr_forward_batch(x, w, gamma, beta, hr.BN_EPS, sr.FLOAT_SLOPE, drop, running, br.MOMENTUM)
        args = (x, w, gamma, mean, invstd, y, c, dy, sr.FLOAT_SLOPE, drop)
        dw, dgamma, dbeta, dx = ops.cbr_backward_batch(*args)
        r = dict(y=y, c=c, mean=mean, var=1.0 / (invstd.double() ** 2) - hr.BN_EPS, running_mean=running[0], running_var=running[1])
    else:
        scale, shift, mean, invstd = (t.to(DEV) for t in sr.running_vectors(inp))
        y, c = ops.cbr_forward(x, w, scale, shift, sr.FLOAT_SLOPE)
        args = (x, w, scale, mean, invstd, y, c, dy, sr.FLOAT_SLOPE)
        dw, dgamma, dbeta, dx = ops.cbr_backward(*args)
        r = dict(y=y, c=c)
    r.update(dweight=dw, dgamma=dgamma, dbeta=dbeta, dx=dx)
    return r, args


@pytest.mark.parametrize("case", sr.FLOAT_CASES, ids=sr.case_id)
def test_layer_within_the_float32_bound(bounds, case):
    ref = sr.reference(case)
    r, _ = _run_float(case)
    assert set(r) == set(ref)
    over = []
    for k in sr.QUANTITIES:
        if k not in ref:
            continue
        got = r[k].cpu().numpy().astype(np.float64)
        assert got.shape == ref[k].shape, k
        e = sr.rel_err(got, ref[k])
        print(f"{sr.case_id(case)}: E({k}) {e:.3e} = {e / bounds[k]:.3f} of {bounds[k]:.3e}")
        if not e <= bounds[k]:
            over.append(k)
    assert not over, over


def test_batch_layer_exact_statements():
    """G1 on batch statistics: a plane dropped in every frame has exactly zero y, dbeta, dgamma and dweight rows; a plane
    dropped in one frame is zero there and lives elsewhere; the running statistics moved; need_dx=False and a second run give
    the same bits."""
    from nano_vs_slam_amd import train_ops as ops
    case = sr.FLOAT_CASES[0]
    assert case[:2] == ("batch", "G1")
    inp = sr.float_inputs(case)
    r, args = _run_float(case)
    every, once = sr.DROPPED_EVERYWHERE, sr.DROPPED_ONCE
    assert not r["y"][:, every].any() and float(r["dbeta"][every]) == 0 and float(r["dgamma"][every]) == 0 and not r["dweight"][every].any()
    assert not r["y"][0, once].any() and r["y"][1:, once].any() and float(r["dbeta"][once]) != 0 and r["dweight"][once].any()
    assert not torch.equal(r["running_mean"], _dev(inp["running_mean"])) and not torch.equal(r["running_var"], _dev(inp["running_var"]))
    again, _ = _run_float(case)
    for k in r:
        assert torch.equal(again[k], r[k]), k
    without = ops.cbr_backward_batch(*args, need_dx=False)
    assert without[3] is None
    _equal_runs("cbr_backward_batch without dx", (r["dweight"], r["dgamma"], r["dbeta"]), without[:3])
