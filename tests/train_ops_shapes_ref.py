"""Cases and float64 references of the training layer ops (nano_vs_slam_amd.train_ops; csrc/train_conv.h,
csrc/vpr_head_train.hip, csrc/seg_train.hip) past one tile per weight-gradient slab, one pass of a plane loop and the few
channel widths the trainers' fixtures reach.  test_train_ops_shapes_cpu.py holds everything here to itself without a device,
test_gpu_train_ops_shapes.py holds the kernels to it.

* The geometry: geo_of restates csrc/train_conv.h's (8 x 16 tiles, at most 128 slabs of ceil(tiles / 128) tiles), GEOMETRY
  the figures the three shapes were chosen for, carve over cbr_pieces / conv_bias_pieces the two scratch walks.
* Exact cases: inputs on a dyadic grid (small integers, signed powers of two, slope 0.5) on which every product and every
  partial sum of every quantity, in any order, is a float32 number, so the device must give the float64 result bit for
  bit.  exact_cbr / exact_conv_bias return the float64 results with, per quantity, (A, q): A the largest sum of the
  magnitudes of an entry's terms, 2^-q the grid the terms lie on; check_exact asserts A 2^q < 2^24.
* Float cases: inputs drawn the way vpr_head_training_ref.make_inputs draws them; torch_batch_graph / torch_running_graph
  run conv2d, batch_norm, leaky_relu and the dropout factors under autograd in float64 or float32 on the CPU; bounds() is
  max(8 x the float32 run's error against the float64 run, 16 x 2^-24) per quantity, the maximum over FLOAT_CASES.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import vpr_head_bn_ref as br

hr = br.hr
rel_err = hr.rel_err

# ---- geometry (csrc/train_conv.h, csrc/api_common.h) -----------------------------------------------------------------------
TH, TW, KC = 8, 16, 16
MAX_SLABS = 128
PLANE_THREADS = 256       # a plane loop's stride: for (e = tid; e < HW; e += 256)
ALIGN = 256               # a scratch piece starts, and the total ends, on a multiple of this

SHAPES = {"G1": (15, 19, 37), "G2": (11, 40, 80), "G3": (2, 9, 17)}      # N, H, W
# what each shape was chosen for: tiles_y, tiles_x, tiles, tiles per slab, slabs, tiles of the last slab, HW
GEOMETRY = {"G1": dict(tiles_y=3, tiles_x=3, tiles=135, tps=2, slabs=68, last=1, HW=703),
            "G2": dict(tiles_y=5, tiles_x=5, tiles=275, tps=3, slabs=92, last=2, HW=3200),
            "G3": dict(tiles_y=2, tiles_x=2, tiles=8, tps=1, slabs=8, last=1, HW=153)}


def geo_of(N, H, W):
    tiles_x, tiles_y = -(-W // TW), -(-H // TH)
    tpf = tiles_x * tiles_y
    tiles = N * tpf
    tps = -(-tiles // MAX_SLABS)
    slabs = -(-tiles // tps)
    return dict(tiles_x=tiles_x, tiles_y=tiles_y, tpf=tpf, tiles=tiles, tps=tps, slabs=slabs, last=tiles - (slabs - 1) * tps, HW=H * W)


def straddling_slabs(g):
    """The slabs whose tiles lie in more than one frame."""
    return [s for s in range(g["slabs"]) if (s * g["tps"]) // g["tpf"] != (min((s + 1) * g["tps"], g["tiles"]) - 1) // g["tpf"]]


def pad16(c):
    return (c + 15) & ~15


def conv_lds_bytes(co):
    return (KC * 208 + KC * 9 * (co | 16)) * 4


def dw_lds_bytes(co):
    return (co * (TH * TW + 4) + KC * 196) * 4


def carve(counts, itemsize=4):
    """Carve's walk over float pieces: each starts at the next multiple of ALIGN, and so does the end."""
    end = 0
    for n in counts:
        end = -(-end // ALIGN) * ALIGN + n * itemsize
    return -(-end // ALIGN) * ALIGN


def cbr_pieces(N, H, W, Cin, Cout):
    """head_plan's: packed weights, dc, the frames' BatchNorm sums, the slabs' weight-gradient partials (floats each)."""
    return [9 * Cin * Cout, N * Cout * H * W, N * Cout * 2, geo_of(N, H, W)["slabs"] * Cout * Cin * 9]


def conv_bias_pieces(N, H, W, Cin, Cout):
    """bias_plan's: packed weights padded to 16, the frames' bias sums, the slabs' weight-gradient partials."""
    return [9 * Cin * pad16(Cout), N * Cout, geo_of(N, H, W)["slabs"] * Cout * Cin * 9]


# ---- the cases ---------------------------------------------------------------------------------------------------------------
WIDTHS = ((16, 128), (32, 112), (48, 96), (64, 80), (80, 64), (96, 48), (112, 32), (128, 16), (128, 128))
MASK_WIDTHS = ((16, 1), (48, 15), (32, 17), (128, 47), (64, 65), (16, 100), (96, 127), (128, 128),
               (80, 50), (112, 95))      # the last two: NT = 4 and 6 as a padded Cout, NT = 5 and 7 as the masked data gradient's width
CBR_CASES = (("G1", 16, 16), ("G2", 16, 32)) + tuple(("G3", ci, co) for ci, co in WIDTHS)            # (shape, Cin, Cout)
BIAS_CASES = tuple(("G3", ci, co) for ci, co in MASK_WIDTHS) + (("G1", 16, 19), ("G2", 16, 1))
FLOAT_CASES = (("batch", "G1", 16, 16), ("batch", "G2", 16, 32), ("batch", "G3", 128, 128), ("running", "G1", 16, 16))
EXACT_SLOPE, FLOAT_SLOPE = 0.5, 0.01
# dyadic ranges: x, dy in [-3, 3], w in [-2, 2], bias in [-4, 4], shift in [-8, 8], scale +-2^-3..2^0;
# per shape: |mean| <= MEAN[shape], invstd = 2^e for e in INVSTD_EXP[shape] (G2 narrowed until dgamma fits its 35200 terms)
MEAN = {"G1": 8, "G2": 2, "G3": 8}
INVSTD_EXP = {"G1": (-2, 1), "G2": (-1, 0), "G3": (-2, 1)}


def case_id(case):
    return "-".join(str(v) for v in case)


def _seed(case):
    shape, ci, co = case[-3:]
    return 7000 + 100000 * int(shape[1]) + 300 * ci + co


def dyadic_inputs(case):
    """-> dict of float64 CPU tensors: x, w, dy, and the vectors of both layer kinds (scale, shift, mean, invstd; bias)."""
    shape, Cin, Cout = case
    N, H, W = SHAPES[shape]
    rng = np.random.default_rng(_seed(case))

    def ints(lo, hi, *size):
        return torch.from_numpy(rng.integers(lo, hi + 1, size).astype(np.float64))

    e_lo, e_hi = INVSTD_EXP[shape]
    return {"x": ints(-3, 3, N, Cin, H, W), "w": ints(-2, 2, Cout, Cin, 3, 3), "dy": ints(-3, 3, N, Cout, H, W),
            "scale": (2 * ints(0, 1, Cout) - 1) * 2.0 ** ints(-3, 0, Cout), "shift": ints(-8, 8, Cout),
            "mean": ints(-MEAN[shape], MEAN[shape], Cout), "invstd": 2.0 ** ints(e_lo, e_hi, Cout), "bias": ints(-4, 4, Cout)}


def grid_q(*arrays):
    """The smallest q >= 0 for which every entry of every array is a multiple of 2^-q."""
    for q in range(0, 64):
        if all(bool((a * 2.0 ** q == torch.round(a * 2.0 ** q)).all()) for a in arrays):
            return q
    raise AssertionError("not dyadic")


def _ch(v):
    return v[None, :, None, None]


def conv(x, w):
    return F.conv2d(x, w, padding=1)


def conv_dw(dc, x, w):
    return torch.nn.grad.conv2d_weight(x, w.shape, dc, padding=1)


def conv_dx(dc, x, w):
    return torch.nn.grad.conv2d_input(x.shape, w, dc, padding=1)


def exact_cbr(inp, slope=EXACT_SLOPE):
    """cbr_forward and cbr_backward by the formulas of include/kp2d.h -> (ref, head, stats): ref[name] the float64 result,
    head[name] = (A, q), stats the share of outputs on the slope branch and the count of pre-activations that are exactly 0.
    The backward's operands are dy, y, c and the vectors, as the call takes them."""
    x, w, dy, scale, shift, mean, invstd = (inp[k] for k in ("x", "w", "dy", "scale", "shift", "mean", "invstd"))
    assert grid_q(x, w, dy, shift, mean) == 0 and grid_q(torch.tensor(slope)) == 1
    c = conv(x, w)
    pre = c * _ch(scale) + _ch(shift)
    y = torch.where(pre > 0, pre, slope * pre)
    dpre = torch.where(y > 0, dy, slope * dy)
    dc = dpre * _ch(scale)
    ref = {"c": c, "y": y, "dbeta": dpre.sum((0, 2, 3)), "dgamma": (dpre * (c - _ch(mean)) * _ch(invstd)).sum((0, 2, 3)),
           "dweight": conv_dw(dc, x, w), "dx": conv_dx(dc, x, w)}
    ac = conv(x.abs(), w.abs())
    q_pre, q_dpre, q_dc = grid_q(scale), grid_q(dpre), grid_q(dpre) + grid_q(scale)
    head = {"c": (ac.max(), 0), "y": ((ac * _ch(scale.abs()) + _ch(shift.abs())).max(), q_pre + 1),
            "dbeta": (dpre.abs().sum((0, 2, 3)).max(), q_dpre),
            "dgamma": ((dpre.abs() * (c.abs() + _ch(mean.abs())) * _ch(invstd.abs())).sum((0, 2, 3)).max(), q_dpre + grid_q(invstd)),
            "dweight": (conv_dw(dc.abs(), x.abs(), w).max(), q_dc), "dx": (conv_dx(dc.abs(), x, w.abs()).max(), q_dc)}
    stats = {"slope_share": float((pre <= 0).double().mean()), "zeros": int((pre == 0).sum())}
    return ref, {k: (float(a), q) for k, (a, q) in head.items()}, stats


def exact_conv_bias(inp):
    """conv_bias_forward and conv_bias_backward -> (ref, head) as exact_cbr; everything is an integer."""
    x, w, dy, bias = (inp[k] for k in ("x", "w", "dy", "bias"))
    assert grid_q(x, w, dy, bias) == 0
    ref = {"y": conv(x, w) + _ch(bias), "dweight": conv_dw(dy, x, w), "dbias": dy.sum((0, 2, 3)), "dx": conv_dx(dy, x, w)}
    head = {"y": ((conv(x.abs(), w.abs()) + _ch(bias.abs())).max(), 0), "dweight": (conv_dw(dy.abs(), x.abs(), w).max(), 0),
            "dbias": (dy.abs().sum((0, 2, 3)).max(), 0), "dx": (conv_dx(dy.abs(), x, w.abs()).max(), 0)}
    return ref, {k: (float(a), q) for k, (a, q) in head.items()}


def check_exact(ref, head):
    """What makes "exact" a checked fact -> {name: A 2^q / 2^24}: every term of an entry lies on the grid 2^-q and the
    magnitudes of an entry's terms sum to at most A, so with A 2^q < 2^24 every partial sum, in any order, is an integer
    below 2^24 times 2^-q: a float32 number.  And the float64 result itself passes through float32 unchanged."""
    used = {}
    for k, (a, q) in head.items():
        used[k] = a * 2.0 ** q / 2.0 ** 24
        assert used[k] < 1.0, f"{k}: the terms' magnitudes sum to {a:.4g} on the grid 2^-{q}: {a * 2.0 ** q:.4g} >= 2^24"
        assert grid_q(ref[k]) <= q, f"{k}: off the grid 2^-{q}"
        assert torch.equal(ref[k].float().double(), ref[k]), f"{k}: does not round-trip through float32"
    return used


# ---- float cases ---------------------------------------------------------------------------------------------------------------
QUANTITIES = ("y", "c", "mean", "var", "running_mean", "running_var", "dweight", "dgamma", "dbeta", "dx")
RUNNING_QUANTITIES = ("y", "c", "dweight", "dgamma", "dbeta", "dx")
DROPPED_EVERYWHERE, DROPPED_ONCE = 3, 5        # channels of the drop mask
FLOOR = br.FLOOR


def float_inputs(case):
    """-> dict of float32 numpy arrays, drawn as vpr_head_training_ref.make_inputs draws a layer's: x, w, gamma, beta, the
    running statistics, dy, and drop [N, Cout] of 0 or 1.25 with one channel dropped in every frame and one in frame 0."""
    _, shape, Cin, Cout = case
    N, H, W = SHAPES[shape]
    rng = np.random.default_rng(_seed(case) + 1)
    x = np.stack([np.abs(rng.standard_normal((Cin, H, W))) * 0.8 + 0.3 * rng.standard_normal((Cin, 1, 1)) for _ in range(N)])
    drop = np.full((N, Cout), 1.25)
    drop[:, DROPPED_EVERYWHERE] = 0.0
    drop[0, DROPPED_ONCE] = 0.0
    inp = {"x": x, "w": rng.standard_normal((Cout, Cin, 3, 3)) * np.sqrt(2.0 / (9 * Cin)), "gamma": rng.uniform(0.5, 1.5, Cout),
           "beta": 0.2 * rng.standard_normal(Cout), "running_mean": 0.3 * rng.standard_normal(Cout),
           "running_var": rng.uniform(0.5, 1.5, Cout), "dy": rng.standard_normal((N, Cout, H, W)), "drop": drop}
    return {k: v.astype(np.float32) for k, v in inp.items()}


def _leaves(inp, dtype):
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items()}
    for k in ("x", "w", "gamma", "beta"):
        t[k].requires_grad_(True)
    return t


def _grads(t, c, y, out):
    y.backward(t["dy"])
    out.update(y=y.detach(), c=c.detach(), dweight=t["w"].grad, dgamma=t["gamma"].grad, dbeta=t["beta"].grad, dx=t["x"].grad)
    return out


def torch_batch_graph(inp, dtype, slope=FLOAT_SLOPE):
    """conv2d, batch_norm(training=True) with the running update, leaky_relu, times the dropout factors, and autograd with
    dy, all in ``dtype`` on the CPU -> dict of QUANTITIES."""
    t = _leaves(inp, dtype)
    c = conv(t["x"], t["w"])
    rm, rv = t["running_mean"].clone(), t["running_var"].clone()
    y = F.leaky_relu(F.batch_norm(c, rm, rv, t["gamma"], t["beta"], True, br.MOMENTUM, hr.BN_EPS), slope) * t["drop"][:, :, None, None]
    out = {"mean": c.detach().mean((0, 2, 3)), "var": c.detach().var((0, 2, 3), unbiased=False), "running_mean": rm, "running_var": rv}
    return _grads(t, c, y, out)


def running_vectors(inp):
    """(scale, shift, mean, invstd) in float32, formed with torch the way train_ops.bn_vectors forms them."""
    gamma, beta, mean, var = (torch.from_numpy(inp[k]) for k in ("gamma", "beta", "running_mean", "running_var"))
    invstd = 1.0 / torch.sqrt(var + hr.BN_EPS)
    scale = gamma * invstd
    return scale, beta - mean * scale, mean, invstd


def torch_running_graph(inp, dtype, slope=FLOAT_SLOPE):
    """The same layer on its running statistics, no dropout -> dict of RUNNING_QUANTITIES."""
    t = _leaves(inp, dtype)
    c = conv(t["x"], t["w"])
    y = F.leaky_relu(F.batch_norm(c, t["running_mean"], t["running_var"], t["gamma"], t["beta"], False, br.MOMENTUM, hr.BN_EPS), slope)
    return _grads(t, c, y, {})


def torch_graph(case, dtype):
    return (torch_batch_graph if case[0] == "batch" else torch_running_graph)(float_inputs(case), dtype)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The float64 run of a float case, computed once and shared: nobody writes to it."""
    return {k: v.numpy() for k, v in torch_graph(case, torch.float64).items()}


@functools.lru_cache(maxsize=None)
def own_float32_errors():
    """-> {case: {quantity: E of torch's float32 run against its float64 run}}"""
    return {case: {k: rel_err(v.numpy(), reference(case)[k]) for k, v in torch_graph(case, torch.float32).items()} for case in FLOAT_CASES}


def bounds():
    """-> {quantity: max(8 x torch's own float32 error, 16 x 2^-24)}, the maximum over FLOAT_CASES; from the reference alone."""
    errs = own_float32_errors()
    return {k: max(8.0 * max(e[k] for e in errs.values() if k in e), FLOOR) for k in QUANTITIES}
