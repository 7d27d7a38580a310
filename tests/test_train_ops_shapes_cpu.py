"""train_ops_shapes_ref held to itself without a device: the geometry the three shapes were chosen for, the condition under
which the dyadic cases are exact in float32 in any order, torch's float32 convolution equal to its float64 one on them, and
the numpy oracles of the trainers' tests equal to the torch float64 graphs that test_gpu_train_ops_shapes.py compares the
kernels with."""
import numpy as np
import pytest
import torch

import train_ops_shapes_ref as sr

hr, br = sr.hr, sr.br


# ---- 1. geometry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(sr.SHAPES))
def test_geometry_table(shape):
    g = sr.geo_of(*sr.SHAPES[shape])
    for k, v in sr.GEOMETRY[shape].items():
        assert g[k] == v, (shape, k, g[k], v)
    assert g["tpf"] == g["tiles_x"] * g["tiles_y"] and g["slabs"] <= sr.MAX_SLABS
    assert (g["slabs"] - 1) * g["tps"] < g["tiles"] <= g["slabs"] * g["tps"]


def test_what_each_shape_reaches():
    g1, g2, g3 = (sr.geo_of(*sr.SHAPES[s]) for s in ("G1", "G2", "G3"))
    (_, H1, W1), (_, H2, W2), (_, H3, W3) = (sr.SHAPES[s] for s in ("G1", "G2", "G3"))
    # G1: ragged on both edges, two tiles per slab, slabs across frame boundaries (9 tiles per frame, odd), a short last
    # slab, three passes of a plane loop with a ragged tail
    assert H1 % sr.TH and W1 % sr.TW and g1["tps"] == 2 and g1["tpf"] % 2 and g1["last"] < g1["tps"]
    assert len(sr.straddling_slabs(g1)) == 7 and g1["HW"] == 2 * sr.PLANE_THREADS + 191
    # G2: exact tiles, three per slab, 25 per frame is no multiple of 3, a last slab of two, 12.5 passes
    assert H2 % sr.TH == 0 and W2 % sr.TW == 0 and g2["tps"] == 3 and g2["tpf"] % 3 and 1 < g2["last"] < g2["tps"]
    assert sr.straddling_slabs(g2) and g2["HW"] == 12 * sr.PLANE_THREADS + 128
    # G3: one tile per slab, ragged tiles one row and one column thick, less than one pass
    assert g3["tps"] == 1 and H3 % sr.TH == 1 and W3 % sr.TW == 1 and g3["HW"] < sr.PLANE_THREADS


def test_width_sweeps_reach_every_instantiation():
    """Every NT = 1..8 is the output width of the forward and the weight gradient (Cout) and of the data gradient (Cin), in
    the plain and in the padded form; the padded widths sit below, on and above a multiple of 16; both kernels' LDS images
    cross the 64 KB above which a launch needs its opt-in."""
    nts = set(range(1, 9))
    assert {co // 16 for _, co in sr.WIDTHS} == nts and {ci // 16 for ci, _ in sr.WIDTHS} == nts
    assert {sr.pad16(co) // 16 for _, co in sr.MASK_WIDTHS} == nts and {ci // 16 for ci, _ in sr.MASK_WIDTHS} == nts
    assert {co % 16 for _, co in sr.MASK_WIDTHS} >= {0, 1, 15}
    assert all(ci % 16 == 0 and 16 <= ci <= 128 and 1 <= co <= 128 for ci, co in sr.WIDTHS + sr.MASK_WIDTHS)
    assert min(co for _, co in sr.WIDTHS if sr.conv_lds_bytes(co) > 65536) == 96 and sr.conv_lds_bytes(128) == 96256
    assert min(co for _, co in sr.WIDTHS if sr.dw_lds_bytes(co) > 65536) == 112 and sr.dw_lds_bytes(128) == 80128
    assert {3 * (co // 16) % 4 for _, co in sr.WIDTHS} == {0, 1, 2, 3}         # idle waves in the weight gradient's last round


def test_scratch_walk():
    assert sr.carve([1]) == 256 and sr.carve([64, 1]) == 512 and sr.carve([65, 1]) == 768 and sr.carve([]) == 0
    for case in sr.CBR_CASES + sr.BIAS_CASES:
        shape, ci, co = case
        for pieces in (sr.cbr_pieces(*sr.SHAPES[shape], ci, co), sr.conv_bias_pieces(*sr.SHAPES[shape], ci, co)):
            assert 4 * sum(pieces) <= sr.carve(pieces) < 4 * sum(pieces) + sr.ALIGN * len(pieces)
            assert 4 * pieces[-1] // sr.geo_of(*sr.SHAPES[shape])["slabs"] > sr.ALIGN      # the size pins the slab count


# ---- 2. the exact cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.CBR_CASES, ids=sr.case_id)
def test_cbr_case_is_exact_in_float32(case):
    inp = sr.dyadic_inputs(case)
    ref, head, stats = sr.exact_cbr(inp)
    used = sr.check_exact(ref, head)
    print(f"{sr.case_id(case)}: share of 2^24 used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items())
          + f"; slope branch {stats['slope_share']:.2f}, pre-activations exactly 0: {stats['zeros']}")
    assert 0.3 < stats["slope_share"] < 0.7 and stats["zeros"] > 0
    # torch's own float32 convolution and its two gradients equal the float64 ones
    x, w, dc = inp["x"].float(), inp["w"].float(), (torch.where(ref["y"] > 0, inp["dy"], sr.EXACT_SLOPE * inp["dy"]) * sr._ch(inp["scale"])).float()
    assert torch.equal(sr.conv(x, w).double(), ref["c"])
    assert torch.equal(sr.conv_dw(dc, x, w).double(), ref["dweight"]) and torch.equal(sr.conv_dx(dc, x, w).double(), ref["dx"])


@pytest.mark.parametrize("case", sr.BIAS_CASES, ids=sr.case_id)
def test_conv_bias_case_is_exact_in_float32(case):
    inp = sr.dyadic_inputs(case)
    ref, head = sr.exact_conv_bias(inp)
    used = sr.check_exact(ref, head)
    print(f"{sr.case_id(case)}: share of 2^24 used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    x, w, dy = inp["x"].float(), inp["w"].float(), inp["dy"].float()
    assert torch.equal((sr.conv(x, w) + sr._ch(inp["bias"].float())).double(), ref["y"])
    assert torch.equal(sr.conv_dw(dy, x, w).double(), ref["dweight"]) and torch.equal(sr.conv_dx(dy, x, w).double(), ref["dx"])


def test_check_exact_refuses_what_does_not_fit():
    ref = {"a": torch.tensor([3.0], dtype=torch.float64), "b": torch.tensor([0.375], dtype=torch.float64)}
    sr.check_exact(ref, {"a": (2.0 ** 24 - 1, 0), "b": (0.375, 3)})
    for head in ({"a": (2.0 ** 24, 0)}, {"a": (2.0 ** 21, 3)}, {"b": (1.0, 2)}):
        with pytest.raises(AssertionError):
            sr.check_exact(ref, head)
    with pytest.raises(AssertionError):
        sr.check_exact({"a": torch.tensor([2.0 ** 24 + 1], dtype=torch.float64)}, {"a": (1.0, 0)})
    assert sr.grid_q(torch.tensor([1.0, -0.5, 0.125])) == 3 and sr.grid_q(torch.tensor([4.0])) == 0


@pytest.mark.parametrize("case", [("G1", 16, 16), ("G3", 48, 96)], ids=sr.case_id)
def test_numpy_oracle_equals_the_exact_reference(case):
    """vpr_head_training_ref's conv3x3, conv3x3_dw, conv3x3_dx, cbr_forward and cbr_backward give the same numbers: on the
    dyadic grid float64 is exact too, whatever the order."""
    inp = sr.dyadic_inputs(case)
    ref, _, _ = sr.exact_cbr(inp)
    x, w, dy, scale, shift, mean, invstd = (inp[k].numpy() for k in ("x", "w", "dy", "scale", "shift", "mean", "invstd"))
    y, c, sc, iv = hr.cbr_forward(x, w, scale / invstd, shift + mean * scale, mean, 1.0 / invstd ** 2, sr.EXACT_SLOPE, eps=0.0)
    assert np.array_equal(sc, scale) and np.array_equal(iv, invstd)
    assert np.array_equal(c, ref["c"].numpy()) and np.array_equal(y, ref["y"].numpy())
    dw, dgamma, dbeta, dx = hr.cbr_backward(x, w, scale, mean, invstd, sr.EXACT_SLOPE, y, c, dy)
    for k, got in (("dweight", dw), ("dgamma", dgamma), ("dbeta", dbeta), ("dx", dx)):
        assert np.array_equal(got, ref[k].numpy()), k
    bias_ref, _ = sr.exact_conv_bias(inp)
    assert np.array_equal(hr.conv3x3_dw(dy, x), bias_ref["dweight"].numpy()) and np.array_equal(hr.conv3x3_dx(dy, w), bias_ref["dx"].numpy())


# ---- 3. the float cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.FLOAT_CASES, ids=sr.case_id)
def test_numpy_oracle_equals_the_torch_graph(case):
    """vpr_head_bn_ref's (batch statistics) and vpr_head_training_ref's (running statistics) layer against torch's float64
    graph to 1e-10: the two references cannot drift apart."""
    inp = sr.float_inputs(case)
    ref = sr.reference(case)
    if case[0] == "batch":
        y, c, mean, var, invstd = br.cbr_forward_batch(inp["x"], inp["w"], inp["gamma"], inp["beta"], sr.FLOAT_SLOPE, inp["drop"])
        M = c.shape[0] * c.shape[2] * c.shape[3]
        rm, rv = br.running_update((inp["running_mean"], inp["running_var"]), mean, var, M)
        dw, dgamma, dbeta, dx, _ = br.cbr_backward_batch(inp["x"], inp["w"], inp["gamma"], mean, invstd, sr.FLOAT_SLOPE, y, c,
                                                         inp["dy"].astype(np.float64), inp["drop"])
        got = dict(y=y, c=c, mean=mean, var=var, running_mean=rm, running_var=rv, dweight=dw, dgamma=dgamma, dbeta=dbeta, dx=dx)
        assert not ref["y"][:, sr.DROPPED_EVERYWHERE].any() and not ref["y"][0, sr.DROPPED_ONCE].any() and ref["y"][1:, sr.DROPPED_ONCE].any()
    else:
        y, c, scale, invstd = hr.cbr_forward(inp["x"], inp["w"], inp["gamma"], inp["beta"], inp["running_mean"], inp["running_var"], sr.FLOAT_SLOPE)
        dw, dbn, dbeta, dx = hr.cbr_backward(inp["x"], inp["w"], scale, inp["running_mean"], invstd, sr.FLOAT_SLOPE, y, c, inp["dy"].astype(np.float64))
        got = dict(y=y, c=c, dweight=dw, dgamma=dbn, dbeta=dbeta, dx=dx)
    assert set(got) == set(ref)
    for k, v in got.items():
        d = float(np.abs(v - ref[k]).max())
        print(f"{sr.case_id(case)}: max|oracle - torch| of {k} {d:.2e}")
        assert v.shape == ref[k].shape and d <= 1e-10, k


def test_bounds_come_from_the_reference_alone():
    b = sr.bounds()
    errs = sr.own_float32_errors()
    assert set(b) == set(sr.QUANTITIES) and set(errs) == set(sr.FLOAT_CASES)
    for case, e in errs.items():
        assert set(e) == set(sr.QUANTITIES if case[0] == "batch" else sr.RUNNING_QUANTITIES)
    for k in sr.QUANTITIES:
        worst = max(e[k] for e in errs.values() if k in e)
        print(f"{k}: torch float32 E {worst:.3e}, bound {b[k]:.3e}")
        assert 0 < worst < 1e-4 and b[k] == max(8 * worst, 16 * 2.0 ** -24) and b[k] < 1e-3      # a missing term gives 1e-2
