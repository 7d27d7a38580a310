"""The per-layer float64 checker of tests/layer_ref.py has teeth, and its GPU cases cover every tile form.

A numpy emulation of each arithmetic mode — split fp16 (x = xh + xl, w 2^e = wh + wl, RNE with subnormals, xh wh + xh wl +
xl wh summed in fp32 tap by tap and 16-channel chunk by chunk) and fp32 — runs one layer on seeded activations and weights
with the statistics of the real layers (K = 144 ... 576, LeakyReLU outputs of O(0.1 - 1) with their 0.01x negatives,
BatchNorm epilogues).  The faithful emulation must stay 4x below layer_ref's bound; each modelled kernel fault must exceed
it 4x at some element.  Together the two margins pin layer_ref.ALPHA from both sides.  No GPU needed."""
import ast
import os

import numpy as np
import pytest

import layer_ref as L
from oracle import kp2d_oracle as orc

H, W = 20, 40          # one and a quarter 16-row tile rows (ragged), one and a quarter 32-column tiles
RAG_Y, RAG_X = 18, 5   # a pixel of the ragged last tile row
MARGIN = 4.0


def _layer(cin, cout, seed):
    rng = np.random.default_rng(seed)
    pre = rng.normal(0.0, 0.6, (cin, H, W))
    x = np.where(pre >= 0, pre, 0.01 * pre).astype(np.float32)      # a LeakyReLU output: many |x| < 0.1, lo halves subnormal
    w = (rng.normal(0.0, 1.0, (cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    sd = {"l.conv.weight": w,
          "l.bn.weight": rng.uniform(0.5, 1.5, cout).astype(np.float32), "l.bn.bias": rng.normal(0, 0.1, cout).astype(np.float32),
          "l.bn.running_mean": rng.normal(0, 0.1, cout).astype(np.float32),
          "l.bn.running_var": rng.uniform(0.5, 2.0, cout).astype(np.float32)}
    return x, sd


def _split16(v):
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(np.float32)).astype(np.float16)


def _patches(x):
    """the nine shifted copies of x (zero padding), [9, C, H * W], tap = 3 * (dy + 1) + (dx + 1)"""
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    return np.stack([xp[:, dy:dy + H, dx:dx + W].reshape(x.shape[0], -1) for dy in range(3) for dx in range(3)])


def emulate(x, sd, mode, fault=None):
    """One 3x3 CBR (LeakyReLU) as the kernels compute it, optionally with one modelled fault."""
    w = sd["l.conv.weight"]
    cout, cin = w.shape[:2]
    s, sh = L.fold(sd, L.Spec("l", []))
    f32 = np.float32
    P = _patches(x)
    if fault == "tap_missing_at_ragged_pixel":
        P[0, :, RAG_Y * W + RAG_X] = 0.0
    if fault == "halo_row_off":
        # output row 16 (first row of the second 16-row tile) reads its dy = -1 halo from row 14 instead of row 15
        xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
        for dx in range(3):
            P[dx, :, 16 * W:17 * W] = xp[:, 14, dx:dx + W]
    acc = np.zeros((cout, H * W), f32)
    if mode == "f16x3":
        wmax = float(np.abs(w).max())
        e = 11
        while e > -96 and wmax * 2.0 ** e > 32768.0:
            e -= 1
        wh, wl = _split16((w * f32(2.0 ** e)).astype(f32))
        xh, xl = _split16(P)
        if fault == "denormals_flushed":
            xl = np.where(np.abs(xl) < 2.0 ** -14, np.float16(0), xl)
            wl = np.where(np.abs(wl) < 2.0 ** -14, np.float16(0), wl)
        terms = [(xh, wh), (xh, wl)] + ([] if fault == "xl_wh_dropped" else [(xl, wh)])
        for t in range(9):
            for c0 in range(0, cin, 16):
                for xs, ws in terms:
                    a = ws[:, c0:c0 + 16, t // 3, t % 3].astype(f32)
                    acc += a @ xs[t, c0:c0 + 16].astype(f32)
        scale = (s * f32(2.0 ** -e)).astype(f32)
    else:
        for t in range(9):
            for c0 in range(0, cin, 8):
                acc += w[:, c0:c0 + 8, t // 3, t % 3] @ P[t, c0:c0 + 8]
        scale = s
    if fault == "n_tile_halves_swapped":
        acc[5] = acc[5 + 16]
    shift = sh.copy()
    if fault == "bn_shift_twice":
        shift[7] = shift[7] * 2
    pre = acc * scale[:, None] + shift[:, None]
    y = np.where(pre >= 0, pre, pre * f32(0.01))
    return y.reshape(cout, H, W)


def ratio(x, sd, mode, fault=None, scale=1.0):
    xs = (x * np.float32(scale)).astype(np.float32)
    y64, b = L.reference(L.Spec("l", [("in", None)]), [xs], sd, split=(mode == "f16x3"))
    r, _, finite = L.check(emulate(xs, sd, mode, fault), y64, b)
    assert finite
    return r


LAYERS = [(16, 32), (32, 32), (32, 64), (64, 64)]      # K = 144, 288, 288, 576


@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
@pytest.mark.parametrize("cin,cout", LAYERS)
def test_faithful_emulation_stays_4x_below_the_bound(cin, cout, mode):
    worst = max(ratio(*_layer(cin, cout, seed), mode) for seed in range(3))
    print(f"K = {9 * cin} {mode}: faithful max err / bound = {worst:.3f}")
    assert worst <= 1.0 / MARGIN, worst


F16_FAULTS = ["xl_wh_dropped", "denormals_flushed"]
ANY_FAULTS = ["tap_missing_at_ragged_pixel", "halo_row_off", "n_tile_halves_swapped", "bn_shift_twice"]


@pytest.mark.parametrize("mode,fault", [("f16x3", f) for f in F16_FAULTS + ANY_FAULTS] + [("fp32", f) for f in ANY_FAULTS])
@pytest.mark.parametrize("cin,cout", LAYERS)
def test_every_modelled_fault_exceeds_the_bound_4x(cin, cout, mode, fault):
    if fault == "n_tile_halves_swapped" and cout < 32:
        pytest.fail("the layer needs a 32-channel N-tile")
    r = ratio(*_layer(cin, cout, 11), mode, fault)
    print(f"K = {9 * cin} {mode} {fault}: max err / bound = {r:.1f}")
    assert r >= MARGIN, r


def test_magnitude_sweep_of_the_split_stays_inside_the_bound():
    """x 2^k from k = -24 (every value an fp16 subnormal or zero) up to the largest k with max|x| 2^k < 2^16: the range
    over which the split-fp16 arithmetic is fp32-grade in the sense of the bound (include/kp2d.h KP2D_PREC_F16X3)."""
    x, sd = _layer(64, 64, 5)
    kmax = int(np.floor(np.log2(2.0 ** 16 / float(np.abs(x).max()))))
    if float(np.abs(x).max()) * 2.0 ** kmax >= 2.0 ** 16:
        kmax -= 1
    worst = {}
    for k in range(-24, kmax + 1):
        worst[k] = ratio(x, sd, "f16x3", scale=2.0 ** k)
    print("sweep max err / bound:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    assert kmax >= 14      # O(1) activations: the bound holds up to |x| ~ 2^15 and more


def test_gpu_cases_cover_every_tile_form_of_the_policy():
    """Every variant literal in conv_policy.h is declared by some case of tests/test_gpu_layer_fp64.py, which asserts
    that its declared set is exactly what its profiled forward ran and compares each such layer with float64.  A form
    added to the policy later fails here until a case reaches it."""
    forms = L.policy_variants()
    assert len(forms) >= 18, forms
    declared = set().union(*(c.variants for c in L.CASES))
    assert set(forms) <= declared, sorted(set(forms) - declared)
    assert declared <= set(forms), sorted(declared - set(forms))
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_layer_fp64.py")).read()
    assert "L.CASES" in src and "pytest.mark.gpu" in src
    ast.parse(src)


def test_reference_matches_the_oracle_cbr():
    """layer_ref's fp32-folded epilogue against the oracle's float64 CBR on the same layer: the fold differs only in
    fp32 rounding of the folded scale / shift."""
    x, sd = _layer(32, 64, 3)
    y64, b = L.reference(L.Spec("l", [("in", None)]), [x], sd, split=False)
    ref = orc.cbr(x[None].astype(np.float64), orc.cast_params(sd, np.float64), "l")[0]
    assert np.max(np.abs(y64 - ref)) <= 1e-6 * max(1.0, float(np.abs(ref).max()))
    assert np.all(b > 0)
