"""The stage references of tests/attention_head_ref.py have teeth, and its GPU cases reach the attention forms they name.

Inputs: the float32 oracle's own intermediates of the GPU cases' seeded weights and frames (same configurations, same frame
sizes, so the same maps: 20 x 28 and 10 x 14, 18 x 22 and the odd 9 x 11, C = 64 and 48), computed once per case.  For every
stage of both modules a numpy float32 emulation of the launch — the same order class of operations as the kernel, products
split into float16 hi / lo where the device splits — must stay 4x below the stage's bound, and every modelled kernel fault
must exceed the bound 4x at some element.  Together the two margins pin every constant of attention_head_ref (and
layer_ref.GELU_ERR, measured here) from both sides; none is fitted to a device measurement.  No GPU needed."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import attention_head_ref as A
import layer_ref as L
from oracle import kp2d_oracle as orc
from oracle.weights import state_dict_for, synthetic_frames

f32 = np.float32
MARGIN = 4.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nano-vs-slam_amd", "csrc")
CASES = {c.id: c for c in A.CASES}
CPU_CASES = ["A_S_A_v3_80x112", "B_S_A_v2_72x88", "D_N_A_v3_72x88"]      # (C's maps: the same stages on 34 x 34 / 17 x 17)


# ---------------------------------------------------------------------------------------------------------------------
# inputs: every tap of the two modules from the float32 oracle, frame 0 of the case
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_taps(cid):
    c = CASES[cid]
    cfg = orc.get_config(c.config, c.v3)
    sd = state_dict_for("spread", orc.state_dict_shapes(cfg, c.ncls), seed=1234)
    x = synthetic_frames(c.B, c.H, c.W, seed=41)[:1]
    xb, _ = orc.backbone(x, sd, cfg)
    t = {"seg_head.convs.0": orc.cbr(xb, sd, "seg_head.convs.0", cfg["leaky_relu"])}
    src = "seg_head.convs.0"
    for p, pool in (("seg_head.convs.1", True), ("seg_head.convs.2", False)):
        a, m = p + ".att", p + ".mff"
        t[a + ".norm"] = orc.channel_layernorm(t[src], sd[a + ".norm.g"], sd[a + ".norm.b"])
        t[a + ".fn.to_q"] = orc.conv2d_1x1(t[a + ".norm"], sd[a + ".fn.to_q.weight"])
        t[a + ".fn.to_kv"] = orc.conv2d_2x2_s2(t[a + ".norm"], sd[a + ".fn.to_kv.weight"])
        out = orc.efficient_self_attention(t[a + ".norm"], sd, a + ".fn")
        att = A.attention_ref(t[a + ".fn.to_q"][0], t[a + ".fn.to_kv"][0], False)[0].astype(f32)[None]
        assert np.abs(orc.conv2d_1x1(att, sd[a + ".fn.to_out.weight"]) - out).max() <= 1e-4 * max(1.0, np.abs(out).max())
        t[a + ".fn"], t[a + ".fn.to_out"] = att, out
        t[m + ".norm"] = orc.channel_layernorm(out, sd[m + ".norm.g"], sd[m + ".norm.b"])
        f = m + ".fn.net."
        t[f + "0"] = orc.conv2d_1x1(t[m + ".norm"], sd[f + "0.weight"], sd[f + "0.bias"])
        t[f + "1.net.0"] = orc.dwconv2d_3x3(t[f + "0"], sd[f + "1.net.0.weight"], sd[f + "1.net.0.bias"])
        t[f + "1.net.1"] = orc.gelu_erf(orc.conv2d_1x1(t[f + "1.net.0"], sd[f + "1.net.1.weight"], sd[f + "1.net.1.bias"]))
        y = orc.conv2d_1x1(t[f + "1.net.1"], sd[f + "3.weight"], sd[f + "3.bias"])
        t[f + "3"] = t[m] = orc.maxpool2(y) if pool else y
        src = m
    graph = L.layer_graph(cfg)
    return cfg, sd, {k: np.ascontiguousarray(v[0], dtype=f32) for k, v in t.items()}, graph


def module_stages(graph):
    return [sp for name, sp in graph.items() if ".att." in name or ".mff" in name]


# ---------------------------------------------------------------------------------------------------------------------
# float32 emulations of the launches
# ---------------------------------------------------------------------------------------------------------------------
def split16(v):
    with np.errstate(over="ignore"):
        hi = v.astype(np.float16)
        return hi, (v - hi.astype(f32)).astype(np.float16)


def weight_exp(w):
    wmax, e = float(np.abs(w).max()), 11
    while e > -96 and wmax * 2.0 ** e > 32768.0:
        e -= 1
    return e


def emu_matmul(w, x, split, drop=None, chunk=16):
    """w [Co, K] . x [K, N] in fp32, 16 channels at a time; split: wh xh + wl xh + wh xl with w scaled by 2^e (returned scale
    2^-e).  drop = (k-step, "xl" | "wl"): that cross term of that K-step is left out."""
    Co, K = w.shape
    acc = np.zeros((Co, x.shape[1]), f32)
    if not split:
        for c0 in range(0, K, 8):
            acc += w[:, c0:c0 + 8] @ x[c0:c0 + 8]
        return acc, f32(1.0)
    e = weight_exp(w)
    wh, wl = split16((w * f32(2.0 ** e)).astype(f32))
    xh, xl = split16(x)
    for i, c0 in enumerate(range(0, K, chunk)):
        sl = slice(c0, c0 + chunk)
        if not (drop and drop == (i, "wl")):
            acc += wl[:, sl].astype(f32) @ xh[sl].astype(f32)
        if not (drop and drop == (i, "xl")):
            acc += wh[:, sl].astype(f32) @ xl[sl].astype(f32)
        acc += wh[:, sl].astype(f32) @ xh[sl].astype(f32)
    return acc, f32(2.0 ** -e)


def gelu_fast32(x):
    """conv_common.h gelu_fast in numpy float32 (rcp and exp2 correctly rounded)"""
    x = x.astype(f32)
    z = np.abs(x) * f32(0.70710678118654752)
    t = f32(1.0) / (f32(0.3275911) * z + f32(1.0))
    p = f32(1.061405429) * t + f32(-1.453152027)
    p = p * t + f32(1.421413741)
    p = p * t + f32(-0.284496736)
    p = p * t + f32(0.254829592)
    e = np.exp2(f32(-1.44269504088896340736) * z * z).astype(f32)
    erf_abs = f32(1.0) - p * t * e
    return f32(0.5) * x * (f32(1.0) + np.copysign(erf_abs, x))


def gelu_tanh32(x):
    x = x.astype(f32)
    return f32(0.5) * x * (f32(1.0) + np.tanh(f32(0.7978845608) * (x + f32(0.044715) * x * x * x)))


def pool2(y, partner_row=1):
    C, H, W = y.shape
    H2, W2 = H // 2, W // 2
    r0 = y[:, 0:2 * H2:2]
    rows = np.minimum(np.arange(0, 2 * H2, 2) + partner_row, H - 1)
    r1 = y[:, rows]
    m = np.maximum(r0, r1)
    return np.maximum(m[:, :, 0:2 * W2:2], m[:, :, 1:2 * W2:2])


def emu_pw(sp, x, sd, split, fault=None):
    """a 1x1 layer (or the 2x2 stride-2 to_kv as a 1x1 over its four taps) with its bias, GELU and pooled store"""
    w = np.asarray(sd[sp.name + ".weight"], f32)
    k = w.shape[-1]
    C, H, W = x.shape
    if k == 2:
        if fault == "kv_taps_transposed":
            w = w.transpose(0, 1, 3, 2)
        H, W = H // 2, W // 2
        cols = np.concatenate([x[:, dy:2 * H:2, dx:2 * W:2].reshape(C, -1) for dy in range(2) for dx in range(2)])
        wm = np.concatenate([w[:, :, dy, dx] for dy in range(2) for dx in range(2)], axis=1)
    else:
        cols, wm = x.reshape(C, -1), w[:, :, 0, 0]
    acc, sc = emu_matmul(np.ascontiguousarray(wm), np.ascontiguousarray(cols), split, drop=(1, "xl") if fault == "cross_term_dropped" else None)
    b = sd.get(sp.name + ".bias")
    pre = acc * sc + (np.asarray(b, f32)[:, None] if b is not None else f32(0.0))
    y = {"none": lambda v: v, "gelu": gelu_tanh32 if fault == "tanh_gelu" else gelu_fast32}[sp.act](pre).reshape(-1, H, W)
    return pool2(y, 2 if fault == "pool_wrong_row" else 1) if sp.post == "pool" else y


def tree_sum(a):
    n = 1
    while n < a.shape[0]:
        n *= 2
    a = np.concatenate([a, np.zeros((n - a.shape[0],) + a.shape[1:], f32)])
    while a.shape[0] > 1:
        h = a.shape[0] // 2
        a = a[:h] + a[h:]
    return a[0]


def emu_ln(sp, x, sd, fault=None):
    C = x.shape[0]
    g, b = np.asarray(sd[sp.name + ".g"], f32).reshape(C, 1, 1), np.asarray(sd[sp.name + ".b"], f32).reshape(C, 1, 1)
    inv = f32(1.0) / f32(C)
    v = x - tree_sum(x) * inv
    q = tree_sum(v * v)
    if fault == "unbiased_variance":
        d = np.sqrt(q * (f32(1.0) / f32(C - 1))) + f32(1e-5)
    elif fault == "eps_under_sqrt":
        d = np.sqrt(q * inv + f32(1e-5))
    else:
        d = np.sqrt(q * inv) + f32(1e-5)
    return ((v / d).astype(np.float64) * g + b).astype(f32)      # (the multiply-add contracts to an FMA)


def emu_attention(q, kv, split, fault=None, heads=A.HEADS):
    """the streaming kernels: 32-key tiles (64 in fp32), a running maximum, the accumulator rescaled when it moves; f16x3:
    q' = q * scale * log2 e, split operands for both products, exp2, the denominator summed from the split probabilities"""
    C, h, w = q.shape
    d, S = C // heads, h * w
    scale = f32(1.0) / np.sqrt(f32(16 if fault == "scale_of_padded_head_dim" else d))
    out = np.zeros((C, S), f32)
    for hd in range(heads):
        qh = q[hd * d:(hd + 1) * d].reshape(d, S)
        kh = kv[hd * d:(hd + 1) * d].reshape(d, -1).T.copy()      # T, d
        vh = kv[C + hd * d:C + (hd + 1) * d].reshape(d, -1).T.copy()
        T = kh.shape[0]
        if fault == "padding_key_admitted":
            kh, vh = np.concatenate([kh, np.zeros((1, d), f32)]), np.concatenate([vh, np.zeros((1, d), f32)])
            T += 1
        tile = 32 if split else 64
        m, l, o = np.zeros(S, f32), np.zeros(S, f32), np.zeros((d, S), f32)
        if split:
            qs = qh * f32(scale * f32(1.44269504088896340736))
            q_hi, q_lo = split16(qs)
        for i, k0 in enumerate(range(0, T, tile)):
            kt, vt = kh[k0:k0 + tile], vh[k0:k0 + tile]
            if split:
                k_hi, k_lo = split16(kt)
                sc = -m[None] + k_lo.astype(f32) @ q_hi.astype(f32)
                sc = sc + k_hi.astype(f32) @ q_lo.astype(f32)
                sc = sc + k_hi.astype(f32) @ q_hi.astype(f32)
            else:
                sc = (kt @ qh) * scale - m[None]
            mx = sc.max(axis=0)
            delta = mx if i == 0 else np.maximum(mx, f32(0.0))
            m = m + delta
            sc = sc - delta[None]
            if i > 0 and not (fault == "accumulator_not_rescaled" and i == 1):
                alpha = (np.exp2(-delta) if split else np.exp(-delta)).astype(f32)
                o, l = o * alpha[None], l * alpha
            p = (np.exp2(sc) if split else np.exp(sc)).astype(f32)
            if split:
                p_hi, p_lo = split16(p)
                v_hi, v_lo = split16(vt)
                o = o + v_lo.astype(f32).T @ p_hi.astype(f32)
                o = o + v_hi.astype(f32).T @ p_lo.astype(f32)
                o = o + v_hi.astype(f32).T @ p_hi.astype(f32)
                l = l + (p_hi.astype(f32) + p_lo.astype(f32)).sum(axis=0)
            else:
                o = o + vt.T @ p
                l = l + p.sum(axis=0)
        out[hd * d:(hd + 1) * d] = o * (f32(1.0) / l)[None]
    return out.reshape(C, h, w)


def emu_dw(x, w, b, fault=None):
    """nine multiply-adds on top of the bias, in tap order"""
    C, H, W = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    acc = np.broadcast_to(np.asarray(b, f32)[:, None, None], x.shape).copy()
    for dy in range(3):
        for dx in range(3):
            v = xp[:, dy:dy + H, dx:dx + W].copy()
            if fault == "dw_tap_zero_at_tile_edge" and dy == 1 and dx == 0 and W > 16:
                v[:, :, 16] = 0.0      # the left neighbour of the first column of the second 16 x 16 tile
            # (an FMA: one rounding)
            acc = (acc.astype(np.float64) + v.astype(np.float64) * np.asarray(w, np.float64)[:, 0, dy, dx][:, None, None]).astype(f32)
    return acc


def emu_tail(sp, x, sd, fault=None):
    """mff_tail.hip: depthwise (fp32) -> split -> W1 -> + bias, gelu_fast -> split -> W3 (K in the kernel's permutation: the
    same sum) -> + bias -> max-pool"""
    p = sp.prefix
    C, H, W = x.shape
    y = emu_dw(x, sd[p + ".net.1.net.0.weight"], sd[p + ".net.1.net.0.bias"], fault).reshape(C, -1)
    acc, sc = emu_matmul(np.asarray(sd[p + ".net.1.net.1.weight"], f32)[:, :, 0, 0], y, True)
    pre = acc * sc + np.asarray(sd[p + ".net.1.net.1.bias"], f32)[:, None]
    g = (gelu_tanh32 if fault == "tanh_gelu" else gelu_fast32)(pre)
    if fault == "k_permutation_swapped":
        g = g.copy()
        g[[4, 8]] = g[[8, 4]]      # positions 4 and 8 of K-step 0 hold channels 8 and 4: read the other way round
    acc, sc = emu_matmul(np.asarray(sd[p + ".net.3.weight"], f32)[:, :, 0, 0], np.ascontiguousarray(g), True,
                         drop=(3, "xl") if fault == "cross_term_dropped" else None)
    out = (acc * sc + np.asarray(sd[p + ".net.3.bias"], f32)[:, None]).reshape(-1, H, W)
    return pool2(out, 2 if fault == "pool_wrong_row" else 1) if sp.pool else out


def emulate(sp, inputs, sd, split, fault=None):
    if isinstance(sp, A.LayerNorm):
        return emu_ln(sp, inputs[0], sd, fault)
    if isinstance(sp, A.Attention):
        return emu_attention(inputs[0], inputs[1], split, fault)
    if isinstance(sp, A.Depthwise):
        return emu_dw(inputs[0], sd[sp.name + ".weight"], sd[sp.name + ".bias"], fault)
    if isinstance(sp, A.Tail):
        return emu_tail(sp, inputs[0], sd, fault)
    return emu_pw(sp, inputs[0], sd, split, fault)


def ratio(cid, name, mode, fault=None, scale=1.0):
    cfg, sd, taps, graph = case_taps(cid)
    sp = graph[name]
    split = mode == "f16x3"
    inputs = [(taps[s] * f32(scale)).astype(f32) for s, _ in sp.srcs]
    y64, b = L.reference(sp, inputs, sd, split)
    r, where, finite = L.check(emulate(sp, inputs, sd, split, fault), y64, b)
    assert finite and np.all(b > 0)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------
def test_gelu_err_is_the_measured_value():
    """layer_ref.GELU_ERR = 2 x the largest |gelu_fast (numpy float32) - gelu64| / |x| over a dense grid of [-12, 12]"""
    x = np.linspace(-12.0, 12.0, 2400001).astype(f32)
    x = x[x != 0]
    err = np.abs(gelu_fast32(x).astype(np.float64) - orc.gelu_erf(x.astype(np.float64))) / np.abs(x.astype(np.float64))
    worst = float(err.max())
    print(f"gelu_fast (float32 emulation) against the exact-erf GELU: max |err| / |x| = {worst:.3e} at x = {float(x[err.argmax()]):.4f}; "
          f"GELU_ERR = {L.GELU_ERR:.3e}")
    assert 2 * worst <= L.GELU_ERR <= 2 * worst * 1.05, (worst, L.GELU_ERR)
    # the slope the pre-activation bound passes through GELU with
    xs = np.linspace(-6, 6, 120001)
    slope = np.abs(np.diff(orc.gelu_erf(xs)) / np.diff(xs)).max()
    assert slope <= L.GELU_SLOPE <= slope * 1.01, slope


@pytest.mark.parametrize("cid", CPU_CASES)
def test_stage_chain_is_the_oracle_module(cid):
    """the float64 stages, chained from the oracle's module input, give the oracle's module output (both MixFFN paths)"""
    c = CASES[cid]
    cfg, sd, taps, graph = case_taps(cid)
    val = {"seg_head.convs.0": taps["seg_head.convs.0"].astype(np.float64)}
    for sp in module_stages(graph):
        y, b = L.reference(sp, [val[s] for s, _ in sp.srcs], sd, True)
        assert np.all(b > 0) and np.isfinite(b).all()
        if isinstance(sp, A.Tail) and cfg["channel_dims"][4] == 64:      # (the fused tail exists for C = 64)
            assert np.abs(y - val[sp.name[:-len(".mff")] + ".mff.fn.net.3"]).max() <= 1e-12 * max(1.0, np.abs(y).max())
        val[sp.name] = y
    p64 = orc.cast_params(sd, np.float64)
    x = val["seg_head.convs.0"][None]
    m1 = orc.maxpool2(orc.attention_module(x, p64, "seg_head.convs.1"))
    m2 = orc.attention_module(m1, p64, "seg_head.convs.2")
    for name, ref in (("seg_head.convs.1.mff", m1), ("seg_head.convs.2.mff", m2)):
        assert val[name].shape == ref[0].shape, (name, val[name].shape, ref.shape)
        assert np.abs(val[name] - ref[0]).max() <= 1e-9 * max(1.0, np.abs(ref).max()), name
    hs = c.maps(cfg["downsample"])
    assert val["seg_head.convs.1.att.fn.to_q"].shape[1:] == hs[0] and val["seg_head.convs.2.att.fn.to_q"].shape[1:] == hs[1]


@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
@pytest.mark.parametrize("cid", CPU_CASES)
def test_faithful_emulations_stay_4x_below_the_bounds(cid, mode):
    cfg, sd, taps, graph = case_taps(cid)
    worst = {}
    for sp in module_stages(graph):
        if isinstance(sp, A.Tail) and (mode == "fp32" or cfg["channel_dims"][4] != 64):
            continue
        worst[sp.name] = ratio(cid, sp.name, mode)
        if isinstance(sp, A.LayerNorm):      # the bound follows the input down to 2^-24 of its scale (std << eps)
            worst[sp.name + " x 2^-24"] = ratio(cid, sp.name, mode, scale=2.0 ** -24)
    print(f"\n{cid} [{mode}] faithful max err / bound:")
    for k, v in worst.items():
        print(f"  {v:8.4f}  {k}")
    # (at 2^-24 the output is b + O(1e-3) and its own rounding, up to half of the 2^-23 |y| term, is all the error there is)
    bad = {k: v for k, v in worst.items() if not v <= (1.0 if "2^-24" in k else 1.0 / MARGIN)}
    assert not bad, bad


P1, P2 = "seg_head.convs.1", "seg_head.convs.2"
A_, B_, D_ = CPU_CASES
FAULTS = [
    # (case, stage, mode, fault)
    (A_, P1 + ".att.fn.to_q", "f16x3", "cross_term_dropped"),
    (D_, P1 + ".mff.fn.net.0", "f16x3", "cross_term_dropped"),
    (D_, P1 + ".mff.fn.net.1.net.1", "f16x3", "cross_term_dropped"),
    (A_, P1 + ".mff", "f16x3", "cross_term_dropped"),
    (A_, P1 + ".mff", "f16x3", "k_permutation_swapped"),
    (A_, P1 + ".mff", "f16x3", "tanh_gelu"),
    (B_, P2 + ".mff", "f16x3", "cross_term_dropped"),
    (A_, P2 + ".mff", "f16x3", "tanh_gelu"),
    (B_, P1 + ".mff.fn.net.1.net.1", "f16x3", "tanh_gelu"),
    (D_, P1 + ".mff.fn.net.1.net.1", "fp32", "tanh_gelu"),
    (A_, P1 + ".mff", "f16x3", "dw_tap_zero_at_tile_edge"),
    (B_, P1 + ".mff.fn.net.1.net.0", "f16x3", "dw_tap_zero_at_tile_edge"),
    (A_, P1 + ".mff", "f16x3", "pool_wrong_row"),
    (B_, P1 + ".mff.fn.net.3", "f16x3", "pool_wrong_row"),
    (A_, P1 + ".att.norm", "f16x3", "unbiased_variance"),
    (D_, P2 + ".mff.norm", "fp32", "unbiased_variance"),
    (A_, P1 + ".att.norm", "f16x3", "eps_under_sqrt"),
    (D_, P1 + ".mff.norm", "fp32", "eps_under_sqrt"),
    (D_, P1 + ".att.fn", "f16x3", "scale_of_padded_head_dim"),
    (A_, P1 + ".att.fn", "f16x3", "padding_key_admitted"),
    (D_, P2 + ".att.fn", "fp32", "padding_key_admitted"),
    (A_, P1 + ".att.fn", "f16x3", "accumulator_not_rescaled"),
    (A_, P1 + ".att.fn", "fp32", "accumulator_not_rescaled"),
    (B_, P2 + ".att.fn.to_kv", "f16x3", "kv_taps_transposed"),
    (D_, P1 + ".att.fn.to_kv", "fp32", "kv_taps_transposed"),
]


@pytest.mark.parametrize("cid,stage,mode,fault", FAULTS, ids=[f"{f[3]}-{f[1].split('convs.')[1]}-{f[0][0]}-{f[2]}" for f in FAULTS])
def test_every_modelled_fault_exceeds_the_bound_4x(cid, stage, mode, fault):
    r = ratio(cid, stage, mode, fault)
    print(f"{cid} {stage} [{mode}] {fault}: max err / bound = {r:.1f}")
    assert r >= MARGIN, r


# ---------------------------------------------------------------------------------------------------------------------
# attention_form.h for the GPU cases, with the library's default tuning values
# ---------------------------------------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "attention_form.h"
#include "options.h"
using namespace kp2d;
namespace kp2d { void set_last_error(const char*) {} }
static const char* no_env(const char*) { return nullptr; }
int main(int argc, char** argv) {
  const Tuning t = tuning_from_env(no_env);      // the defaults
  for (int i = 1; i + 5 <= argc; i += 5) {
    AttForm f;
    const int e = choose_attention(atoi(argv[i]), atoi(argv[i + 1]), 4, atoi(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4]),
                                   t.att_ksplit, t.att_q, t.att_affine, f);
    std::printf("%d %d %d %d\n", e, f.kernel, f.inst, (int)f.affine);
  }
  return 0;
}
"""
KERNEL = {0: "fp32", 1: "ksplit", 2: "split"}


def test_gpu_cases_reach_the_attention_forms_they_name(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is required to evaluate attention_form.h")
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = tmp_path / "driver"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(tmp_path / "driver.cpp"), os.path.join(CSRC, "options.cpp"),
                    "-o", str(exe)], check=True)
    rows, argv = [], []
    for c in A.CASES:
        cfg = orc.get_config(c.config, c.v3)
        for i, (h, w) in enumerate(c.maps(cfg["downsample"])):
            for prec in (1, 0):
                rows.append((c, i, prec))
                argv += [h * w, (h // 2) * (w // 2), c.B, cfg["channel_dims"][4], prec]
    out = subprocess.run([str(exe)] + [str(v) for v in argv], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(rows)
    reached = set()
    for (c, i, prec), ln in zip(rows, out):
        e, kern, inst, aff = (int(v) for v in ln.split())
        assert e == 0, (c.id, i, prec)
        if prec == 0:
            assert (KERNEL[kern], inst) == ("fp32", 1), (c.id, i, ln)
        else:
            assert (KERNEL[kern], inst, bool(aff)) == c.forms[i], (c.id, i, ln, c.forms[i])
            reached.add(c.forms[i])
    assert reached == {A.KSPLIT, A.SPLIT256, A.SPLIT256_AFFINE, A.SPLIT512_AFFINE}, reached


def test_cases_reach_what_they_are_named_for():
    """the reasons of the case table that are plain arithmetic on the shapes"""
    c = CASES["A_S_A_v3_80x112"]
    (h1, w1), (h2, w2) = c.maps(2)
    assert (h1 * w1) % 32 and (h1 // 2) * (w1 // 2) >= 128 and (h1 // 2) * (w1 // 2) % 32      # ragged query group and key tile
    assert h1 % 16 and w1 % 16 and h1 > 16 and w1 > 16 and h2 < 16 and w2 < 16              # 2 x 2 ragged tiles; one ragged tile
    c = CASES["B_S_A_v2_72x88"]
    (h1, w1), (h2, w2) = c.maps(2)
    assert h2 % 2 and w2 % 2 and (c.B * 4) % 8 == 0
    assert 256 * 4 * 4 // (h2 * w2) >= c.B      # dwconv3x3: a 256-thread block's 4096 pixels span both frames of module 2
    assert CASES["B_unfused"].options["mff_fused"] == 0
    c = CASES["C_S_A_v3_30x136x136"]
    (h1, w1), (h2, w2) = c.maps(2)
    assert -(-h1 // 16) * -(-w1 // 16) * c.B == A.TAIL_TILES_C == 270 and h2 % 2 and w2 % 2
    assert orc.get_config("N_A", True)["channel_dims"][4] == 48 and orc.get_config("S_A", True)["channel_dims"][4] == 64
    # nothing excuses the modules' launches any more
    assert L.excluded("seg_head.convs.1.att.fn.to_q") is None and L.excluded("seg_head.convs.2.mff.fn.net.3") is None
    assert L.excluded("vlad_head.netvlad")
