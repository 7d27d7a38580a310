"""Every launch of the attention segmentation head (S_A, N_A) against float64, one launch at a time, with an error bound.

For each case of tests/attention_head_ref.py CASES and each arithmetic mode, as tests/test_gpu_layer_fp64.py does for the
plain configurations:

1. a profiled forward says which kernel ran each layer.  f16x3: attention_f16x3 (which of its forms a shape takes is
   evaluated from attention_form.h by tests/test_attention_head_ref_cpu.py), the fused mff_tail where C = 64 unless the
   case switches it off.  fp32: no split family, no mff_tail, the plain attention kernel;
2. every launch the profile lists under a convolution family or under channel_layernorm / attention* / dwconv3x3 / mff_tail
   is compared, over every element of the compared frames, with its float64 stage on the device's own tapped input(s):
   |got - ref64| <= bound and finite.  A launch that is neither modelled nor in layer_ref.EXCLUDED fails the case;
3. every tapped forward's outputs are bit-identical to the untapped forward's;
4. (f16x3) magnitude sweeps of the LayerNorm, mff_tail / depthwise / GELU and attention stages through scaled weights."""
import numpy as np
import pytest
import torch

import attention_head_ref as A
import layer_ref as L
from test_gpu_layer_fp64 import _Run

pytestmark = pytest.mark.gpu
CASES = {c.id: c for c in A.CASES}
P1 = "seg_head.convs.1"


def _launches(run, graph):
    """[(stage, split arithmetic, kernels)] of every modelled launch the profile lists; fails on one neither modelled nor excluded"""
    by_launch = {sp.launch: name for name, sp in graph.items()}
    todo = []
    for layer, kerns in sorted(run.ran.items()):
        ks = sorted(k for k in kerns if L.is_conv_family(k) or A.is_head_family(k))
        if not ks or L.excluded(layer):
            continue
        names = L.merged_parts(run.cfg) if layer == "heads.first" else [by_launch.get(layer)]
        assert all(n in graph for n in names), f"{run.case.id}: launch {layer} {ks} is neither compared nor in layer_ref.EXCLUDED"
        todo += [(n, any(L.is_split_family(k) for k in ks), ks) for n in names]
    return todo


def _fused(case, cfg, mode):
    return mode == "f16x3" and cfg["channel_dims"][4] == 64 and case.options.get("mff_fused", 1) == 1


@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
@pytest.mark.parametrize("case", A.CASES, ids=[c.id for c in A.CASES])
def test_every_head_launch_against_float64(case, mode):
    if case.id.startswith("C_"):
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert A.TAIL_TILES_C > cus, f"case C needs more mff_tail tiles ({A.TAIL_TILES_C}) than the device has CUs ({cus})"
    run = _Run(case, mode)
    graph = L.layer_graph(run.cfg)
    kernels = {k for ks in run.ran.values() for k in ks}
    todo = _launches(run, graph)
    results = []
    for name, split, ks in todo:
        worst, where, finite = run.compare(graph[name], split)
        results.append((worst, name, "/".join(ks), where, finite))
    order = sorted(results, key=lambda r: -r[0])
    print(f"\nLAYER_FP64 {case.id} [{mode}]: {len(results)} launches, worst {order[0][1]} ({order[0][2]}) err/bound = {order[0][0]:.3f} "
          f"at (frame, c, y, x) = {order[0][3]}")
    for w, name, ks, where, finite in order:
        print(f"  {w:9.4f}  {name:36s} {ks}  at {where}{'' if finite else '  NON-FINITE'}")
    # the kernels the mode and the case ask for
    att = {k for k in kernels if k.startswith("attention")}
    fused = _fused(case, run.cfg, mode)
    assert ("mff_tail" in kernels) == fused, sorted(kernels)
    if mode == "f16x3":
        assert att == {"attention_f16x3"}, att
    else:
        assert att == {"attention"} and not any(L.is_split_family(k) for k in kernels), sorted(kernels)
    # every stage ran as a launch of its own (conv1a only inside conv1b's: the stem fusion), but for the MixFFN path not taken
    missing = set(graph) - {n for n, _, _ in todo}
    other_path = {n for n in graph if ".mff" in n and n.endswith(A.UNFUSED_ONLY if fused else A.FUSED_ONLY)}
    assert other_path <= missing and missing - other_path <= {"backbone.conv1a"}, (case.id, sorted(missing))
    assert len(other_path) == (6 if fused else 2)
    if "backbone.conv1a" in missing:
        assert any("stem" in k for k in run.ran["backbone.conv1b"]), run.ran["backbone.conv1b"]
    bad = [(f"{n}: max err / bound = {w:.3g} at (frame, c, y, x) = {where}" + ("" if fin else ", non-finite"))
           for w, n, _, where, fin in results if not (w <= 1.0 and fin)]
    assert not bad, (case.id, mode, bad)


class _Scaled:
    """the run's model with some weights times 2^k (load_state_dict), restored on exit"""

    def __init__(self, run):
        self.run = run
        self.base = {k: np.array(v, copy=True) for k, v in run.sd.items()}

    def load(self, keys, k):
        sd = dict(self.base)
        for key in keys:
            sd[key] = (self.base[key] * np.float32(2.0 ** k)).astype(np.float32)
        self.run.model.load_state_dict({kk: torch.from_numpy(np.asarray(v)) for kk, v in sd.items()}, strict=True)
        self.run.ref_out = self.run._forward()
        self.run.taps = {}
        return sd

    def restore(self):
        self.run.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in self.base.items()}, strict=True)
        self.run.ref_out = self.run._forward()
        self.run.taps = {}


def _sweep(run, scaled, title, keys, ks, stages, split, peak_of):
    """keys times 2^k for k in ks: each stage against its bound while peak_of(k) < PEAK_LIMIT (peak_of: the largest operand of
    the stages' split products in the float64 reference, from the unscaled taps); beyond, the device is not run"""
    graph = L.layer_graph(run.cfg)
    lines = []
    for k in ks:
        peak = peak_of(k)
        assert np.isfinite(peak), (title, k)
        if peak >= A.PEAK_LIMIT:
            lines.append(f"  2^{k}: peak {peak:.4g} >= 2^15: the device is not run")
            continue
        sd = scaled.load(keys, k)
        for st in stages:
            worst, where, finite = run.compare(graph[st], split, sd=sd)
            lines.append(f"  {worst:9.4f}  2^{k:<4d} {st:36s} peak {peak:.4g}  at {where}{'' if finite else '  NON-FINITE'}")
            assert finite and worst <= 1.0, f"{run.case.id} {title} x 2^{k} -> {st}: max err / bound = {worst:.3g} at (frame, c, y, x) = {where}, finite: {finite}"
    print(f"\nSWEEP {run.case.id} {title}:")
    print("\n".join(lines))


def _kmax(amax):
    return int(np.floor(np.log2(65504.0 / amax)))


def test_magnitude_sweeps_of_module_1_against_float64():
    """case A, f16x3: (1) convs.0's BatchNorm weight and bias times 2^k -> the LayerNorm, from std << eps up to activations
    near 2^16; (2) mff.fn.net.0 times 2^k -> mff_tail; (3) to_q times 2^k -> attention with logits in the thousands."""
    run = _Run(CASES["A_S_A_v3_80x112"], "f16x3")
    scaled = _Scaled(run)
    try:
        # (1)
        prod = "seg_head.convs.0"
        kmax = _kmax(float(np.abs(run.tap(prod)).max()))
        _sweep(run, scaled, f"{prod} bn x 2^k -> LayerNorm", [prod + ".bn.weight", prod + ".bn.bias"],
               sorted(set(list(range(-24, kmax + 1, 4)) + [kmax])), [P1 + ".att.norm"], False, lambda k: 0.0)
        scaled.restore()
        # (2)
        f = P1 + ".mff.fn"
        h0 = run.tap(f + ".net.0").astype(np.float64)
        peak0 = {k: max(A.tail_peak(h0[i] * 2.0 ** k, run.sd, f) for i in range(len(run.case.frames))) for k in range(-24, 29, 4)}
        _sweep(run, scaled, f"{f}.net.0 x 2^k -> mff_tail", [f + ".net.0.weight", f + ".net.0.bias"], sorted(peak0),
               [P1 + ".mff"], True, lambda k: peak0[k])
        assert any(p >= A.PEAK_LIMIT for p in peak0.values()) and peak0[0] < A.PEAK_LIMIT
        scaled.restore()
        # (3)
        a = P1 + ".att.fn"
        q0, kv0 = float(np.abs(run.tap(a + ".to_q")).max()), float(np.abs(run.tap(a + ".to_kv")).max())
        _sweep(run, scaled, f"{a}.to_q x 2^k -> attention", [a + ".to_q.weight"], (-8, 0, 4, 8, 12), [a], True,
               lambda k: max(q0 * 2.0 ** k, kv0))
    finally:
        scaled.restore()


def test_magnitude_sweep_of_the_three_launch_mixffn_against_float64():
    """case B with mff_fused = 0, f16x3: mff.fn.net.0 times 2^k -> the depthwise 3x3, the 1x1 + gelu_fast and the pooled 1x1"""
    run = _Run(CASES["B_unfused"], "f16x3")
    scaled = _Scaled(run)
    try:
        f = P1 + ".mff.fn"
        h0 = run.tap(f + ".net.0").astype(np.float64)
        peak0 = {k: max(A.tail_peak(h0[i] * 2.0 ** k, run.sd, f) for i in range(len(run.case.frames))) for k in range(-24, 29, 4)}
        _sweep(run, scaled, f"{f}.net.0 x 2^k -> dwconv3x3, 1x1 + GELU, 1x1 + pool", [f + ".net.0.weight", f + ".net.0.bias"], sorted(peak0),
               [f + ".net.1.net.0", f + ".net.1.net.1", f + ".net.3"], True, lambda k: peak0[k])
        assert any(p >= A.PEAK_LIMIT for p in peak0.values()) and peak0[0] < A.PEAK_LIMIT
    finally:
        scaled.restore()
