"""Every convolution layer of the engine, in every tile form the policy can pick, against float64 with an error bound.

For each case of tests/layer_ref.py CASES (config, frame shape, kp2d_set_option tile-form options) and each arithmetic
mode:

1. a profiled forward (kp2d_profile_get) says which kernel family and tile form ran each layer; in f16x3 the set of
   conv3x3_f16x3 forms must be exactly the one the case declares (tests/test_layer_ref_cpu.py checks that the cases
   together declare every form conv_policy.h has);
2. every layer the profile lists under a convolution family is compared, over every pixel of the compared frames, with
   layer_ref.reference on the device's own tapped input(s): |got - ref64| <= bound and finite.  A conv layer that is
   neither modelled nor in layer_ref.EXCLUDED fails the case;
3. every tapped forward's outputs are bit-identical to the untapped forward's (taps switch off the levels schedule,
   the grouped multi-launch and, on conv1a, the stem fusion: what a per-layer pass says must hold for the shipped path);
4. (f16x3, the cases with a sweep) the producing layer's BatchNorm weight and bias are scaled by 2^k, so its activation
   scales by 2^k, and the consumer is checked against the bound from k = -24 up to where the activation nears 2^16.
"""
import numpy as np
import pytest
import torch

import layer_ref as L
from conftest import product_model
from oracle import kp2d_oracle as orc
from oracle.weights import synthetic_frames

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _profile(model, x):
    """{layer: kernel family + tile form} of one forward, read back through kp2d_profile_get."""
    import ctypes as C
    eng = model._engine
    lib = eng.lib
    lib.kp2d_set_profiling(eng.handle, 1)
    with torch.no_grad():
        model(x)
    torch.cuda.synchronize()
    out = {}
    layer, kern = C.c_char_p(), C.c_char_p()
    ms, fl, by = C.c_float(), C.c_double(), C.c_double()
    for i in range(lib.kp2d_profile_count(eng.handle)):
        lib.kp2d_profile_get(eng.handle, i, C.byref(layer), C.byref(kern), C.byref(ms), C.byref(fl), C.byref(by))
        out.setdefault(layer.value.decode(), set()).add(kern.value.decode())
    lib.kp2d_set_profiling(eng.handle, 0)
    return out


def _set_options(model, options):
    eng = model._engine
    for k, v in options.items():
        assert eng.lib.kp2d_set_option(eng.handle, k.encode(), int(v)) == 0, k


class _Run:
    """One model, frames and options: untapped outputs, and taps of the compared frames (every tapped forward checked
    bit-identical to the untapped one)."""

    def __init__(self, case, mode):
        self.case, self.mode = case, mode
        self.model, self.sd = product_model(case.config, case.v3, case.ncls)
        self.cfg = orc.get_config(case.config, case.v3)
        self.x = torch.from_numpy(synthetic_frames(case.B, case.H, case.W, seed=41)).to(DEV)
        self.fr = torch.tensor(case.frames, device=DEV)
        self.model.set_precision(mode)
        with torch.no_grad():
            self.model(self.x[:1])                 # (creates the engine)
        _set_options(self.model, case.options)
        self.shapes = L.tap_shapes(self.cfg, self.sd, case.H, case.W)
        self.ran = _profile(self.model, self.x)
        self.ref_out = self._forward()
        self.taps = {}

    def _forward(self):
        with torch.no_grad():
            return {k: v.clone() for k, v in self.model(self.x).items()}

    def tap(self, name):
        if name == "@x":
            return self.x.index_select(0, self.fr).cpu().numpy()
        if name not in self.taps:
            with torch.no_grad():
                out, t = self.model.forward_with_tap(self.x, name, self.shapes[name])
            for k, v in self.ref_out.items():
                assert torch.equal(out[k], v), f"{self.case.id} [{self.mode}]: tap on {name} changed output {k}"
            self.taps[name] = t.index_select(0, self.fr).cpu().numpy()
        return self.taps[name]

    def output(self, sp):
        if sp.out[0] == "tap":
            return self.tap(sp.name)
        parts = [self.ref_out[k].index_select(0, self.fr)[:, c0:c1] for k, c0, c1 in sp.out[1]]
        return torch.cat(parts, dim=1).cpu().numpy()

    def compare(self, sp, split, sd=None):
        """(worst err / bound, (frame, c, y, x) of it, every element finite) of layer sp over the compared frames."""
        inputs = [self.tap(s) for s, _ in sp.srcs]
        got = self.output(sp)
        worst, where, finite = 0.0, None, True
        for i, f in enumerate(self.case.frames):
            y, b = L.reference(sp, [t[i] for t in inputs], sd or self.sd, split)
            r, idx, fin = L.check(got[i], y, b)
            finite = finite and fin
            if r > worst or where is None:
                worst, where = r, (f,) + tuple(int(v) for v in idx)
        return worst, where, finite


def _conv_layers(run):
    """[(modelled layer, split arithmetic, kernels)] of every conv launch the profile lists; fails on one neither modelled
    nor excluded."""
    graph = L.layer_graph(run.cfg)
    todo = []
    for layer, kerns in sorted(run.ran.items()):
        conv = sorted(k for k in kerns if L.is_conv_family(k))
        if not conv or L.excluded(layer):
            continue
        names = L.merged_parts(run.cfg) if layer == "heads.first" else [layer]
        missing = [n for n in names if n not in graph]
        assert not missing, f"{run.case.id}: conv launch {layer} {conv} is neither compared nor in layer_ref.EXCLUDED"
        split = any(L.is_split_family(k) for k in conv)
        todo += [(n, split, conv) for n in names]
    return todo


@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
@pytest.mark.parametrize("case", L.CASES, ids=[c.id for c in L.CASES])
def test_every_conv_layer_against_float64(case, mode):
    run = _Run(case, mode)
    kernels = {k for ks in run.ran.values() for k in ks}
    forms = {L.variant_of(k) for k in kernels if k.startswith("conv3x3_f16x3")}
    todo = _conv_layers(run)
    graph = L.layer_graph(run.cfg)
    results = []
    for name, split, conv in todo:
        worst, where, finite = run.compare(graph[name], split)
        results.append((worst, name, "/".join(conv), where, finite))
    results.sort(key=lambda r: -r[0])
    print(f"\nLAYER_FP64 {case.id} [{mode}]: forms {sorted(forms)}; {len(results)} layers, worst {results[0][1]} "
          f"({results[0][2]}) err/bound = {results[0][0]:.3f} at (frame, c, y, x) = {results[0][3]}")
    for w, name, conv, where, finite in results:
        print(f"  {w:9.4f}  {name:24s} {conv}{'' if finite else '  NON-FINITE'}")
    if mode == "f16x3":
        assert forms == case.variants, (case.id, sorted(forms), {l: sorted(k) for l, k in run.ran.items()})
    else:
        assert not any(L.is_split_family(k) for k in kernels), sorted(kernels)
    # every modelled layer ran as a conv launch of its own or of the merged first layer; conv1a only inside conv1b's
    # launch (the stem fusion)
    missing = set(graph) - {n for n, _, _ in todo}
    assert missing <= {"backbone.conv1a"}, (case.id, sorted(missing))
    if missing:
        assert any("stem" in k for k in run.ran["backbone.conv1b"]), run.ran["backbone.conv1b"]
    bad = [(f"{n}: max err / bound = {w:.3g} at (frame, c, y, x) = {where}" + ("" if fin else ", non-finite"))
           for w, n, _, where, fin in results if not (w <= 1.0 and fin)]
    assert not bad, (case.id, mode, bad)


@pytest.mark.parametrize("case", [c for c in L.CASES if c.sweep], ids=[c.id for c in L.CASES if c.sweep])
def test_activation_magnitude_sweep_against_float64(case):
    """The producer's BatchNorm weight and bias times 2^k: its LeakyReLU output times 2^k, the consumer against the bound
    for k = -24 ... the largest k that keeps the activation below 2^16 (include/kp2d.h KP2D_PREC_F16X3)."""
    run = _Run(case, "f16x3")
    graph = L.layer_graph(run.cfg)
    base_sd = {k: np.array(v, copy=True) for k, v in run.sd.items()}
    split = {n: s for n, s, _ in _conv_layers(run)}
    try:
        for producer, consumer in case.sweep:
            amax = float(np.abs(run.tap(producer)).max())
            kmax = int(np.floor(np.log2(65504.0 / amax)))
            ks = sorted(set(list(range(-24, kmax + 1, 4)) + [kmax]))
            worst = {}
            for k in ks:
                sd = dict(base_sd)
                for key in (f"{producer}.bn.weight", f"{producer}.bn.bias"):
                    sd[key] = (base_sd[key] * np.float32(2.0 ** k)).astype(np.float32)
                run.model.load_state_dict({kk: torch.from_numpy(np.asarray(v)) for kk, v in sd.items()}, strict=True)
                run.ref_out = run._forward()
                run.taps = {}
                worst[k], where, finite = run.compare(graph[consumer], split[consumer], sd=sd)
                assert finite and worst[k] <= 1.0, (f"{case.id} {producer} x 2^{k} -> {consumer}: max err / bound = "
                                                     f"{worst[k]:.3g} at (frame, c, y, x) = {where}, finite: {finite}")
            print(f"\nSWEEP {case.id} {producer} -> {consumer}: max|act| 2^k from {amax * 2.0 ** -24:.2e} to "
                  f"{amax * 2.0 ** kmax:.4g}: " + ", ".join(f"{k}: {v:.3f}" for k, v in worst.items()))
    finally:
        run.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in base_sd.items()}, strict=True)
