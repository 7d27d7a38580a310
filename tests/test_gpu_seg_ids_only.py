"""KP2D_FWD_NO_SEG_LOGITS: the streaming entry points' last segmentation layer as conv3x3_s16.hip's ids-only form ("<s16>ids":
transposed products, the argmax over the class logits found in registers, one int64 per pixel stored and no logits).

The form needs the all-split plan of big grids, forced here at small batches as tests/test_gpu_parity.py does (s16_min_items,
ws_min_tiles, wsm_min_items = 1, one stream lane).  Shapes: 3 frames of 104 x 272 — a 52 x 136 class map, ragged in both tile
directions (3.25 x 16 rows, 4.25 x 32 columns), 60 work items on 56 workgroups (n_my = 1 | 2) — and one frame of 240 x 320
(120 x 160: a half-empty last tile row, 40 items).  Every comparison is bit for bit: the form computes the logits the other
forms store (same products, same order, same fused multiply-add) and compares them in torch.argmax's order."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_inputs, load_golden, product_model
from oracle.weights import synthetic_frames

DEV = "cuda:0"
LAST = "seg_head.convs.8"


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the constant and the switch
# ---------------------------------------------------------------------------------------------------------------------
def test_flag_constant_equals_the_headers():
    from nano_vs_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "kp2d.h"), encoding="utf-8").read()
    flags = {n: int(v) for n, v in re.findall(r"#define (KP2D_FWD_\w+) (\d+)u", hdr)}
    assert flags == {"KP2D_FWD_EVAL": 1, "KP2D_FWD_ONLY_ENCODER": 2, "KP2D_FWD_NO_SEG_LOGITS": 4}
    for name, value in flags.items():
        assert getattr(_lib, name) == value, name


def test_switch_is_a_launcher_knob_read_in_the_one_place_and_documented():
    """KP2D_SEG_IDS_ONLY=0 is the way back.  It lives with the process-wide launcher knobs (options.h Tuning), not in
    kOptions: tests/test_options.py pins that table's rows."""
    csrc = os.path.join(ROOT, "nano-vs-slam_amd", "csrc")
    assert "bool seg_ids_only;" in open(os.path.join(csrc, "options.h"), encoding="utf-8").read()
    assert 't.seg_ids_only = on("KP2D_SEG_IDS_ONLY");' in open(os.path.join(csrc, "options.cpp"), encoding="utf-8").read()
    assert "tuning().seg_ids_only" in open(os.path.join(csrc, "plan.cpp"), encoding="utf-8").read()
    rows = [ln for ln in open(os.path.join(ROOT, "README.md"), encoding="utf-8") if ln.startswith("| `KP2D_SEG_IDS_ONLY")]
    assert len(rows) == 1


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _force(model, x):
    with torch.no_grad():
        model(x[:1])                                     # (creates the engine)
    eng = model._engine
    for key, value in ((b"s16_min_items", 1), (b"ws_min_tiles", 1), (b"wsm_min_items", 1), (b"lanes", 1)):
        assert eng.lib.kp2d_set_option(eng.handle, key, value) == 0


def _ran(model, fn):
    """{layer: kernel family + tile form} of the forward fn() runs, read back through kp2d_profile_get."""
    import ctypes as C
    eng = model._engine
    lib = eng.lib
    lib.kp2d_set_profiling(eng.handle, 1)
    with torch.no_grad():
        fn()
    torch.cuda.synchronize()
    out = {}
    layer, kern = C.c_char_p(), C.c_char_p()
    ms, fl, by = C.c_float(), C.c_double(), C.c_double()
    for i in range(lib.kp2d_profile_count(eng.handle)):
        lib.kp2d_profile_get(eng.handle, i, C.byref(layer), C.byref(kern), C.byref(ms), C.byref(fl), C.byref(by))
        out.setdefault(layer.value.decode(), set()).add(kern.value.decode())
    lib.kp2d_set_profiling(eng.handle, 0)
    return out


def _ids_form(ran):
    return any("<s16>ids" in k for k in ran[LAST])


def _assert_form(model, x, want=True):
    """The precondition of every case: with the flag the last segmentation layer ran the ids-only form (want) or did not;
    without the flag it never does."""
    assert not _ids_form(_ran(model, lambda: model(x))), "plain forward"
    ran = _ran(model, lambda: model._forward_input(x, drop_logits=True))
    assert _ids_form(ran) == want, ran[LAST]


def _plain(model, x, top_k=300):
    """post_processing(net(x)) + select_and_gather, and the plain forward's logits."""
    from nano_vs_slam_amd.selectors import select_and_gather
    H, W = x.shape[-2:]
    with torch.no_grad():
        logits = model(x)["seg"].clone()
        out = model.post_processing(model(x), H, W)
        _i, _v, cnt, pts, desc = select_and_gather(out["score"], out["coord"], out["feat"], top_k, 0.7)
    return logits, {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}, pts.clone(), desc.clone(), cnt.clone()


def _dropped(model, x, top_k=300):
    """The same through _forward(drop_logits=True) + post_processing."""
    from nano_vs_slam_amd.selectors import select_and_gather
    H, W = x.shape[-2:]
    with torch.no_grad():
        out = model.post_processing(model._forward_input(x, drop_logits=True), H, W)
        _i, _v, cnt, pts, desc = select_and_gather(out["score"], out["coord"], out["feat"], top_k, 0.7)
    return {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}, pts.clone(), desc.clone(), cnt.clone()


def _assert_same(want, got, label):
    (wo, wp, wd, wc), (go, gp, gd, gc) = want, got
    assert set(wo) == set(go), label
    for k in wo:
        assert wo[k].dtype == go[k].dtype and torch.equal(wo[k], go[k]), (label, k)
    assert torch.equal(wc, gc) and torch.equal(wp, gp) and torch.equal(wd, gd), label


@pytest.fixture(scope="module")
def net():
    model, sd = product_model("S", False, 28)
    _force(model, torch.from_numpy(synthetic_frames(1, 104, 272, seed=3)).to(DEV))
    return model, sd


def _frames(kind, B, H, W):
    if kind == "golden":
        meta, _ = load_golden("v2_S_240x320")
        assert (meta["config"], meta["v3"], meta["n_classes"], meta["weight_seed"], meta["H"], meta["W"]) == ("S", False, 28, 1234, H, W)
        return torch.from_numpy(np.ascontiguousarray(golden_inputs(meta)[2][:B])).to(DEV)      # (the fixture's weights are net()'s)
    return torch.from_numpy(synthetic_frames(B, H, W, seed=91)).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B,H,W", [("seeded", 3, 104, 272), ("seeded", 1, 240, 320), ("golden", 1, 240, 320)])
def test_ids_only_form_equals_the_plain_path(net, kind, B, H, W):
    from nano_vs_slam_amd.pipeline import BatchStream
    model, _ = net
    x = _frames(kind, B, H, W)
    _assert_form(model, x)
    logits, *want = _plain(model, x)
    ids = logits.argmax(1, keepdim=True)                 # torch's argmax of the plain forward's logits, on the device
    assert torch.equal(want[0]["seg"], ids)
    got = _dropped(model, x)
    _assert_same(want, got, "_forward(drop_logits=True)")
    assert torch.equal(got[0]["seg"], ids) and int(got[0]["seg"].max()) < 28
    bs = BatchStream(model, slots=2, top_k=300, nn_thresh=0.7, device=DEV)
    try:
        res = [({k: v.clone() for k, v in o.items() if torch.is_tensor(v)}, p.clone(), d.clone(), c.clone()) for o, p, d, c in bs.map([x, x, x])]
    finally:
        bs.close()                                       # (gives the engine its default lane count back)
        assert model._engine.lib.kp2d_set_option(model._engine.handle, b"lanes", 1) == 0
    assert len(res) == 3
    for i, r in enumerate(res):
        _assert_same(want, r, f"BatchStream batch {i}")
    # a public forward afterwards still returns the logits
    with torch.no_grad():
        assert torch.equal(model(x)["seg"], logits)


@pytest.mark.gpu
def test_post_processing_refuses_a_dict_whose_logits_were_dropped_and_whose_ids_are_gone(net):
    model, _ = net
    x = _frames("seeded", 3, 104, 272)
    with torch.no_grad():
        out = model._forward_input(x, drop_logits=True)
        model(x)                                         # (another forward in between: the ids cache now belongs to it)
        with pytest.raises(RuntimeError, match="drop"):
            model.post_processing(out, 104, 272)


def _with_last_layer(sd, weight=None, bias=None):
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    if weight is not None:
        sd[LAST + ".weight"] = weight(sd[LAST + ".weight"]).astype(np.float32)
    sd[LAST + ".bias"] = np.asarray(bias, dtype=np.float32)
    return {k: torch.from_numpy(v) for k, v in sd.items()}


@pytest.fixture()
def net_edit(net):
    """net() with another last layer for one test; the seeded weights come back afterwards."""
    model, sd = net

    def load(weight=None, bias=None):
        model.load_state_dict(_with_last_layer(sd, weight, bias), strict=True)
        return model
    yield load
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)


@pytest.mark.gpu
def test_padding_channels_never_win(net_edit):
    """Rows 28 .. 31 of the 32-channel weight pack are zero: their "logit" is the shift, 0.  With a bias of -10 (and the
    weights halved: |w . x| stays below 8.1 on the reference fixture, the margin is for other frames) every real logit is
    negative, so a padding channel that took part would win every pixel."""
    model = net_edit(weight=lambda w: 0.5 * w, bias=np.full(28, -10.0))
    x = _frames("seeded", 3, 104, 272)
    _assert_form(model, x)
    logits, *want = _plain(model, x)
    assert bool((logits < 0).all()), float(logits.max())
    got = _dropped(model, x)
    _assert_same(want, got, "bias -10")
    assert int(got[0]["seg"].max()) < 28 and int(got[0]["seg"].min()) >= 0
    assert torch.equal(got[0]["seg"], logits.argmax(1, keepdim=True))


@pytest.mark.gpu
@pytest.mark.parametrize("high,first", [
    ((), 0),                     # equal bias everywhere
    ((5, 17, 22), 5),            # c = 16 n + 4 lg + r: (n 0, lg 1), (n 1, lg 0), (n 1, lg 1) — two lane groups, both N-tiles
    ((3, 9, 14, 26), 3),         # lane groups 0, 2, 3 and 2: across the half-wave exchange too
    ((27,), 27),                 # the last real channel, next to the padding rows
])
def test_ties_across_lanes_and_n_tiles_go_to_the_first_class(net_edit, high, first):
    bias = np.full(28, 0.25)
    bias[list(high)] = 1.5
    model = net_edit(weight=lambda w: 0.0 * w, bias=bias)
    x = _frames("seeded", 3, 104, 272)
    _assert_form(model, x)
    logits, *want = _plain(model, x)
    got = _dropped(model, x)
    _assert_same(want, got, f"ties {high}")
    assert bool((got[0]["seg"] == first).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fp32", "v3", "sample_segmentation", "120x160"])
def test_fallbacks_write_logits_and_ids_as_without_the_flag(case):
    v3 = case == "v3"
    model, _ = product_model("S", v3, 19 if v3 else 28)
    B, H, W = (1, 120, 160) if case == "120x160" else (3, 104, 272)
    x = torch.from_numpy(synthetic_frames(B, H, W, seed=92)).to(DEV)
    if case == "fp32":
        model.set_precision("fp32")
    if case == "sample_segmentation":
        model.sample_segmentation = True
    _force(model, x)
    _assert_form(model, x, want=False)
    logits, *want = _plain(model, x)
    with torch.no_grad():
        fwd = model._forward_input(x, drop_logits=True)
        assert torch.equal(fwd["seg"], logits) and bool(torch.isfinite(fwd["seg"]).all())
    _assert_same(want, _dropped(model, x), case)


CHILD = r"""
import sys
import numpy as np
import torch
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import test_gpu_seg_ids_only as t
model, _ = t.product_model("S", False, 28)
x = t._frames("seeded", 1, 240, 320)
t._force(model, x)
ran = t._ran(model, lambda: model._forward_input(x, drop_logits=True))
with torch.no_grad():
    plain = model(x)["seg"].clone()
    fwd = model._forward_input(x, drop_logits=True)
    seg = fwd["seg"].clone()
    ids = model.post_processing(fwd, 240, 320)["seg"]
np.savez(sys.argv[2], form=np.array(sorted(ran[t.LAST])), plain=plain.cpu().numpy(), seg=seg.cpu().numpy(), ids=ids.cpu().numpy())
"""


@pytest.mark.gpu
def test_switch_off_restores_the_logits_and_the_plain_forward_never_depended_on_it(net, tmp_path):
    """KP2D_SEG_IDS_ONLY=0 is read when the library first plans a forward, so it gets a process of its own: there the flag is
    ignored (the general kernel runs and writes logits and ids), and the plain forward's logits are this process's."""
    model, _ = net
    x = _frames("seeded", 1, 240, 320)
    _assert_form(model, x)
    with torch.no_grad():
        logits = model(x)["seg"].clone()
    assert bool(torch.isfinite(logits).all())
    out = tmp_path / "off.npz"
    env = dict(os.environ, KP2D_SEG_IDS_ONLY="0")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(out)], check=True, env=env, cwd=ROOT, timeout=300)
    z = np.load(out)
    assert not any("<s16>ids" in str(k) for k in z["form"]), z["form"]
    assert np.array_equal(z["plain"], logits.cpu().numpy())
    assert np.array_equal(z["seg"], logits.cpu().numpy())
    assert np.array_equal(z["ids"], logits.argmax(1, keepdim=True).cpu().numpy())
