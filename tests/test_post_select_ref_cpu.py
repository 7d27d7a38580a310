"""CPU side of the keypoint post-processing and selection tests (tables, references, bounds: post_select_ref.py; the device:
test_gpu_post_select_fp64.py).

1. csrc/select_form.h, compiled with g++ (no HIP), gives every case the form it is named for; the cases together select
   every value the header can return; KP2D_TOPK_SMALL = 8192 and 16384 never give a 256-thread form with more than 64 KB;
2. the restated post-processing IS oracle.kp2d_oracle.post_processing (float32 and float64, bit for bit), its float64
   sampling equals torch.nn.functional.grid_sample (bilinear and nearest, align_corners=True, zeros) to 1e-12, its class ids
   equal torch.argmax;
3. the input conditions of the regimes hold (``grid``: exact integers and halves in float32 and float64; ``z``: NaN cells and
   finite cells; ``clamp``: clamped cells at both ends; ``ties``: tied pixels);
4. the float32 emulation (the oracle in float32) meets every bound and equality on every case, the 2 % cap included;
5. every mutant of the emulation breaks a bound or an equality on at least one case; likewise the top-k mutants.
"""
import shutil
import subprocess

import numpy as np
import os
import pytest
import torch

import post_select_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "nano-vs-slam_amd", "csrc")
POST = list(R.POST_CASES)

# ---------------------------------------------------------------------------------------------------------------------
# select_form.h
# ---------------------------------------------------------------------------------------------------------------------
# argv: groups "t n k small", "g B C n k lds", "a HW seg_mis ids_mis postB segB postC" -> one line each; then the sweeps
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include "select_form.h"
int main(int argc, char** argv) {
  using namespace kp2d;
  char name[128];
  int i = 1;
  while (i < argc) {
    const char kind = argv[i][0];
    auto arg = [&](int j) { return atoi(argv[i + j]); };
    if (kind == 't') {
      TopkForm f;
      const int rc = choose_topk(arg(1), arg(2), arg(3), f);
      topk_form_name(f, name, sizeof name);
      std::printf("%d|%s|%zu\n", rc, rc ? "" : name, f.lds);
      i += 4;
    } else if (kind == 'g') {
      GatherForm f;
      const int rc = choose_gather(arg(1), arg(2), arg(3), arg(4), arg(5) != 0, f);
      gather_form_name(f, name, sizeof name);
      std::printf("%d|%s|%zu\n", rc, rc ? "" : name, f.lds);
      i += 6;
    } else {
      argmax_form_name(choose_post_seg(arg(1), (unsigned)arg(2), (unsigned)arg(3), arg(4), arg(5), arg(6)), name, sizeof name);
      std::printf("0|%s|0\n", name);
      i += 7;
    }
  }
  // everything the header can return, with kpow struck from the top-k names
  std::set<std::string> topk, gather, argmax;
  size_t small_lds[2] = {0, 0};
  const int smalls[] = {-1, 0, 64, 256, 4096, 8192, 16384, 1 << 30};
  for (int n = 1; n <= 40000; n = n < 64 ? n + 1 : n + n / 3)
    for (int k = 1; k <= 40000; k = k < 64 ? k + 1 : k + k / 3)
      for (int small : smalls) {
        TopkForm f;
        if (choose_topk(n, k, small, f)) continue;
        if (f.kernel == TOPK_256 && small >= 8192) small_lds[small > 8192] = f.lds > small_lds[small > 8192] ? f.lds : small_lds[small > 8192];
        if (f.kernel == TOPK_256 && f.lds > LDS_PLAIN_MAX) { std::printf("bad 256-thread form with %zu bytes\n", f.lds); return 1; }
        if (f.lds > 160 * 1024) { std::printf("bad lds %zu\n", f.lds); return 1; }
        topk_form_name(f, name, sizeof name);
        std::string s(name);
        const size_t a = s.find("kpow="), b = a == std::string::npos ? a : s.find(',', a);
        if (a != std::string::npos) s.erase(a, b - a + 1);
        topk.insert(s);
      }
  for (int B = 1; B <= 64; B += 7)
    for (int C = 2; C <= 128; C += 2)
      for (int n : {1, 2, 3, 4, 7, 8, 48, 117, 1200, 2047, 2048, 2049, 2052, 4800, 5119, 5120, 5121, 5124, 8191, 8192, 8193, 9000})
        for (int k = 1; k <= n; k = k < 8 ? k + 1 : k * 2)
          for (int lds = 0; lds < 2; ++lds) {
            GatherForm f;
            if (choose_gather(B, C, n, k, lds != 0, f)) continue;
            if (f.lds > 80 * 1024 || (f.lds > LDS_PLAIN_MAX && !f.lds_opt_in)) { std::printf("bad gather lds %zu\n", f.lds); return 1; }
            gather_form_name(f, name, sizeof name);
            gather.insert(name);
          }
  for (int HW = 1; HW <= 9; ++HW)
    for (unsigned sm = 0; sm < 16; sm += 4)
      for (unsigned im = 0; im < 16; im += 8)
        for (int sb = 1; sb <= 2; ++sb)
          for (int C : {32, 48, 64, 128}) {
            argmax_form_name(choose_post_seg(HW, sm, im, 1, sb, C), name, sizeof name);
            argmax.insert(name);
          }
  for (const auto& s : topk) std::printf("topk %s\n", s.c_str());
  for (const auto& s : gather) std::printf("gather %s\n", s.c_str());
  for (const auto& s : argmax) std::printf("argmax %s\n", s.c_str());
  std::printf("small8192 %zu\nsmall16384 %zu\n", small_lds[0], small_lds[1]);
  GatherForm g;
  TopkForm t;
  std::printf("refused %d %d %d\n", choose_gather(4, 1, 100, 10, true, g), choose_topk(0, 4, 256, t), choose_topk(16, 0, 256, t));
  return 0;
}
"""


@pytest.fixture(scope="module")
def form_driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    d = tmp_path_factory.mktemp("select_form")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    # no ROCm include path: select_form.h must stay free of HIP
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "driver.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _ask(driver, rows):
    argv = [str(v) for r in rows for v in r]
    out = subprocess.run([driver] + argv, check=True, capture_output=True, text=True).stdout.splitlines()
    return [l.split("|") for l in out[:len(rows)]], out[len(rows):]


def _strike_kpow(name):
    return ",".join(p for p in name.split(",") if not p.startswith("kpow="))


def test_every_case_gets_the_form_it_is_named_for(form_driver):
    rows, want = [], []
    for shape, (n, k, form) in R.TOPK_SHAPES.items():
        rows.append(("t", n, k, 256))
        want.append((shape, form))
    for shape, (n, k, forms) in R.TOPK_KNOB_SHAPES.items():
        for small, form in forms.items():
            rows.append(("t", n, k, small))
            want.append((f"{shape} at {small}", form))
    for case, g in R.GATHER_CASES.items():
        rows.append(("g", g["B"], g["C"], g["n"], g["k"], 1))
        want.append((case, g["form"]))
        rows.append(("g", g["B"], g["C"], g["n"], g["k"], 0))
        want.append((case + " at KP2D_GATHER_LDS=0", R.D_))
    for case, c in R.POST_CASES.items():
        d = R.post_dims(case)
        rows.append(("a", d["Hs"] * d["Ws"], 4 * c["seg_off"], 0, d["B"], d["B"], d["C"]))
        want.append((case, f"argmax<{c['argmax']}>"))
    got, _ = _ask(form_driver, rows)
    wrong = [(c, w, g) for (c, w), g in zip(want, got) if g[0] != "0" or g[1] != w]
    assert not wrong, wrong


def test_the_cases_select_every_value_the_header_can_return(form_driver):
    _, rest = _ask(form_driver, [])
    can = {kind: {l.split(" ", 1)[1] for l in rest if l.startswith(kind + " ")} for kind in ("topk", "gather", "argmax")}
    topk = {_strike_kpow(f) for _, _, f in R.TOPK_SHAPES.values()} | {_strike_kpow(f) for _, _, fs in R.TOPK_KNOB_SHAPES.values() for f in fs.values()}
    assert topk == can["topk"], (sorted(topk), sorted(can["topk"]))
    assert {g["form"] for g in R.GATHER_CASES.values()} == can["gather"], sorted(can["gather"])
    # "two,quad" is launch_post_seg's answer to a descriptor width post_kernel has no instance for or to two batch sizes, both
    # of which kp2d_post refuses or cannot express: no case can name it
    assert {f"argmax<{c['argmax']}>" for c in R.POST_CASES.values()} == can["argmax"] - {"argmax<two,quad>"}, sorted(can["argmax"])
    kpows = {int(p[5:]) for _, _, f in R.TOPK_SHAPES.values() for p in f.strip(">").split(",") if p.startswith("kpow=")}
    assert {128, 256, 512, 4096, 8192, 16384} <= kpows


def test_topk_small_is_bounded(form_driver):
    """KP2D_TOPK_SMALL above 4096 used to launch topk_kernel<256> with more than 64 KB of dynamic LDS and no opt-in (refused by
    the runtime); the header honours it up to 4096.  Values that worked keep their form."""
    rows = [("t", 19200, 8192, 8192), ("t", 19200, 8192, 16384), ("t", 19200, 16384, 16384), ("t", 19200, 4096, 8192),
            ("t", 19200, 4097, 8192), ("t", 19200, 4096, 4096), ("t", 300, 7, 0), ("t", 300, 7, -5), ("t", 4800, 1000, 1000),
            ("t", 4800, 1001, 1000)]
    got, rest = _ask(form_driver, rows)
    assert [g[1] for g in got] == [
        "topk<1024,kpow=8192,uncached,loop,optin>", "topk<1024,kpow=8192,uncached,loop,optin>",
        "topk<1024,kpow=16384,uncached,loop,optin>", "topk<256,kpow=4096,uncached,loop>", "topk<1024,kpow=8192,uncached,loop,optin>",
        "topk<256,kpow=4096,uncached,loop>", "topk<1024,kpow=8,cached,reg>", "topk<1024,kpow=8,cached,reg>",
        "topk<256,kpow=1024,uncached,loop>", "topk<1024,kpow=1024,cached,reg>"], got
    assert all(int(g[2]) <= 65536 for g in got if g[1].startswith("topk<256"))
    fig = dict(l.split() for l in rest if l.startswith("small"))
    assert 0 < int(fig["small8192"]) <= 65536 and 0 < int(fig["small16384"]) <= 65536, fig
    assert [l for l in rest if l.startswith("refused")] == ["refused -1310 -1300 -1300"]


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@pytest.mark.parametrize("case", POST)
def test_the_restated_post_processing_is_the_oracle(case):
    for dt in (np.float32, np.float64):
        mine = R.emulate(case, dt)
        dense, samp = R.oracle_post(case, dt, False), R.oracle_post(case, dt, True)
        assert _same(mine["score"], dense["score"]) and _same(mine["coord"], dense["coord"]) and _same(mine["desc"], dense["feat"])
        assert _same(mine["ids_dense"], dense["seg"]) and _same(mine["ids_samp"], samp["seg"])


@pytest.mark.parametrize("case", POST)
def test_float64_reference_against_torch(case):
    d, inp = R.post_dims(case), R.post_inputs(case)
    ref = R.emulate(case, np.float64)
    coord = torch.from_numpy(ref["coord"])
    gx = coord[:, 0] / ((d["W"] - 1) / 2.0) - 1.0
    gy = coord[:, 1] / ((d["H"] - 1) / 2.0) - 1.0
    grid = torch.stack([gx, gy], -1)
    f = torch.nn.functional.grid_sample(torch.from_numpy(inp["feat"]).double(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    want = (f / f.norm(dim=1, keepdim=True)).numpy()
    assert np.array_equal(np.isnan(want), np.isnan(ref["desc"]))
    assert np.nanmax(np.abs(want - ref["desc"]), initial=0.0) <= 1e-12
    seg = torch.from_numpy(inp["seg"])
    assert np.array_equal(torch.argmax(seg, dim=1, keepdim=True).numpy(), ref["ids_dense"]) or R.POST_CASES[case]["seg_regime"] == "ties"
    if R.POST_CASES[case]["seg_regime"] == "ties":      # torch.argmax names no tie rule: the value it picks is the maximum
        pick = torch.gather(seg, 1, torch.from_numpy(ref["ids_dense"]))
        assert torch.equal(pick, seg.max(dim=1, keepdim=True).values)
    near = torch.nn.functional.grid_sample(seg.double(), grid, mode="nearest", padding_mode="zeros", align_corners=True)
    assert np.array_equal(torch.argmax(near, dim=1, keepdim=True).numpy(), ref["ids_samp"])


def test_input_conditions_of_the_regimes():
    for case, c in R.POST_CASES.items():
        d, inp = R.post_dims(case), R.post_inputs(case)
        if c["regime"] == "grid":
            for dt in (np.float32, np.float64):
                e = R.emulate(case, dt)
                assert np.array_equal(e["coord"].astype(np.float64), R.emulate(case, np.float64)["coord"])
                for a, (size, full) in enumerate(((d["Wf"], d["W"]), (d["Hf"], d["H"]), (d["Ws"], d["W"]), (d["Hs"], d["H"]))):
                    i = R._sample_coords(e["coord"][:, a % 2], size, full, np.dtype(dt), None).astype(np.float64)
                    assert np.all((i * 2) == np.rint(i * 2)), (case, dt)
                    assert np.array_equal(i, e["coord"][:, a % 2].astype(np.float64) * (size - 1) / (full - 1))
                    halves = i[(i * 2) % 2 == 1]
                    assert halves.size > 20
                    if case == "S-grid97" and a >= 2:
                        assert np.all(np.floor(halves) % 2 == 0)          # halves on even k: half-up and half-even differ
            x = R.emulate(case, np.float64)["coord"][:, 0]
            assert set(np.unique(x - 4 * np.arange(d["Wc"])[None, None, :])) == {0.0, 3.0}
        if c["regime"] == "z":
            nan = np.isnan(R.post_bounds(case)["desc"])
            assert nan.all(axis=1).sum() >= 4 and (~nan).all(axis=1).sum() >= 4 and np.array_equal(nan.any(axis=1), nan.all(axis=1))
        if c["regime"] == "clamp":
            co = R.emulate(case, np.float64)["coord"]
            assert (co[:, 0] == 0).sum() >= 2 and (co[:, 0] == d["W"] - 1).sum() >= 2 and (co[:, 1] == 0).sum() >= 2 and (co[:, 1] == d["H"] - 1).sum() >= 2
        if c["seg_regime"] == "ties":
            seg = inp["seg"]
            tied = (seg == seg.max(axis=1, keepdims=True)).sum(axis=1) >= 2
            assert 0.2 <= tied.mean() <= 0.5, (case, tied.mean())
            assert (np.signbit(np.take_along_axis(seg, seg.argmax(axis=1)[:, None], 1)) & (seg.max(axis=1, keepdims=True) == 0)).sum() >= 1
    assert R.post_dims("S-3x5-clamp-h")["H"] == 4 * 3 - 3
    for name, (cfg, cell, C) in R.MODELS.items():
        assert 2 ** R.orc.get_config(cfg)["downsample"] == cell and R.orc.get_config(cfg)["nfeatures"] == C


@pytest.mark.parametrize("case", POST)
def test_float32_emulation_meets_every_bound(case):
    line, bad = R.evaluate_post(case, R.emulate(case, np.float32))
    print("\n" + line)
    assert not bad, (case, bad)


@pytest.mark.parametrize("mut", R.POST_MUTANTS)
def test_every_post_mutant_is_caught(mut):
    caught = [case for case in POST if R.evaluate_post(case, R.emulate(case, np.float32, mut))[1]]
    print(f"\n{mut}: caught on {len(caught)} of {len(POST)} cases: {caught[:6]}")
    assert caught, mut
    if mut == "eps":
        assert all(R.POST_CASES[c]["regime"] == "z" for c in caught)
    if mut == "half_up":
        assert "S-grid97" in caught
    if mut == "last_max":
        assert all(R.POST_CASES[c]["seg_regime"] == "ties" for c in caught)


def test_float64_reference_is_far_inside_the_bounds():
    """the bounds are about float32: the float64 restatement sits at 1e-8 of them or below"""
    for case in POST:
        bd = R.post_bounds(case)
        ok = ~np.isnan(bd["desc"])
        assert R._ratio(np.abs(R.emulate(case, np.float64)["desc"] - bd["ref"]["desc"])[ok], bd["desc"][ok]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# top-k and gather
# ---------------------------------------------------------------------------------------------------------------------
def _emulated_topk(shape, regime, thr, mut=None):
    n, k = R.topk_shape(shape)
    s = R.topk_scores(shape, regime, thr)
    kk = min(k, n)
    idx, val, cnt = np.full((3, kk), -1, np.int32), np.zeros((3, kk), np.float32), np.zeros(3, np.int32)
    for b in range(3):
        order = R.topk_reference(s[b], k, thr, mut)
        idx[b, :len(order)], val[b, :len(order)], cnt[b] = order, s[b][order], len(order)
    return {"idx": idx, "val": val, "cnt": cnt}


SMALL_TOPK = [c for c in R.topk_cases() if R.topk_shape(c[0])[0] <= 2049]


@pytest.mark.parametrize("shape,regime,thr", SMALL_TOPK, ids=[R.topk_id(*c) for c in SMALL_TOPK])
def test_topk_reference_against_torch(shape, regime, thr):
    """torch.topk on the CPU returns the reference's VALUES; its order among equal values is unspecified, the reference's is
    index ascending with -0.0 == +0.0"""
    n, k = R.topk_shape(shape)
    s = R.topk_scores(shape, regime, thr)
    line, bad = R.evaluate_topk(shape, regime, thr, _emulated_topk(shape, regime, thr))
    assert not bad, bad
    for b in (0, 2):
        order = R.topk_reference(s[b], k, thr)
        keep = torch.from_numpy(s[b])
        keep = keep[(keep > thr)]
        want = torch.topk(keep, min(len(order), len(keep))).values.numpy()
        assert len(order) == min(k, n, len(keep)) and np.array_equal(s[b][order] + 0.0, want + 0.0)
        same = s[b][order][1:] == s[b][order][:-1]
        assert np.all(np.diff(order)[same] > 0)


@pytest.mark.parametrize("mut", R.TOPK_MUTANTS)
def test_every_topk_mutant_is_caught(mut):
    caught = [R.topk_id(*c) for c in SMALL_TOPK if R.evaluate_topk(*c, _emulated_topk(*c, mut))[1]]
    print(f"\n{mut}: caught on {len(caught)} of {len(SMALL_TOPK)} cases: {caught[:6]}")
    assert caught, mut
    if mut == "zero_order":
        assert any("-zeros-" in c for c in caught)
    if mut == "nan_selected":
        assert all("-special-" in c for c in caught)


def test_topk_regimes_hold_what_they_promise():
    for shape in R.TOPK_SHAPES:
        z = R.topk_scores(shape, "zeros", -R.INF)
        assert (np.signbit(z) & (z == 0)).sum() > 50 and (~np.signbit(z) & (z == 0)).sum() > 50
        sp = R.topk_scores(shape, "special", -R.INF)[0]
        assert np.isnan(sp).any() and np.isposinf(sp).any() and np.isneginf(sp).any() and ((np.abs(sp) < 1e-38) & (sp != 0)).any()
        assert len(np.unique(R.topk_scores(shape, "equal", 0.0)[0])) == 1
        assert (R.topk_scores(shape, "signed", -0.5)[0] < 0).any()


def test_gather_inputs_hold_what_they_promise():
    ks = set()
    for case, c in R.GATHER_CASES.items():
        if c["n"] > 2100:
            continue
        idx = R.gather_inputs(case)["idx"]
        ks.add(c["k"])
        assert idx.shape == (c["B"], c["k"]) and idx.min() >= -1 and idx.max() < c["n"]
        if c["k"] >= 3:
            assert (idx[1::2, 1:-1] == -1).any() and any(len(np.unique(r[r >= 0])) < (r >= 0).sum() for r in idx[1::2])
    assert {1, 2, 3, 7} <= ks
    emu = R.gather_inputs("g-lds8-117-k15")
    bi = np.arange(32)[:, None]
    safe = np.maximum(emu["idx"], 0)
    rec = {"dsel": np.where((emu["idx"] >= 0)[..., None], emu["desc"].transpose(0, 2, 1)[bi, safe], np.float32(0)),
           "pts": np.where((emu["idx"] >= 0)[..., None], emu["coord"].transpose(0, 2, 1)[bi, safe], np.float32(0))}
    assert not R.evaluate_gather("g-lds8-117-k15", rec)[1]
    rec["dsel"] = rec["dsel"].copy()
    rec["dsel"][emu["idx"] < 0] = 1.0
    assert R.evaluate_gather("g-lds8-117-k15", rec)[1]
