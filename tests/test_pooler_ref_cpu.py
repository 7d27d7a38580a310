"""CPU side of the descriptor-pooler stage tests (table, references, bound: pooler_fp64_ref.py; the device:
test_gpu_pooler_fp64.py).  The inputs here are the oracle's own convlad3 maps of the cases' seeded frames.

1. the float64 references agree: the oracle's literal and restated NetVLAD, this suite's staged restatement (the one the
   perturbations and mutations go through) and vlad_training_ref.forward, to 1e-12; regime z against its closed form;
2. the stored E32 (per regime) and Esplit (per split case) regenerate;
3. the input conditions of regime s hold;
4. the bound has teeth: each mutation of the float64 reference that applies to a case's layout gives E >= 10 x its bound;
5. csrc/netvlad_form.h, compiled with g++ (no HIP), gives every case the form it is named for, and the cases together
   select every kernel instantiation and every vlad_ordered_sum branch the header can return.
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import pooler_fp64_ref as R
import vlad_training_ref as T
from conftest import ROOT
from oracle import kp2d_oracle as orc

CSRC = os.path.join(ROOT, "nano-vs-slam_amd", "csrc")
NETVLAD = R.cases(kind="netvlad") + [c for f in R.FORMS for c in R.cases(kind="netvlad", form=f)]
ALL = list(R.CASES)


@functools.lru_cache(maxsize=None)
def figures():
    return R.cpu_figures()


@pytest.mark.parametrize("case", NETVLAD)
def test_float64_references_agree(case):
    x, p = R.cpu_input(case)
    x64 = np.asarray(x, np.float64)
    q = R._np_params(p, np.float64)
    literal = R.reference(case, x, p)
    restated = orc.netvlad(x64, q, literal=False)
    staged = R.vlad64(x, p)
    train = T.forward(x64.reshape(x.shape[0], x.shape[1], -1), p["W"], p["cent"])["vlad"]
    for name, v in (("restated", restated), ("staged", staged), ("vlad_training_ref", train)):
        d = float(np.abs(np.asarray(v).reshape(literal.shape) - literal).max())
        print(f"{case}: literal vs {name}: {d:.2e}")
        assert d <= 1e-12, (case, name, d)
    if R.is_zero(case):
        assert np.all(x == 0)
        K = p["W"].shape[0]
        cent = np.asarray(p["cent"], np.float64)
        closed = (-cent / np.linalg.norm(cent, axis=1, keepdims=True) / np.sqrt(K)).reshape(-1)
        assert np.abs(literal - closed[None]).max() <= 1e-12


def test_stored_e32_regenerates():
    got = R.regime_e32(figures())
    print({k: f"{v:.4g}" for k, v in got.items()})
    assert set(got) == set(R.E32)
    for k, v in R.E32.items():
        assert abs(got[k] / v - 1.0) <= R.E32_RTOL, (k, got[k], v)


def test_stored_esplit_regenerates():
    fig = figures()
    split = {c for c in ALL if R.is_split(c, "f16x3")}
    assert split == set(R.ESPLIT_CPU)
    for c in sorted(split):
        assert abs(fig[c][1] - R.ESPLIT_CPU[c]) <= 0.02 * R.ESPLIT_CPU[c], (c, fig[c][1], R.ESPLIT_CPU[c])     # (regime z: 0)


@pytest.mark.parametrize("case", [c for c in NETVLAD if R.CASES[c]["regime"] == "s"])
def test_input_conditions_of_the_sharp_regime(case):
    x, p = R.cpu_input(case)
    cond = R.conditions(x, p["W"])
    print(f"{case}: top assignment >= 0.9 on {cond[0]:.2f} of the pixels; rarest cluster per frame (rowsum / (S / K)): {cond[1]}; planted {p['planted']}")
    assert R.conditions_hold(cond), cond


@pytest.mark.parametrize("case", NETVLAD)
def test_the_bound_has_teeth(case):
    """padding: one padding pixel of a ragged tile counted; rowsum: the rowsum * centroid term dropped for one cluster;
    fp16: the assignment rounded to fp16 before the aggregation; slab: one slab's partial skipped."""
    x, p = R.cpu_input(case)
    base = R.vlad64(x, p)
    b = max(R.bound(case, mode, x, p)[0] for mode in R.MODES)      # (the wider of the two modes' bounds)
    bad = []
    for mut in R.mutations(case):
        E = R.err(R.vlad64(x, p, mutate=mut, px=R.vlad_px(case)), base)
        print(f"{case}: {mut:8s} E = {E:.3e} = {E / b:.1f} x the bound {b:.3e}")
        if not E >= R.TEETH * b:
            bad.append((mut, E, b))
    assert not bad, (case, bad)


def test_the_cases_cover_every_mutation():
    seen = {m for c in NETVLAD for m in R.mutations(c)}
    assert seen == {"padding", "rowsum", "fp16", "slab"}


# ---------------------------------------------------------------------------------------------------------------------
# netvlad_form.h
# ---------------------------------------------------------------------------------------------------------------------
# argv: groups "K C prec split S B px" -> "rc|name"; then "all": every (kernel, inst, split) and sum branch the header returns
# over a sweep of shapes, modes and tile counts
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include "netvlad_form.h"
int main(int argc, char** argv) {
  using namespace kp2d;
  int i = 1;
  for (; i + 6 < argc; i += 7) {
    const int K = atoi(argv[i]), C = atoi(argv[i + 1]), prec = atoi(argv[i + 2]), split = atoi(argv[i + 3]);
    const int S = atoi(argv[i + 4]), B = atoi(argv[i + 5]), px = atoi(argv[i + 6]);
    VladForm f;
    const int rc = choose_netvlad(K, C, prec, split != 0, f);
    char name[128] = "";
    if (rc == 0) netvlad_form_name(f, netvlad_nsplit(S, px), netvlad_tiles_per_slab(S, B, px), name, sizeof name);
    std::printf("%d|%s\n", rc, name);
  }
  std::set<std::string> inst, sums;
  int refused = 0;
  for (int K = 0; K <= 72; ++K)
    for (int C = 4; C <= 260; C += 2)
      for (int prec = 0; prec < 2; ++prec)
        for (int split = 0; split < 2; ++split) {
          VladForm f;
          if (choose_netvlad(K, C, prec, split != 0, f)) { ++refused; continue; }
          char b[64];
          std::snprintf(b, sizeof b, "%s%d,%s", f.kernel == VLAD_MFMA ? "mfma" : "generic", f.inst, f.split ? "split" : "exact");
          inst.insert(b);
        }
  static const char* const kSum[] = {"direct", "unrolled", "loop"};
  for (int tps = 0; tps <= 40; ++tps) sums.insert(kSum[netvlad_sum_branch(tps)]);
  for (const auto& s : inst) std::printf("inst %s\n", s.c_str());
  for (const auto& s : sums) std::printf("sum %s\n", s.c_str());
  std::printf("refused %d\n", refused);
  return 0;
}
"""


@pytest.fixture(scope="module")
def form_driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    d = tmp_path_factory.mktemp("netvlad_form")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    # no ROCm include path: netvlad_form.h must stay free of HIP
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "driver.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _ask(driver, rows):
    argv = [str(v) for r in rows for v in r]
    out = subprocess.run([driver] + argv, check=True, capture_output=True, text=True).stdout.splitlines()
    return out[:len(rows)], out[len(rows):]


def test_every_case_gets_the_form_it_is_named_for(form_driver):
    rows, want = [], []
    for case in NETVLAD:
        c, m = R.CASES[case], R.MODELS[R.CASES[case]["model"]]
        for mode in R.MODES:
            rows.append((m["K"], m["C"], int(mode == "f16x3"), 1, c["S"], c["B"], R.vlad_px(case)))
            want.append((case, mode, "0|" + R.form_string(case, mode)))
            if "alone" in c:
                rows.append((m["K"], m["C"], int(mode == "f16x3"), 1, c["S"], c["nref"], R.vlad_px(case)))
                want.append((case, mode + " alone", "0|" + R.form_string(case, mode, c["alone"])))
    got, _ = _ask(form_driver, rows)
    wrong = [(c, m, w, g) for (c, m, w), g in zip(want, got) if w != g]
    assert not wrong, wrong


def test_the_cases_select_every_instantiation_and_sum_branch(form_driver):
    _, rest = _ask(form_driver, [])
    can = {l.split(" ", 1)[1] for l in rest if l.startswith("inst ")}
    sums = {l.split(" ", 1)[1] for l in rest if l.startswith("sum ")}
    assert can == {"mfma1,split", "mfma1,exact", "mfma2,split", "mfma2,exact", "generic16,exact", "generic32,exact"}, can
    assert sums == {"direct", "unrolled", "loop"}
    picked = {(R.KERNEL[R.CASES[c]["model"]], "split" if R.is_split(c, mode) else "exact") for c in NETVLAD for mode in R.MODES}
    assert {f"{k},{s}" for k, s in picked} == can
    assert {R.CASES[c]["sum"] for c in NETVLAD} | {R.CASES[c]["alone"][2] for c in NETVLAD if "alone" in R.CASES[c]} == sums


def test_split_switch_and_refusals(form_driver):
    """KP2D_VLAD_SPLIT=0 in the f16x3 mode: the instantiation of the fp32 mode.  Shapes launch_netvlad refused before the
    header existed are refused with the same code."""
    rows = [(64, 64, 1, 0, 324, 2, 320), (64, 64, 0, 1, 324, 2, 320), (32, 48, 1, 0, 132, 2, 320),
            (68, 64, 1, 1, 324, 2, 320), (2, 64, 1, 1, 324, 2, 320), (30, 64, 1, 1, 324, 2, 320), (64, 62, 1, 1, 324, 2, 320),
            (64, 132, 1, 1, 324, 2, 320)]
    got, _ = _ask(form_driver, rows)
    assert got[0] == got[1] == "0|netvlad<mfma2,exact,tile ns=2 tps=3 sum=unrolled>"
    assert got[2] == "0|netvlad<mfma1,exact,tile ns=1 tps=3 sum=unrolled>"
    assert got[3:] == ["-1100|"] * 5
