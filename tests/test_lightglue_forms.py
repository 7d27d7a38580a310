"""CPU side of the LightGlue launch-form tests (GPU side: test_gpu_lightglue_forms.py; table, inputs and reference:
lightglue_fp64_ref.py).

1. csrc/attention_form.h and csrc/lightglue_form.h are plain C++.  They are compiled here with g++, together with options.cpp,
   and evaluated for every (case, form) pair of the table, each in a process whose environment is the one the GPU test gives
   the form's child: the knobs go through tuning_from_env as in the library.  The launcher cannot report which kernel ran, so
   this is what proves that the GPU runs exercise what they are named for: the table reaches every form the headers can
   return for prec = 1 (found by enumeration, not listed by hand), and each row runs the form it is named for.
2. The input conditions of the corresponding family (the comparison mask keeps >= 95 % of the rows, >= 15 % of all rows are
   kept and matched) hold for the float64 reference alone, and E32 is printed per case."""
import os
import shutil
import subprocess

import pytest

import lightglue_fp64_ref as R
from oracle import lightglue_oracle as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nano-vs-slam_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <tuple>
#include "attention_form.h"
#include "lightglue_form.h"
#include "options.h"
using namespace kp2d;
namespace kp2d { void set_last_error(const char*) {} }      // (options.cpp reports errors through the library's)
static const char* env(const char* n) { return getenv(n); }
int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "enumerate")) {
    // every (kernel, instance, affine) choose_attention returns for prec = 1 with head dims the split kernels take, and
    // every LgForm / tail instance: far wider than any test shape
    const int sizes[] = {1, 31, 32, 96, 127, 128, 129, 255, 256, 257, 1024, 4096, 70000};
    const long ks[] = {0, 256, 1L << 20, 1L << 40};
    std::set<std::tuple<int, int, int>> seen;
    for (int S : sizes) for (int T : sizes) for (int heads : {1, 2, 3, 4, 8, 16}) for (int hd : {4, 8, 12, 16})
      for (int B = 1; B <= 80; ++B) for (long k : ks) for (int q : {128, 256, 0}) for (int aff = 0; aff < 2; ++aff) {
        AttForm f;
        if (choose_attention(S, T, heads, B, heads * hd, 1, k, q, aff != 0, f)) { std::printf("error\n"); return 1; }
        seen.insert(std::make_tuple(f.kernel, f.inst, (int)f.affine));
      }
    for (auto& t : seen) std::printf("att %d %d %d\n", std::get<0>(t), std::get<1>(t), std::get<2>(t));
    std::set<std::tuple<int, int, int>> lgs;
    for (int D : {32, 64}) for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) for (int nw : {0, 1, 4}) {
      const LgForm f = choose_lg_form(D, a != 0, b != 0);
      lgs.insert(std::make_tuple((int)f.fuse_tail, (int)f.fused, f.fuse_tail ? lg_tail_waves(nw) : 0));
    }
    for (auto& t : lgs) std::printf("lg %d %d %d\n", std::get<0>(t), std::get<1>(t), std::get<2>(t));
    std::printf("waves %d %d %d %d\n", lg_tail_waves(0), lg_tail_waves(1), lg_tail_waves(4), lg_tail_waves(2));
    return 0;
  }
  const int D = atoi(argv[1]), heads = atoi(argv[2]), B = atoi(argv[3]), M = atoi(argv[4]), N = atoi(argv[5]);
  const Tuning t = tuning_from_env(env);
  const LgForm f = choose_lg_form(D, t.lg_fuse, t.lg_fuse_next);
  std::printf("lg %d %d %d\n", (int)f.fuse_tail, (int)f.fused, f.fuse_tail ? lg_tail_waves(t.lg_tail_nw) : 0);
  for (int cross = 0; cross < 2; ++cross) {
    LgAttLaunch l[2];
    const int n = lg_attention_launches(B, M, N, cross != 0, l);
    for (int j = 0; j < n; ++j) {
      AttForm a;
      const int e = choose_attention(l[j].S, l[j].T, heads, l[j].B, D, 1, t.att_ksplit, t.att_q, t.att_affine, a);
      std::printf("att %s %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", cross ? "cross" : "self", l[j].B, l[j].S, l[j].T, l[j].q_set,
                  l[j].k_set, l[j].kv_bshift, e, a.kernel, a.inst, (int)a.affine, a.gx, a.gy, a.gz, a.block);
    }
  }
  return 0;
}
"""

FP32, KSPLIT, SPLIT = 0, 1, 2       # attention_form.h AttKernel


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is required for the LightGlue form test")
    d = tmp_path_factory.mktemp("lg_forms")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    # no ROCm include path: the form headers must stay free of HIP
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "driver.cpp"), os.path.join(CSRC, "options.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def _parse(out):
    rec = {"att": []}
    for ln in out.splitlines():
        w = ln.split()
        if w[0] == "lg":
            rec["lg"] = tuple(int(x) for x in w[1:])       # (fuse_tail, fused, tail waves or 0)
        elif w[0] == "att":
            keys = ("B", "S", "T", "q_set", "k_set", "kv_bshift", "err", "kernel", "inst", "affine", "gx", "gy", "gz", "block")
            rec["att"].append(dict(zip(keys, (int(x) for x in w[2:])), block_kind=w[1]))
    return rec


@pytest.fixture(scope="module")
def table(driver):
    """{(case, form): the headers' choices for the case's forward in the form's environment}"""
    out = {}
    for case, c in R.CASES.items():
        conf = lg.get_config(R.conf_in(case))
        argv = [driver] + [str(v) for v in (conf["descriptor_dim"], conf["num_heads"], c["B"], c["M"], c["N"])]
        for form in R.FORMS:
            out[case, form] = _parse(subprocess.run(argv, check=True, capture_output=True, text=True, env=R.child_env(form)).stdout)
            assert all(a["err"] == 0 for a in out[case, form]["att"])
    return out


def test_table_reaches_every_form_the_headers_can_return(driver, table):
    att, lgf = set(), set()
    for ln in subprocess.run([driver, "enumerate"], check=True, capture_output=True, text=True).stdout.splitlines():
        w = ln.split()
        if w[0] == "waves":
            assert w[1:] == ["4", "1", "4", "0"]            # automatic, one, four, not built
        else:
            (att if w[0] == "att" else lgf).add(tuple(int(x) for x in w[1:]))
    assert att == {(KSPLIT, 0, 0), (SPLIT, 256, 0), (SPLIT, 256, 1), (SPLIT, 512, 0), (SPLIT, 512, 1)}      # pins the enumeration
    assert lgf == {(0, 0, 0), (1, 0, 1), (1, 0, 4), (1, 1, 1), (1, 1, 4)}
    got_att = {(a["kernel"], a["inst"], a["affine"]) for rec in table.values() for a in rec["att"]}
    got_lg = {rec["lg"] for rec in table.values()}
    assert got_att == att
    # (unfused projections with one-wave tails would need two knobs at once: the projections' fusion does not change the
    # tail's own arithmetic, and every form of the table sets one knob)
    assert got_lg == lgf - {(1, 0, 1)}
    # both decodings of the affine 1-D grid (the kernel's choice): sequences % 8 == 0 and heads * sequences % 8 == 0 only
    aff = {a["B"] % 8 == 0 for rec in table.values() for a in rec["att"] if a["affine"]}
    assert aff == {True, False}


def _att(table, case, form, kind=None):
    return [a for a in table[case, form]["att"] if kind is None or a["block_kind"] == kind]


def test_each_row_runs_the_form_it_is_named_for(table):
    d32 = [c for c in R.CASES if lg.get_config(R.conf_in(c))["descriptor_dim"] == 32]
    assert sorted(set(R.CASES) - set(d32)) == ["e"]
    for case in R.CASES:
        # the matcher's knobs leave the attention alone and the attention's knobs the matcher
        for form in ("unfused_tails", "unfused_projections", "one_wave_tails"):
            assert table[case, form]["att"] == table[case, "default"]["att"]
        for form in ("never_ksplit", "always_ksplit", "q128", "plain_grid"):
            assert table[case, form]["lg"] == table[case, "default"]["lg"]
        # -- the matcher's forms --
        assert table[case, "default"]["lg"] == ((1, 1, 4) if case in d32 else (0, 0, 0))
        assert table[case, "unfused_tails"]["lg"] == (0, 0, 0)
        assert table[case, "unfused_projections"]["lg"] == ((1, 0, 4) if case in d32 else (0, 0, 0))
        assert table[case, "one_wave_tails"]["lg"] == ((1, 1, 1) if case in d32 else (0, 0, 0))
        # -- the attention's forms --
        assert not any(a["kernel"] == KSPLIT for a in _att(table, case, "never_ksplit"))
        assert all((a["kernel"] == KSPLIT) == (a["T"] >= 128) for a in _att(table, case, "always_ksplit"))
        assert not any(a["inst"] == 512 for a in _att(table, case, "q128"))
        assert not any(a["affine"] for a in _att(table, case, "plain_grid"))
        for form in R.FORMS:
            for a in _att(table, case, form):
                assert a["kernel"] != FP32
                if a["kernel"] == KSPLIT:
                    assert (a["gx"], a["gy"], a["gz"], a["block"]) == (-(-a["S"] // 32), 4, a["B"], 256)
                else:
                    tiles = -(-a["S"] // (a["inst"] // 2))
                    assert (a["gx"], a["gy"], a["gz"]) == ((tiles * 4 * a["B"], 1, 1) if a["affine"] else (tiles, 4, a["B"]))
                    assert a["block"] == a["inst"]
    # -- the reason of each row --
    # a: T = 130 under key-split (the fourth wave has no keys: 64 keys per wave), T = 100 query-tiled on the affine grid;
    #    460 rows: a ragged 16-row group of the tails
    a = _att(table, "a", "default", "self")
    assert [(x["B"], x["S"], x["T"], x["kernel"], x["affine"]) for x in a] == [(2, 130, 130, KSPLIT, 0), (2, 100, 100, SPLIT, 1)]
    assert ((130 + 127) >> 7) << 5 == 64 and 3 * 64 >= 130 and (2 * 230) % 16 != 0
    assert [(x["S"], x["T"], x["q_set"], x["k_set"]) for x in _att(table, "a", "default", "cross")] == [(130, 100, 0, 1), (100, 130, 1, 0)]
    assert all(x["kernel"] == SPLIT and x["inst"] == 256 and x["affine"] for x in _att(table, "a", "never_ksplit"))
    assert all(not x["affine"] for x in _att(table, "a", "plain_grid") if x["kernel"] == SPLIT)
    # b: three 32-key rounds per wave under key-split; never key-split: the plain grid (4 pairs), three 128-query tiles with
    #    a ragged last one, three staging rounds of 128 keys
    assert all(x["kernel"] == KSPLIT and ((x["T"] + 127) >> 7) == 3 for x in _att(table, "b", "default"))
    b = _att(table, "b", "never_ksplit")
    assert len(b) == 4 and all(x["kernel"] == SPLIT and x["inst"] == 256 and not x["affine"] and x["gx"] == 3 and x["T"] > 256 for x in b)
    assert 300 % 128 and 257 % 128
    # c: one launch of 2B sequences per block, the cross block through kv_bshift; T < 128 is never key-split
    for form in R.FORMS:
        c = _att(table, "c", form)
        assert [(x["block_kind"], x["B"], x["S"], x["T"], x["kv_bshift"], x["kernel"]) for x in c] == \
            [("self", 6, 96, 96, 0, SPLIT), ("cross", 6, 96, 96, 3, SPLIT)]
    # d: M = N with long T: key-split by default, two staging rounds when query-tiled
    assert [(x["B"], x["T"], x["kv_bshift"], x["kernel"]) for x in _att(table, "d", "default")] == [(2, 200, 0, KSPLIT), (2, 200, 1, KSPLIT)]
    assert all(x["kernel"] == SPLIT and x["T"] > 128 for x in _att(table, "d", "never_ksplit"))
    # e: D = 64, head dim 16: the lg_linear chain in every form (asserted above), split-fp16 attention
    assert lg.get_config(R.conf_in("e"))["descriptor_dim"] // 4 == 16
    # f: input_proj
    assert lg.get_config(R.conf_in("f"))["input_dim"] != lg.get_config(R.conf_in("f"))["descriptor_dim"]
    # g: exactly the 512 workgroups attention_split_kernel<512, 6> asks for; 128 queries per workgroup on request;
    #    key-split when forced
    for form, want in (("default", (SPLIT, 512, 1, 512, 1, 1)), ("plain_grid", (SPLIT, 512, 0, 2, 4, 64)),
                       ("q128", (SPLIT, 256, 1, 768, 1, 1)), ("always_ksplit", (KSPLIT, 0, 0, 9, 4, 64)),
                       ("never_ksplit", (SPLIT, 512, 1, 512, 1, 1))):
        g = _att(table, "g", form)
        assert len(g) == 2 and all((x["kernel"], x["inst"], x["affine"], x["gx"], x["gy"], x["gz"]) == want for x in g), form
    # h: the padded sets run at their capacity, M = N
    assert [(x["B"], x["S"], x["T"]) for x in _att(table, "h", "default")] == [(6, 160, 160)] * 2
    # "always key-split" is set above every grid of the table
    assert max(-(-x["S"] // 128) * 4 * x["B"] for rec in table.values() for x in rec["att"]) < R.KSPLIT_ALWAYS


@pytest.mark.parametrize("case", list(R.CASES))
def test_inputs_meet_their_conditions_and_e32(case):
    """Conditions on the INPUTS, met by the float64 reference alone; E32 and the intermediate peak, printed."""
    kept, matched = R.input_conditions(case)
    for b, n0, n1, rec in R.reference(case):
        print(f"case {case} pair {b} {n0} x {n1}: E32 log_assignment {rec['e32_la']:.3e}, ref_descriptors {rec['e32_desc']:.3e}, "
              f"peak {rec['peak']:.4g}")
        # (the float32 oracle itself is inside the absolute bounds the device also has to meet)
        assert rec["finite"] and 0 < rec["e32_la"] < R.ABS_LA and 0 < rec["e32_desc"] < R.ABS_DESC
        assert rec["peak"] < R.PEAK_LIMIT
    print(f"case {case}: the mask keeps {kept:.3f} of the rows, {matched:.3f} are kept and matched")
    need_kept, need_matched = R.required_conditions(case)
    assert kept >= need_kept and matched >= need_matched
    if R.CASES[case]["family"] == "corresponding":      # scores from just above the threshold up to about 0.9
        (_b, _n0, _n1, rec) = R.reference(case)[0]
        s = rec["ref"]["matching_scores0"][rec["ref"]["matches0"] >= 0]
        print(f"case {case}: matched scores {s.min():.3f} .. {s.max():.3f}")
        assert s.max() > 0.5


def test_sweep_references_are_finite_and_say_where_the_device_is_checked():
    for k in R.SWEEP_K:
        (_b, _n0, _n1, rec), = R.reference("a", k)
        print(f"sweep 2^{k}: E32 log_assignment {rec['e32_la']:.3e}, ref_descriptors {rec['e32_desc']:.3e}, peak {rec['peak']:.4g}"
              f" ({'device checked' if rec['peak'] < R.PEAK_LIMIT else 'reference only'})")
        assert rec["finite"]
    assert R.reference("a", 0)[0][3]["peak"] < R.PEAK_LIMIT      # the unit-scale case itself is inside the range
