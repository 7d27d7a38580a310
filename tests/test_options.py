"""CPU unit test of nano-vs-slam_amd/csrc/options.h / options.cpp: the one table behind kp2d_set_option / kp2d_get_option and the
KP2D_* variables read by kp2d_create, and the launchers' process-wide Tuning.  Defaults, ranges and what each variable's text
does are written here as literals taken from the code the table replaced (kp2d_create, kp2d_set_option and the launchers'
function-static reads), never computed through the code under test.  Plain C++, compiled here with g++ and a small driver that
takes a fake environment; no hipcc, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "nano-vs-slam_amd", "csrc")
INT_MAX = 2**31 - 1

# argv: NAME=value (the fake environment; NAME= is the empty string), then set:KEY:VALUE / get:KEY operations on the Options
# that options_from_env filled.  Prints the table, the Options, the Tuning, then one line per operation.
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include "api_common.h"
#include "options.h"
static std::string g_err;
namespace kp2d { void set_last_error(const char* msg) { g_err = msg ? msg : ""; } }
static std::map<std::string, std::string> g_env;
static const char* fake_getenv(const char* name) {
  const auto it = g_env.find(name);
  return it == g_env.end() ? nullptr : it->second.c_str();
}
int main(int argc, char** argv) {
  using namespace kp2d;
  int i = 1;
  for (; i < argc && std::strncmp(argv[i], "set:", 4) && std::strncmp(argv[i], "get:", 4); ++i) {
    const char* eq = std::strchr(argv[i], '=');
    if (!eq) return 2;
    g_env[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
  }
  for (const OptionRow& r : kOptions)
    std::printf("row %s %s %ld %ld %ld\n", r.key ? r.key : "-", r.var ? r.var : "-", r.def, r.min, r.max);
  for (int k = 0; option_name(k); ++k) std::printf("name %d %s\n", k, option_name(k));
  Options o;
  options_from_env(o, fake_getenv);
  for (const OptionRow& r : kOptions) std::printf("opt %s %d\n", r.key ? r.key : r.var, o.*r.field);
  std::printf("opt lanes_default %d\n", o.lanes_default);
  const Tuning t = tuning_from_env(fake_getenv);
  std::printf("tune KP2D_MATCH_MFMA %d\ntune KP2D_TOPK_SMALL %d\ntune KP2D_GATHER_LDS %d\ntune KP2D_VLAD_PX %d\n", (int)t.match_mfma,
              t.topk_small, (int)t.gather_lds, t.vlad_px);
  std::printf("tune KP2D_VLAD_SPLIT %d\ntune KP2D_ATT_KSPLIT %ld\ntune KP2D_ATT_Q %d\ntune KP2D_ATT_AFFINE %d\n", (int)t.vlad_split,
              t.att_ksplit, t.att_q, (int)t.att_affine);
  std::printf("tune KP2D_LG_FUSE %d\ntune KP2D_LG_FUSE_NEXT %d\ntune KP2D_LG_TAIL_NW %d\n", (int)t.lg_fuse, (int)t.lg_fuse_next,
              t.lg_tail_nw);
  for (; i < argc; ++i) {
    std::string op = argv[i];
    g_err.clear();
    if (op.compare(0, 4, "set:") == 0) {
      const size_t c = op.rfind(':');
      const int rc = set_option(o, op.substr(4, c - 4).c_str(), atol(op.c_str() + c + 1));
      std::printf("set %d|%s\n", rc, g_err.c_str());
    } else {
      long v = -12345;
      const int rc = get_option(o, op.c_str() + 4, &v);
      std::printf("get %d %ld|%s\n", rc, v, g_err.c_str());
    }
  }
  return 0;
}
"""

# key -> (variable, default, min, max): the literals of the field initialisers and of kp2d_set_option's range checks before the table
KEYED = {
    "wsm_min_items": ("KP2D_WSM", 0, -1, INT_MAX),
    "ws_min_tiles": (None, 0, 0, INT_MAX),
    "wsm_grid": ("KP2D_WSM_GRID", 0, 0, 65536),
    "wsm_transposed": ("KP2D_WSM_TR", 0, 0, 2),
    "s16_min_items": ("KP2D_S16", 0, -1, INT_MAX),
    "s16_all": ("KP2D_S16ALL", 1, 0, 1),
    "multi_launch": ("KP2D_MULTI", 1, 0, 1),
    "mff_fused": ("KP2D_MFF", 1, 0, 1),
    "stem_fusion": ("KP2D_STEM", 1, 0, 2),
    "side_overlap": ("KP2D_SIDE", 1, 0, 1),
    "lanes": ("KP2D_LANES", 2, 0, 8),
}
VAR_ONLY = {"KP2D_DBG": 0, "KP2D_LANE_PRIORITY": 0}
DEFAULTS = dict({k: v[1] for k, v in KEYED.items()}, lanes_default=2, **VAR_ONLY)
TUNING_DEFAULTS = {"KP2D_MATCH_MFMA": 1, "KP2D_TOPK_SMALL": 256, "KP2D_GATHER_LDS": 1, "KP2D_VLAD_PX": 320, "KP2D_VLAD_SPLIT": 1,
                   "KP2D_ATT_KSPLIT": 256, "KP2D_ATT_Q": 256, "KP2D_ATT_AFFINE": 1, "KP2D_LG_FUSE": 1, "KP2D_LG_FUSE_NEXT": 1,
                   "KP2D_LG_TAIL_NW": 0}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    d = tmp_path_factory.mktemp("options")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    # no ROCm include path: options.* must stay free of HIP
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "driver.cpp"), os.path.join(CSRC, "options.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def run(driver, env=None, ops=()):
    argv = [f"{k}={v}" for k, v in (env or {}).items()] + list(ops)
    out = subprocess.run([driver, *argv], check=True, capture_output=True, text=True).stdout.splitlines()
    rec = {"rows": [], "names": [], "opt": {}, "tune": {}, "ops": []}
    for ln in out:
        kind, _, rest = ln.partition(" ")
        if kind == "row":
            key, var, *nums = rest.split()
            rec["rows"].append((None if key == "-" else key, None if var == "-" else var, *map(int, nums)))
        elif kind == "name":
            rec["names"].append(rest.split()[1])
        elif kind in ("opt", "tune"):
            rec[kind][rest.split()[0]] = int(rest.split()[1])
        else:
            vals, _, err = rest.partition("|")
            rec["ops"].append((*map(int, vals.split()), err))
    return rec


def test_table_holds_the_defaults_and_ranges_of_the_code_it_replaced(driver):
    rec = run(driver)
    assert {r[0]: r[1:] for r in rec["rows"] if r[0]} == KEYED
    assert sorted(r[1] for r in rec["rows"] if r[0] is None) == sorted(VAR_ONLY)
    assert all(r[2] == 0 for r in rec["rows"] if r[0] is None)
    assert rec["names"] == [r[0] for r in rec["rows"] if r[0]] and len(rec["names"]) == 11
    assert rec["opt"] == DEFAULTS
    assert rec["tune"] == TUNING_DEFAULTS


# (variable, text, {option: value it must have afterwards}); every option not named keeps its default
ENV_CASES = [
    ("KP2D_LANES", "", {"lanes": 1, "lanes_default": 1}), ("KP2D_LANES", "0", {"lanes": 1, "lanes_default": 1}),
    ("KP2D_LANES", "12", {"lanes": 8, "lanes_default": 8}), ("KP2D_LANES", "3", {"lanes": 3, "lanes_default": 3}),
    ("KP2D_SIDE", "0", {"side_overlap": 0}), ("KP2D_SIDE", "0x", {"side_overlap": 0}), ("KP2D_SIDE", "1", {}), ("KP2D_SIDE", "", {}),
    ("KP2D_SIDE", "off", {}),
    ("KP2D_MFF", "0", {"mff_fused": 0}), ("KP2D_MFF", "1", {}), ("KP2D_MFF", "", {}), ("KP2D_MFF", "no", {}),
    ("KP2D_STEM", "7", {"stem_fusion": 2}), ("KP2D_STEM", "-1", {"stem_fusion": 0}), ("KP2D_STEM", "abc", {"stem_fusion": 0}),
    ("KP2D_STEM", "", {"stem_fusion": 0}), ("KP2D_STEM", "2", {"stem_fusion": 2}), ("KP2D_STEM", "1", {}),
    ("KP2D_DBG", "5", {"KP2D_DBG": 5}), ("KP2D_DBG", "-3", {"KP2D_DBG": -3}), ("KP2D_DBG", "100000", {"KP2D_DBG": 100000}),
    ("KP2D_LANE_PRIORITY", "-1", {"KP2D_LANE_PRIORITY": -1}), ("KP2D_LANE_PRIORITY", "9", {"KP2D_LANE_PRIORITY": 9}),
    ("KP2D_WSM", "0", {"wsm_min_items": -1}), ("KP2D_WSM", "100", {"wsm_min_items": 100}),
    ("KP2D_WSM", "99999999999", {"wsm_min_items": INT_MAX}), ("KP2D_WSM", "-3", {}), ("KP2D_WSM", "", {}),
    ("KP2D_WSM_GRID", "64", {"wsm_grid": 64}), ("KP2D_WSM_GRID", "100000", {"wsm_grid": 65536}), ("KP2D_WSM_GRID", "0", {}),
    ("KP2D_WSM_GRID", "-1", {}), ("KP2D_WSM_GRID", "", {}),
    ("KP2D_WSM_TR", "1", {"wsm_transposed": 1}), ("KP2D_WSM_TR", "2", {"wsm_transposed": 2}), ("KP2D_WSM_TR", "0", {}),
    ("KP2D_WSM_TR", "3", {}), ("KP2D_WSM_TR", "-1", {}), ("KP2D_WSM_TR", "", {}),
    ("KP2D_S16", "0", {"s16_min_items": -1}), ("KP2D_S16", "1", {}), ("KP2D_S16", "64", {}), ("KP2D_S16", "", {}),
    ("KP2D_S16ALL", "0", {"s16_all": 0}), ("KP2D_S16ALL", "1", {}), ("KP2D_S16ALL", "", {}),
    ("KP2D_MULTI", "0", {"multi_launch": 0}), ("KP2D_MULTI", "1", {}), ("KP2D_MULTI", "", {}),
]


@pytest.mark.parametrize("var,text,changed", ENV_CASES, ids=[f"{v}={t!r}" for v, t, _ in ENV_CASES])
def test_variable_text_becomes_the_option_value(driver, var, text, changed):
    assert run(driver, {var: text})["opt"] == dict(DEFAULTS, **changed)


def test_variables_act_together(driver):
    env = {"KP2D_LANES": "3", "KP2D_WSM": "0", "KP2D_WSM_GRID": "64", "KP2D_WSM_TR": "2", "KP2D_S16": "0", "KP2D_S16ALL": "0",
           "KP2D_MULTI": "0", "KP2D_SIDE": "0", "KP2D_MFF": "0", "KP2D_STEM": "2", "KP2D_UNRELATED": "1"}
    want = dict(DEFAULTS, lanes=3, lanes_default=3, wsm_min_items=-1, wsm_grid=64, wsm_transposed=2, s16_min_items=-1, s16_all=0,
                multi_launch=0, side_overlap=0, mff_fused=0, stem_fusion=2)
    assert run(driver, env)["opt"] == want


TUNING_CASES = [
    ({"KP2D_MATCH_MFMA": "0", "KP2D_GATHER_LDS": "0", "KP2D_VLAD_SPLIT": "0", "KP2D_ATT_AFFINE": "0", "KP2D_LG_FUSE": "0",
      "KP2D_LG_FUSE_NEXT": "0"},
     {"KP2D_MATCH_MFMA": 0, "KP2D_GATHER_LDS": 0, "KP2D_VLAD_SPLIT": 0, "KP2D_ATT_AFFINE": 0, "KP2D_LG_FUSE": 0, "KP2D_LG_FUSE_NEXT": 0}),
    # anything but a leading '0' leaves a switch on
    ({"KP2D_MATCH_MFMA": "1", "KP2D_GATHER_LDS": "", "KP2D_VLAD_SPLIT": "off", "KP2D_ATT_AFFINE": "-0", "KP2D_LG_FUSE": "2",
      "KP2D_LG_FUSE_NEXT": " 0"}, {}),
    ({"KP2D_TOPK_SMALL": "64", "KP2D_VLAD_PX": "160", "KP2D_ATT_KSPLIT": "0", "KP2D_ATT_Q": "128", "KP2D_LG_TAIL_NW": "1"},
     {"KP2D_TOPK_SMALL": 64, "KP2D_VLAD_PX": 160, "KP2D_ATT_KSPLIT": 0, "KP2D_ATT_Q": 128, "KP2D_LG_TAIL_NW": 1}),
    # a number variable that is set replaces the default whatever it holds: atoi / atol of the text
    ({"KP2D_TOPK_SMALL": "", "KP2D_VLAD_PX": "abc", "KP2D_ATT_KSPLIT": "-5", "KP2D_ATT_Q": "", "KP2D_LG_TAIL_NW": "2x"},
     {"KP2D_TOPK_SMALL": 0, "KP2D_VLAD_PX": 0, "KP2D_ATT_KSPLIT": -5, "KP2D_ATT_Q": 0, "KP2D_LG_TAIL_NW": 2}),
]


@pytest.mark.parametrize("env,changed", TUNING_CASES, ids=["off", "not-off", "numbers", "odd-numbers"])
def test_tuning_reads_the_launcher_variables(driver, env, changed):
    rec = run(driver, env)
    assert rec["tune"] == dict(TUNING_DEFAULTS, **changed)
    assert rec["opt"] == DEFAULTS      # (none of them is a model option)


@pytest.mark.parametrize("key", sorted(KEYED))
def test_set_option_accepts_min_and_max_and_refuses_beyond(driver, key):
    _, default, lo, hi = KEYED[key]
    ops = [f"get:{key}", f"set:{key}:{hi}", f"get:{key}", f"set:{key}:{hi + 1}", f"get:{key}", f"set:{key}:{lo - 1}", f"get:{key}",
           f"set:{key}:{lo}", f"get:{key}", f"set:{key}:{hi + 1}", f"set:{key}:{lo - 1}", f"get:{key}"]
    got = run(driver, None, ops)["ops"]
    at_lo = default if key == "lanes" else lo      # ("lanes" = 0 restores the initial value)
    assert [g[:-1] for g in got] == [(0, default), (0,), (0, hi), (-1,), (0, hi), (-1,), (0, hi), (0,), (0, at_lo), (-1,), (-1,),
                                     (0, at_lo)]
    for g in got:
        assert (g[-1] == "") == (g[0] == 0)
        assert g[0] == 0 or key in g[-1]      # the refusal names the option


def test_unknown_and_variable_only_keys_are_refused(driver):
    names = ["no_such_option", "", "KP2D_DBG", "dbg", "KP2D_LANE_PRIORITY", "lane_prio", "lanes_default", "KP2D_WSM"]
    got = run(driver, None, [op for n in names for op in (f"set:{n}:1", f"get:{n}")])
    for n, s, g in zip(names, got["ops"][0::2], got["ops"][1::2]):
        assert s == (-1, f"unknown option '{n}'") and g == (-1, -12345, f"unknown option '{n}'")


def test_lanes_zero_restores_the_variables_value(driver):
    got = run(driver, {"KP2D_LANES": "3"}, ["get:lanes", "set:lanes:5", "get:lanes", "set:lanes:0", "get:lanes", "set:lanes:9", "get:lanes"])
    assert [g[:-1] for g in got["ops"]] == [(0, 3), (0,), (0, 5), (0,), (0, 3), (-1,), (0, 3)]


def _readme_knob_table():
    rows = [ln for ln in open(os.path.join(ROOT, "README.md"), encoding="utf-8") if ln.startswith("| `KP2D_")]
    assert rows
    return "".join(rows)


def test_every_variable_is_in_the_readme_and_every_key_is_documented(driver):
    rec = run(driver)
    table = _readme_knob_table()
    for var in [r[1] for r in rec["rows"] if r[1]] + list(rec["tune"]):
        assert re.search(r"`%s\b" % var, table), f"{var} is missing from README.md's table of knobs"
    docs = table + open(os.path.join(ROOT, "include", "kp2d.h")).read()
    for key in rec["names"]:
        assert f'"{key}"' in docs, f'option "{key}" is in neither include/kp2d.h nor README.md'


def test_the_environment_is_read_in_one_place():
    counts = {}
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if os.path.isfile(path) and name.endswith((".hip", ".cpp", ".h", ".inc")):
            n = open(path, encoding="utf-8").read().count("getenv(")
            if n:
                counts[name] = n
    assert counts.get("kp2d_api.cpp") == 1, counts
    assert set(counts) <= {"kp2d_api.cpp", "options.cpp", "options.h"}, counts
