"""The options table (nano-vs-slam_amd/csrc/options.h) seen from outside the library: kp2d_set_option / kp2d_get_option /
kp2d_option_name on a real handle, and the KP2D_* variables becoming option values in kp2d_create.  kp2d_create needs a visible
HIP device, hence the gpu mark; no kernel is launched.  The variables are read when the handle is created, so they are set in
fresh child processes (ctypes only, one at a time)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from test_options import KEYED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def s_config():
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    return tiny_factory("S", 28)._engine_config(0)      # KP2DTiny-S; no weights are needed


@pytest.fixture()
def handle(s_config):
    from nano_vs_slam_amd import _lib
    lib, h = _lib.load(), C.c_void_p()
    _lib.check(lib.kp2d_create(C.byref(s_config), C.byref(h)))
    yield lib, h
    lib.kp2d_destroy(h)


def _names(lib):
    out, key = [], C.c_char_p()
    while lib.kp2d_option_name(len(out), C.byref(key)) == 0:
        out.append(key.value.decode())
    return out


def _get(lib, h, key):
    v = C.c_long(-12345)
    assert lib.kp2d_get_option(h, key.encode(), C.byref(v)) == 0, key
    return v.value


def test_every_option_round_trips_at_min_and_max(handle):
    lib, h = handle
    names = _names(lib)
    assert sorted(names) == sorted(KEYED)
    assert lib.kp2d_option_name(len(names), C.byref(C.c_char_p())) == -1 and lib.kp2d_option_name(-1, C.byref(C.c_char_p())) == -1
    assert lib.kp2d_option_name(0, None) == -1
    for key in names:
        _, _, lo, hi = KEYED[key]
        initial = _get(lib, h, key)      # (readable before any set)
        for value in (hi, lo):
            assert lib.kp2d_set_option(h, key.encode(), value) == 0, (key, value)
            assert _get(lib, h, key) == (initial if (key, value) == ("lanes", 0) else value)      # "lanes" = 0: the initial count
        assert lib.kp2d_set_option(h, key.encode(), hi) == 0
        for bad in (lo - 1, hi + 1):
            assert lib.kp2d_set_option(h, key.encode(), bad) == -1 and key.encode() in lib.kp2d_last_error()
            assert _get(lib, h, key) == hi


def test_unknown_key_and_null_arguments_are_refused(handle):
    lib, h = handle
    v = C.c_long(7)
    for key in (b"no_such_option", b"KP2D_DBG", b"lane_prio"):
        assert lib.kp2d_set_option(h, key, 1) == -1 and b"unknown option" in lib.kp2d_last_error()
        assert lib.kp2d_get_option(h, key, C.byref(v)) == -1 and b"unknown option" in lib.kp2d_last_error()
    assert v.value == 7
    assert lib.kp2d_get_option(None, b"lanes", C.byref(v)) == -1
    assert lib.kp2d_get_option(h, None, C.byref(v)) == -1
    assert lib.kp2d_get_option(h, b"lanes", None) == -1


def test_side_overlap_off_and_on_before_any_forward(handle):
    lib, h = handle
    assert lib.kp2d_set_option(h, b"side_overlap", 0) == 0 and _get(lib, h, "side_overlap") == 0
    assert lib.kp2d_set_option(h, b"side_overlap", 1) == 0 and _get(lib, h, "side_overlap") == 1


# a fresh process: creates a handle from the configuration in argv[1], applies "key=value" settings from argv[2:], prints every option
CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from nano_vs_slam_amd import _lib
lib, h = _lib.load(), C.c_void_p()
cfg = _lib.Kp2dConfig.from_buffer_copy(bytes.fromhex(sys.argv[1]))
_lib.check(lib.kp2d_create(C.byref(cfg), C.byref(h)))
for kv in sys.argv[2:]:
    _lib.check(lib.kp2d_set_option(h, kv.split("=")[0].encode(), int(kv.split("=")[1])))
out, key, v = {}, C.c_char_p(), C.c_long()
while lib.kp2d_option_name(len(out), C.byref(key)) == 0:
    _lib.check(lib.kp2d_get_option(h, key.value, C.byref(v)))
    out[key.value.decode()] = v.value
lib.kp2d_destroy(h)
print(json.dumps(out))
""" % ROOT


def _child(s_config, env, *settings):
    base = {k: v for k, v in os.environ.items() if not k.startswith("KP2D_") or k == "KP2D_LIB"}
    r = subprocess.run([sys.executable, "-c", CHILD, bytes(s_config).hex(), *settings], env=dict(base, **env), capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[-1])


def test_variables_become_the_documented_option_values(s_config):
    assert _child(s_config, {}) == {k: v[1] for k, v in KEYED.items()}
    env = {"KP2D_LANES": "3", "KP2D_WSM": "0", "KP2D_WSM_GRID": "64", "KP2D_WSM_TR": "2", "KP2D_S16": "0", "KP2D_S16ALL": "0",
           "KP2D_MULTI": "0", "KP2D_SIDE": "0", "KP2D_MFF": "0", "KP2D_STEM": "2"}
    want = {"lanes": 3, "wsm_min_items": -1, "wsm_grid": 64, "wsm_transposed": 2, "s16_min_items": -1, "s16_all": 0, "multi_launch": 0,
            "side_overlap": 0, "mff_fused": 0, "stem_fusion": 2, "ws_min_tiles": 0}
    assert _child(s_config, env, "lanes=5", "lanes=0") == want
