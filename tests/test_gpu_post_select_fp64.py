"""Keypoint post-processing and selection in every launch form against float64 (tables, references, bounds:
post_select_ref.py; the proof that every case runs the form it is named for and that the bounds have teeth:
test_post_select_ref_cpu.py).

kp2d_post per case, once with dense and once with sampled class ids (bit-identical score, coord and desc): score equal, coord
and desc within their per-element bounds (printed as the largest fraction of the bound), NaN exactly where the reference's
norm is 0, dense ids equal to numpy.argmax, sampled ids equal to float64 nearest sampling at the returned coordinates.
kp2d_select_topk and kp2d_gather_keypoints per form: equal to the reference.  Every output sits between guard elements.
The forms behind KP2D_TOPK_SMALL, KP2D_GATHER_LDS=0 and KP2D_MATCH_MFMA=0, read once per process, run in one child process per
value, one after another, each under its own time limit; after a child that ended with anything but status 0 no further
child is started and the tests of the forms that did not run fail.  Figures: profiles/post_select_fp64.txt."""
import subprocess
import sys

import numpy as np
import pytest

import post_select_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT = 240      # seconds; a child takes a few (process start, its cases; the largest: 80 pairs of 400 x 1100 descriptors)
TOPK = R.topk_cases()


@pytest.mark.parametrize("case", list(R.POST_CASES))
def test_post_against_float64(case):
    line, bad = R.evaluate_post(case, R.device_post(case))
    print("\n" + line)
    assert not bad, (case, bad)


@pytest.mark.parametrize("shape,regime,thr", TOPK, ids=[R.topk_id(*c) for c in TOPK])
def test_topk_against_the_reference(shape, regime, thr):
    line, bad = R.evaluate_topk(shape, regime, thr, R.device_topk(shape, regime, thr))
    print("\n" + line + "  " + R.TOPK_SHAPES[shape][2])
    assert not bad, (shape, regime, thr, bad)


@pytest.mark.parametrize("case", list(R.GATHER_CASES))
def test_gather_against_plain_indexing(case):
    line, bad = R.evaluate_gather(case, R.device_gather(case))
    print("\n" + line)
    assert not bad, (case, bad)


class Runner:
    def __init__(self, tmp):
        self.tmp, self.done, self.broken = tmp, {}, None

    def get(self, form):
        if form in self.done:
            return self.done[form]
        if self.broken:
            pytest.fail(f"form {form} did not run: {self.broken}")
        out = self.tmp / f"{form}.npz"
        argv = [sys.executable, "-c", R.CHILD, ROOT, form, str(out)]
        try:
            r = subprocess.run(argv, env=R.child_env(form), cwd=ROOT, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
            status, tail = r.returncode, (r.stdout + r.stderr)[-2000:]
        except subprocess.TimeoutExpired as e:
            status, tail = "time limit", str(e)
        if status != 0:
            self.broken = f"the child of form {form} ended with {status}; no further child is started\n{tail}"
            pytest.fail(self.broken)
        self.done[form] = np.load(out)
        return self.done[form]


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    return Runner(tmp_path_factory.mktemp("post_select_forms_gpu"))


KNOB = [(f, k) for f in R.FORMS for k in R.form_cases(f)]


@pytest.mark.parametrize("form,key", KNOB, ids=[f"{f}-{R.form_key(k).replace('/', '-')}" for f, k in KNOB])
def test_knob_form_against_the_reference(runner, form, key):
    rec = R.unpack(runner.get(form), key)
    assert rec, (form, key)
    if key[0] == "topk":
        line, bad = R.evaluate_topk(*key[1:], rec)
        line += "  " + R.TOPK_KNOB_SHAPES[key[1]][2][int(R.FORMS[form]["KP2D_TOPK_SMALL"])]
    elif key[0] == "gather":
        line, bad = R.evaluate_gather(key[1], rec, form=R.D_)
    else:
        line, bad = R.evaluate_match(key[1], rec)
    print(f"\n{line}  [{' '.join(f'{k}={v}' for k, v in R.FORMS[form].items())}]")
    assert not bad, (form, key, bad)
