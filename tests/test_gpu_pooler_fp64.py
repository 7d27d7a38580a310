"""The descriptor poolers behind vlad_head.convlad3 — NetVLAD in every launch form, GeM, ConvAP and the L2-normalised
encoder map — against float64 on the device's own tapped input (table, references, bound: pooler_fp64_ref.py; the proof
that every case runs the form it is named for and that the bound has teeth: test_pooler_ref_cpu.py).

Per case and arithmetic mode:
1. a profiled forward's ``vlad_head.netvlad`` kernel string (csrc/netvlad_form.h) equals the declared form;
2. the tapped forward's outputs are bit-identical to the untapped forward's;
3. E <= bound, printed as a fraction of the bound, every output finite; regime z: the map (and the encoder map) exactly 0;
4. regimes u and s: vlad_training.netvlad_forward on the same tap meets the exact-form bound against the same reference;
5. regime s: the input conditions hold on the tap.
The forms behind KP2D_VLAD_PX, read once per process, run in one child process per value, one after another, each under its
own time limit; after a child that ended with anything but status 0 no further child is started and the tests of the forms
that did not run fail.  The slab-mode cases also compare their first frames bit for bit with the same frames run alone in
tile mode.  Figures: profiles/pooler_fp64.txt."""
import subprocess
import sys

import numpy as np
import pytest

import pooler_fp64_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT = 240      # seconds; a child takes a few (process start, its cases in both modes; the largest: 128 frames of 48 x 64)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.cases())
def test_pooler_against_float64(case, mode):
    line, bad = R.evaluate(case, mode, R.device_run(case, mode))
    print("\n" + line)
    assert not bad, (case, mode, bad)


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
    return Runner(tmp_path_factory.mktemp("pooler_forms_gpu"))


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("form,case", [(f, c) for f in R.FORMS for c in R.cases(form=f)])
def test_tuned_form_against_float64(runner, form, case, mode):
    line, bad = R.evaluate(case, mode, R.unpack(runner.get(form), case, mode))
    print("\n" + line)
    assert not bad, (case, mode, bad)
