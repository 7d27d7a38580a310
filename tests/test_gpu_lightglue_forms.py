"""LightGlue and its attention in every launch form, against the float64 oracle (table, inputs, reference, tolerance:
lightglue_fp64_ref.py; the proof that each (case, form) pair runs the kernels it is named for: test_lightglue_forms.py).

The knobs of csrc/options.h are read once per process, so every form gets a fresh child process with its variable set.
The child runs the whole case table (and, in two forms, the magnitude sweep) through the product LightGlue module and
writes one .npz; this process holds the float64 references, computed once per case and shared by all forms, and compares.
Children run one after another, each under its own time limit, the first time a test of their form needs them.  After a
child that ended with anything but status 0 no further child is started: the tests of the forms that did not run fail."""
import subprocess
import sys

import numpy as np
import pytest

import lightglue_fp64_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT = 180      # seconds; a child takes a few (process start, eight small forwards)


class Runner:
    def __init__(self, tmp):
        self.tmp, self.done, self.broken = tmp, {}, None

    def sweep_ks(self, form):
        if form not in R.SWEEP_FORMS:
            return []
        return [k for k in R.SWEEP_K if R.reference("a", k)[0][3]["peak"] < R.PEAK_LIMIT]

    def get(self, form):
        if form in self.done:
            return self.done[form]
        if self.broken:
            pytest.fail(f"form {form} did not run: {self.broken}")
        out = self.tmp / f"{form}.npz"
        argv = [sys.executable, "-c", R.CHILD, ROOT, str(out)] + [str(k) for k in self.sweep_ks(form)]
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
    return Runner(tmp_path_factory.mktemp("lg_forms_gpu"))


@pytest.mark.parametrize("case", list(R.CASES))
@pytest.mark.parametrize("form", list(R.FORMS))
def test_form_against_float64(runner, form, case):
    z = runner.get(form)
    kept, matched = R.input_conditions(case)
    need_kept, need_matched = R.required_conditions(case)
    assert kept >= need_kept and matched >= need_matched          # (conditions on the inputs: test_lightglue_forms.py)
    fig, bad = R.compare(case, R.unpack(z, case))
    print(R.format_figures(form, case, fig))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("k", R.SWEEP_K)
@pytest.mark.parametrize("form", R.SWEEP_FORMS)
def test_magnitude_sweep(runner, form, k):
    """Case a (config S: the descriptors enter the residual stream unchanged) with both descriptor sets times 2^k.  The
    device must be finite and within the bound wherever the reference's intermediate peak is below 2^15; above, only the
    reference's finiteness is checked and the device is not run.  Matches are not compared (at small scales the oracle
    leaves no clear rows); the absolute bounds belong to the unit scale.
    What this sweep found (log_assignment error / E32, both forms alike; figures: profiles/lightglue_forms_fp64.txt):
    lg_finalize_kernel summed 2 sim + (ls0 - lse_row) - lse_col, which cancels at |sim| and leaves its ulp: 17 x at 2^4,
    3500 x at 2^8, 36000 x at 2^12; with each maximum subtracted from sim first 0.7 x, 2.5 x, 4.7 x.  The rest at 2^12 was
    the matchability logit of the fused final projection (a cancelling sum as a split-fp16 product; the unfused fp32
    lg_linear form measured 0.9 x): as an fp32 dot product 1.75 x at 2^8 and 1.47 x at 2^12, at a peak of 1.1e4."""
    (_b, _n0, _n1, rec), = R.reference("a", k)
    assert rec["finite"]
    if not rec["peak"] < R.PEAK_LIMIT:
        print(f"{form} 2^{k}: peak {rec['peak']:.4g} >= 2^15, device not run")
        return
    z = runner.get(form)
    fig, bad = R.compare("a", R.unpack(z, f"sweep{k}"), k=k, matches=False, absolute=(k == 0))
    print(R.format_figures(form, "a", fig, k))
    assert not bad, "\n".join(bad)
