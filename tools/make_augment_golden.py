"""Generate tests/golden/augment/ by running the REFERENCE's sample_homography (src/data/dataset_utils.py), loaded read-only
from a checkout of the reference, with its random draws recorded.

    python3 tools/make_augment_golden.py --reference PATH        (or KP2D_REFERENCE=PATH)

How the reference's module is run without its data stack: dataset_utils.py imports torchvision.transforms.v2, torchgeometry
and utils.utils at module level, none of which sample_homography reaches; EMPTY stand-in modules are registered under exactly
those names in THIS process before the file is loaded from its own path.  np.random.normal / uniform / randint are replaced,
for the duration of a call, by recording versions driven by one seeded numpy Generator: normal(loc, scale, size) returns
loc + scale z with z standard normal, uniform(low, high) returns low + (high - low) u, randint(n) returns floor(u n).  The
recorded values are laid out as include/kp2d.h's draws: z0..z3 (the two x and the two y perspective offsets), u_s and z_s (the
scale's index draw and the ONE of the n_scales normals that index picks; 0 when it picks scale 1), u_x, u_y, u_r.

Written: sampler.npz (draws_<case> [16, 9] and hom_<case> [16, 3, 3], the reference's returned matrices, float64; seeds_<case>)
and cases.json (shapes and switches).  Data, settings and seeds only.  A seed is kept only when every discrete choice of the
run (the clips, the angle validity tests, the index floors) is safe by 1e-9, measured on tests/augment_ref's restatement,
which must also reproduce the reference's matrix to 1e-9; refused seeds are printed.  No test, smoke() or bench.py reads the
reference; they read the committed fixtures.
"""
import argparse
import importlib.util
import json
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAFE = 1e-9
PER_CASE = 16
CASES = {
    "a_120x160": {"shape": [120, 160], "options": {}},
    "b_240x320": {"shape": [240, 320], "options": {}},
    "c_100x100": {"shape": [100, 100], "options": {}},
    "d_no_perspective": {"shape": [120, 160], "options": {"perspective": False}},
    "e_no_scaling": {"shape": [120, 160], "options": {"scaling": False}},
    "f_no_rotation": {"shape": [120, 160], "options": {"rotation": False}},
    "g_no_translation": {"shape": [120, 160], "options": {"translation": False}},
}
BASE_SEED = 9100


def reference_sampler(reference):
    """The reference's sample_homography from its own src/data/dataset_utils.py, empty stand-ins registered first."""
    reference = os.path.realpath(reference)
    for name in ("torchvision", "torchvision.transforms", "torchvision.transforms.v2", "torchgeometry", "utils", "utils.utils"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision.transforms"].v2 = sys.modules["torchvision.transforms.v2"]
    if not hasattr(sys.modules["utils.utils"], "load_json"):
        sys.modules["utils.utils"].load_json = None
    path = os.path.join(reference, "src", "data", "dataset_utils.py")
    spec = importlib.util.spec_from_file_location("kp2d_reference_dataset_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.realpath(mod.__file__).startswith(reference + os.sep):
        raise RuntimeError(f"{mod.__file__}: fixtures must come from the reference under {reference}")
    return mod.sample_homography


class Recorder:
    """Stands in for np.random during one call of the reference's function."""

    def __init__(self, seed):
        self.gen = np.random.default_rng(seed)
        self.normals, self.uniforms, self.ints = [], [], []

    def normal(self, loc, scale, size):
        z = self.gen.standard_normal(size)
        self.normals.append(z)
        return loc + scale * z

    def uniform(self, low, high):
        u = float(self.gen.random())
        self.uniforms.append(u)
        return low + (high - low) * u

    def randint(self, n):
        u = float(self.gen.random())
        self.ints.append(u)
        return int(math.floor(u * n))


def run_reference(sample, shape, options, seed, n_scales=100):
    """-> (draws [9], the reference's matrix)."""
    rec = Recorder(seed)
    saved = np.random.normal, np.random.uniform, np.random.randint
    np.random.normal, np.random.uniform, np.random.randint = rec.normal, rec.uniform, rec.randint
    try:
        hom = sample(shape, **options)
    finally:
        np.random.normal, np.random.uniform, np.random.randint = saved
    normals, ints, uniforms = list(rec.normals), list(rec.ints), list(rec.uniforms)
    d = np.zeros(9)
    if options.get("perspective", True):
        d[0:2], d[2:4] = normals.pop(0), normals.pop(0)
    if options.get("scaling", True):
        zs, d[4] = normals.pop(0), ints.pop(0)
        idx = int(math.floor(d[4] * n_scales))
        d[5] = zs[idx - 1] if idx else 0.0
    if options.get("translation", True):
        d[6], d[7] = uniforms
    if options.get("rotation", True):
        d[8] = ints.pop(0)
    assert not normals and not ints
    return d, np.asarray(hom, np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("KP2D_REFERENCE"), help="a checkout of the reference project")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        raise SystemExit("needs --reference PATH (or KP2D_REFERENCE): a checkout of the reference project")
    sample = reference_sampler(args.reference)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import augment_ref as ar
    os.makedirs(ar.GOLDEN, exist_ok=True)
    data = {}
    seed = BASE_SEED
    for name, case in CASES.items():
        draws, homs, seeds = [], [], []
        while len(draws) < PER_CASE:
            seed += 1
            d, hom = run_reference(sample, case["shape"], case["options"], seed)
            margins = []
            ours = ar.sample_homography(d, case["shape"], margins=margins, **case["options"])
            gap = float(np.abs(ours - hom).max())
            if min(margins, default=1.0) <= SAFE:
                print(f"case {name}: seed {seed} refused: a discrete choice is within {min(margins):.2e} of its threshold")
                continue
            assert gap <= 1e-9, f"case {name} seed {seed}: the restatement differs from the reference by {gap:.3e}"
            draws.append(d)
            homs.append(hom)
            seeds.append(seed)
        data["draws_" + name], data["hom_" + name], data["seeds_" + name] = np.stack(draws), np.stack(homs), np.asarray(seeds, np.int64)
        worst = max(float(np.abs(ar.sample_homography(d, case["shape"], **case["options"]) - h).max()) for d, h in zip(draws, homs))
        print(f"case {name}: {PER_CASE} draws, seeds {seeds[0]}..{seeds[-1]}, oracle-vs-reference {worst:.1e}")
    path = os.path.join(ar.GOLDEN, "sampler.npz")
    np.savez_compressed(path, **data)
    with open(os.path.join(ar.GOLDEN, "cases.json"), "w") as f:
        json.dump(CASES, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"sampler.npz: {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
