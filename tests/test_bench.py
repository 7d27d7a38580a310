"""bench.py's command line: the lean default line, --full, and --dump-outputs (the last timed step's results on disk)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SMALL = ["--gpus", "1", "--height", "64", "--width", "96", "--batch", "4", "--warmup", "1"]
DUMPED = {"score", "coord", "feat", "vlad", "seg", "keypoints", "descriptors", "keypoint_count"}


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, "bench.py", "--steps", "0"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain run times only the headline; --dump-outputs writes the last step's results, the same in two runs and the
    same as the product path computes on the bench's seeded frames."""
    import torch
    j = _bench(SMALL + ["--steps", "3", "--dump-outputs", str(tmp_path / "a")])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["higher_is_better"] is True and j["unit"] == "frames/s"
    assert j["metric"].startswith("frames/sec") and j["dtype"].startswith("f16x3")
    assert abs(j["value"] - 4 * 3 / (j["ms_per_step"] * 3e-3)) / j["value"] < 0.01
    assert not {"roofline", "precision_modes", "one_step_at_a_time", "cpu_baseline"} & set(j)
    _bench(SMALL + ["--steps", "2", "--dump-outputs", str(tmp_path / "b")])
    names = {f[:-4] for f in os.listdir(tmp_path / "a")}
    assert names == DUMPED and {f[:-4] for f in os.listdir(tmp_path / "b")} == DUMPED
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in names) <= 64_000_000
    for n, a in got.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        assert np.array_equal(a, np.load(tmp_path / "b" / (n + ".npy"))), n

    # the same step in this process: same weights, same frames (bench.py's generator seed), one stream
    sys.path.insert(0, ROOT)
    import bench
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    from nano_vs_slam_amd.selectors import select_and_gather
    dev = torch.device("cuda", 0)
    model = tiny_factory("S", 28)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in bench.seeded_state_dict(model).items()})
    model = model.to(dev).eval()
    model.training = False
    x = torch.rand(4, 3, 64, 96, device=dev, generator=torch.Generator(device=dev).manual_seed(7)) * 2.0 - 1.0
    with torch.no_grad():
        out = model.post_processing(model(x), 64, 96)
        _, _, cnt, pts, desc = select_and_gather(out["score"], out["coord"], out["feat"], 1000, 0.7)
    want = {k: v for k, v in out.items() if isinstance(v, torch.Tensor)}
    want.update(keypoints=pts, descriptors=desc, keypoint_count=cnt)
    assert set(want) == DUMPED
    for n, t in want.items():
        ref = t.float().cpu().numpy()
        assert got[n].shape == ref.shape, n
        np.testing.assert_allclose(got[n], ref, rtol=0, atol=1e-5, err_msg=n)


@pytest.mark.gpu
def test_bench_full_line_keeps_every_extra():
    j = _bench(SMALL + ["--steps", "3", "--full", "--profile-steps", "1", "--cpu-seconds", "2"])
    assert j["steps"] == 3 and j["value"] > 0
    assert set(j["precision_modes"]) == {"f16x3", "fp32"} and j["precision_modes"]["f16x3"]["ms_per_step"] == j["ms_per_step"]
    assert j["one_step_at_a_time"]["value"] > 0 and j["roofline"]["achieved"] > 0
    assert j["cpu_baseline"]["value"] > 0 and j["speedup_vs_cpu"] > 0
