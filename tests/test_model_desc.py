"""CPU unit test of nano-vs-slam_amd/csrc/model_desc.cpp: which state-dict tensors the engine consumes for every configuration
(names and shapes against the oracle's restatement of the reference's constructors: what _Engine.upload enforces on a GPU box)
and that pack() turns seeded weights into the blob, deterministically and at the size the GPU handle reports.  The file is
plain C++ and is compiled here with g++ together with a small driver; no hipcc, no GPU."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from nano_vs_slam_amd.synthetic import spread_state_dict
from oracle import kp2d_oracle as orc

CSRC = os.path.join(ROOT, "nano-vs-slam_amd", "csrc")
N_CLASSES = 28

# argv: version, channel_dims[6], nfeatures, n_classes, num_clusters, encoder_dim, downsample, use_attention, leaky_relu,
# global_descriptor, remove_netvlad, depth, upscale_method, in_channels [weights.bin blob.bin]
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include "model_desc.h"
static std::string g_err;
namespace kp2d { void set_last_error(const char* msg) { g_err = msg ? msg : ""; } }
int main(int argc, char** argv) {
  if (argc < 20) return 2;
  kp2d::ModelDesc m;
  int i = 1;
  m.cfg.struct_size = (int32_t)sizeof(kp2d_config);
  m.cfg.version = atoi(argv[i++]);
  for (int k = 0; k < 6; ++k) m.cfg.channel_dims[k] = atoi(argv[i++]);
  m.cfg.nfeatures = atoi(argv[i++]); m.cfg.n_classes = atoi(argv[i++]); m.cfg.num_clusters = atoi(argv[i++]);
  m.cfg.encoder_dim = atoi(argv[i++]); m.cfg.downsample = atoi(argv[i++]); m.cfg.use_attention = atoi(argv[i++]);
  m.cfg.leaky_relu = atoi(argv[i++]); m.cfg.global_descriptor = atoi(argv[i++]); m.cfg.remove_netvlad = atoi(argv[i++]);
  m.cfg.depth = atoi(argv[i++]); m.cfg.upscale_method = atoi(argv[i++]); m.cfg.in_channels = atoi(argv[i++]);
  if (kp2d::describe(&m) != KP2D_OK) { std::printf("ERROR %s\n", g_err.c_str()); return 1; }
  for (const auto& s : m.specs) {
    std::printf("%s", s.key.c_str());
    for (auto d : s.shape) std::printf(" %lld", (long long)d);
    std::printf("\n");
  }
  std::printf("blob_floats %zu\n", m.blob_floats);
  if (argc < 22) return 0;
  FILE* f = std::fopen(argv[i++], "rb");      // the tensors of `specs`, in that order, float32
  if (!f) return 3;
  for (const auto& s : m.specs) {
    std::vector<float>& v = m.host[s.key];
    v.resize(s.numel());
    if (std::fread(v.data(), sizeof(float), v.size(), f) != v.size()) return 4;
  }
  std::fclose(f);
  std::vector<float> blob;
  if (kp2d::pack(&m, blob) != KP2D_OK) { std::printf("ERROR %s\n", g_err.c_str()); return 1; }
  if (blob.size() != m.blob_floats) return 5;
  f = std::fopen(argv[i++], "wb");
  if (!f || std::fwrite(blob.data(), sizeof(float), blob.size(), f) != blob.size()) return 6;
  std::fclose(f);
  return 0;
}
"""

# every get_config name x V2 / V3, then depth=True, to_mcu, to_export (remove_netvlad) and use_color=False; GeM and ConvAP are
# configurations of their own (GEM_N, GEM_S_A, CONVAP_S_A, D).  Keys as tools/plan_fingerprint.py model_matrix() writes them.
MODELS = ([(f"v2:{n}", n, False, {}) for n in orc.V2_CONFIGS] + [(f"v3:{n}", n, True, {}) for n in orc.V3_CONFIGS] +
          [("v2:S+depth", "S+depth", False, {}), ("v3:S_A+depth", "S_A+depth", True, {}), ("v2:S+mcu", "S+mcu", False, {}),
           ("v2:N_A+mcu+depth", "N_A+mcu+depth", False, {}), ("v3:S_A+mcu", "S_A+mcu", True, {}),
           ("v2:S+export", "S", False, {"remove_netvlad": True}), ("v3:S+gray", "S+gray", True, {})])

# Reference state-dict keys the engine does not consume: BatchNorm's step counter only (kp2d_set_weight accepts and drops it).
NOT_CONSUMED_SUFFIXES = (".num_batches_tracked",)


def _cfg(name, v3, extra):
    cfg = orc.get_config(name, v3)
    cfg.update(extra)
    return cfg


def _argv(cfg):
    gd = {"netvlad": 0, "gem": 1, "convap": 2}[cfg["global_descriptor_method"]]
    up = {"pixelshuffle": 0, "convtranspose": 1}[cfg["upscale_method"]]
    vals = [3 if cfg["v3"] else 2, *cfg["channel_dims"], cfg["nfeatures"], N_CLASSES, cfg["num_clusters"], cfg["encoder_dim"],
            cfg["downsample"], int(cfg["use_attention"]), int(cfg["leaky_relu"]), gd, int(cfg["remove_netvlad"]), int(cfg["depth"]),
            up, cfg["in_channels"]]
    return [str(int(v)) for v in vals]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    d = tmp_path_factory.mktemp("model_desc")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    # no ROCm include path: model_desc.cpp must stay free of HIP
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "driver.cpp"), os.path.join(CSRC, "model_desc.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def _describe(driver, cfg, extra=()):
    r = subprocess.run([driver, *_argv(cfg), *extra], check=True, capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("blob_floats "), r.stdout[-200:]
    specs = [(ln.split()[0], tuple(int(v) for v in ln.split()[1:])) for ln in lines[:-1]]
    return specs, int(lines[-1].split()[1])


@pytest.mark.parametrize("key,name,v3,extra", MODELS, ids=[m[0] for m in MODELS])
def test_described_tensors_are_the_reference_state_dict(driver, key, name, v3, extra):
    cfg = _cfg(name, v3, extra)
    ref = {k: tuple(s) for k, s in orc.state_dict_shapes(cfg, N_CLASSES).items()}
    specs, _ = _describe(driver, cfg)
    keys = [k for k, _ in specs]
    assert len(set(keys)) == len(keys), "describe() lists a key twice"
    for k, shape in specs:
        assert k in ref, f"{k}: not a reference state-dict key"
        assert ref[k] == shape, f"{k}: engine expects {shape}, the reference has {ref[k]}"
    left = sorted(set(ref) - set(keys))
    assert left and all(k.endswith(NOT_CONSUMED_SUFFIXES) for k in left), [k for k in left if not k.endswith(NOT_CONSUMED_SUFFIXES)]
    assert left == sorted(k for k in ref if k.endswith(NOT_CONSUMED_SUFFIXES))


@pytest.mark.parametrize("key,name,v3,extra", MODELS, ids=[m[0] for m in MODELS])
def test_pack_is_deterministic_and_sized_as_on_the_gpu(driver, tmp_path, key, name, v3, extra):
    cfg = _cfg(name, v3, extra)
    sd = spread_state_dict(orc.state_dict_shapes(cfg, N_CLASSES))
    specs, blob_floats = _describe(driver, cfg)
    with open(tmp_path / "w.bin", "wb") as f:
        for k, shape in specs:
            assert sd[k].dtype == np.float32 and tuple(sd[k].shape) == shape
            f.write(np.ascontiguousarray(sd[k]).tobytes())
    digests = []
    for i in range(2):
        out = tmp_path / f"blob{i}.bin"
        _describe(driver, cfg, (str(tmp_path / "w.bin"), str(out)))
        blob = out.read_bytes()
        assert len(blob) == 4 * blob_floats
        assert np.isfinite(np.frombuffer(blob, np.float32)[: 9 * cfg["in_channels"] * cfg["channel_dims"][0]]).all()
        digests.append(hashlib.sha256(blob).hexdigest())
    assert digests[0] == digests[1]
    with open(os.path.join(GOLDEN, "packed_bytes.json")) as f:
        recorded = json.load(f)      # kp2d_packed_bytes of a handle on the MI355X (tools/plan_fingerprint.py)
    assert 4 * blob_floats == recorded[key]
