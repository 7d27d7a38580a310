"""CPU unit test of nano-vs-slam_amd/csrc/lightglue_desc.cpp: which state-dict tensors the matcher consumes (names, shapes and
order against the state_dict of the LightGlue module built on the CPU), where every packed piece sits in the weight blob, and
what pack() writes there, element by element and bit by bit, against a numpy restatement written from the reference's
comments (lightglue.py:254-255 the Wqkv channel order, :389-390 final_proj / d^0.25, :395-396 the matchability logit) and
from the lane / element order documented above mfma_image.  The file is plain C++ and is compiled here with g++ together
with a small driver; no hipcc, no GPU."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import lightglue_fp64_ref as R
from conftest import GOLDEN, ROOT
from lightglue.lightglue import LightGlue
from lightglue.lightglue_configs import LIGHT_GLUE_CONFIGS

CSRC = os.path.join(ROOT, "nano-vs-slam_amd", "csrc")
ALIGN_FLOATS = 256 // 4       # api_common.h ALIGN, in floats

# argv: input_dim descriptor_dim n_layers num_heads, then any of: "ws B M N" | "drop KEY" | "pack weights.bin blob.bin"
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "lightglue_desc.h"
using namespace kp2d;
static std::string g_err;
namespace kp2d { void set_last_error(const char* msg) { g_err = msg ? msg : ""; } }
static void lin(const std::string& name, const Lin& l) {
  std::printf("lin %s %zu %zu %zu %d %d\n", name.c_str(), l.w, l.b, l.mf, l.K, l.nout);
}
static void vec(const std::string& name, size_t off, int n) { std::printf("vec %s %zu %d\n", name.c_str(), off, n); }
static void ffn(const std::string& name, const Ffn& f, int d) {
  lin(name + ".0", f.l0); vec(name + ".1.weight", f.g, 2 * d); vec(name + ".1.bias", f.be, 2 * d); lin(name + ".3", f.l3);
}
int main(int argc, char** argv) {
  if (argc < 5) return 2;
  LgDesc m;
  m.cfg.struct_size = (int32_t)sizeof(kp2d_lg_config);
  m.cfg.input_dim = atoi(argv[1]); m.cfg.descriptor_dim = atoi(argv[2]); m.cfg.n_layers = atoi(argv[3]); m.cfg.num_heads = atoi(argv[4]);
  if (describe(&m) != KP2D_OK) { std::printf("ERROR %s\n", g_err.c_str()); return 1; }
  const int d = m.cfg.descriptor_dim, n = m.cfg.n_layers;
  for (const auto& s : m.specs) {
    std::printf("spec %s", s.key.c_str());
    for (auto v : s.shape) std::printf(" %lld", (long long)v);
    std::printf("\n");
  }
  if (m.cfg.input_dim != d) lin("input_proj", m.input_proj);
  vec("posenc.Wr.weight", m.wr, d / m.cfg.num_heads);
  for (int i = 0; i < n; ++i) {
    const Layer& L = m.layers[i];
    const std::string s = "transformers." + std::to_string(i) + ".self_attn", c = "transformers." + std::to_string(i) + ".cross_attn";
    lin(s + ".Wqkv", L.qkv); lin(s + ".out_proj", L.out_proj); ffn(s + ".ffn", L.fs, d);
    lin(c + ".to_qk|to_v", L.qkv_x); lin(c + ".to_out", L.to_out); ffn(c + ".ffn", L.fc, d);
  }
  lin("final", m.final);
  for (int i = 0; i + 1 < n; ++i) vec("prune_w." + std::to_string(i), m.prune_w[i], d + 1);
  std::printf("blob_floats %zu\n", m.blob_floats);
  std::string drop;
  for (int i = 5; i < argc;) {
    if (!strcmp(argv[i], "ws") && i + 3 < argc) {
      const int B = atoi(argv[i + 1]), M = atoi(argv[i + 2]), N = atoi(argv[i + 3]);
      std::printf("ws %d %d %d %zu\n", B, M, N, layout(nullptr, &m, B, M, N).total);
      i += 4;
    } else if (!strcmp(argv[i], "drop") && i + 1 < argc) {
      drop = argv[i + 1];
      i += 2;
    } else if (!strcmp(argv[i], "pack") && i + 2 < argc) {
      FILE* f = std::fopen(argv[i + 1], "rb");      // the tensors of `specs`, in that order, float32
      if (!f) return 3;
      for (const auto& s : m.specs) {
        std::vector<float> v(s.numel());
        if (std::fread(v.data(), sizeof(float), v.size(), f) != v.size()) return 4;
        if (s.key != drop) m.host[s.key] = v;
      }
      std::fclose(f);
      std::vector<float> blob;
      if (pack(&m, blob) != KP2D_OK) { std::printf("ERROR %s\n", g_err.c_str()); return 1; }
      if (blob.size() != m.blob_floats) return 5;
      f = std::fopen(argv[i + 2], "wb");
      if (!f || std::fwrite(blob.data(), sizeof(float), blob.size(), f) != blob.size()) return 6;
      std::fclose(f);
      i += 3;
    } else {
      return 2;
    }
  }
  return 0;
}
"""

S, F = LIGHT_GLUE_CONFIGS["S"], LIGHT_GLUE_CONFIGS["F"]
CONFIGS = {
    "S": S,                                      # 32 -> 32, four layers
    "F": F,                                      # 64 -> 64: head dim 16, K = 128 in the ffn
    "input_proj": R.CASES["f"]["conf"],          # the input_proj configuration of the forms table: 64 -> 32, two layers
    "one_layer": dict(S, n_layers=1),            # no pruning layers, `final` directly after layer 0
}
WORKSPACE_CASES = {"a": "S", "c": "S", "e": "F", "f": "input_proj"}      # forms-table case -> configuration


def _module_conf(conf):
    """the configuration as the module holds it: num_heads is what lightglue.py hands kp2d_lg_create"""
    c = LightGlue(conf).conf
    return dict(input_dim=int(c.input_dim), descriptor_dim=int(c.descriptor_dim), n_layers=int(c.n_layers), num_heads=int(c.num_heads))


def _conf(name):
    return _module_conf(CONFIGS[name])


def _argv(conf):
    return [str(conf[k]) for k in ("input_dim", "descriptor_dim", "n_layers", "num_heads")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is required for the LightGlue description test")
    d = tmp_path_factory.mktemp("lightglue_desc")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    # no ROCm include path: lightglue_desc.cpp must stay free of HIP
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "driver.cpp"), os.path.join(CSRC, "lightglue_desc.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def _run(driver, conf, *extra):
    return subprocess.run([driver, *_argv(conf), *[str(e) for e in extra]], capture_output=True, text=True)


def _describe(driver, conf, *extra):
    r = _run(driver, conf, *extra)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:])
    rec = {"specs": [], "lin": {}, "vec": {}, "ws": {}}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "spec":
            rec["specs"].append((w[1], tuple(int(v) for v in w[2:])))
        elif w[0] == "lin":
            rec["lin"][w[1]] = dict(zip(("w", "b", "mf", "K", "nout"), (int(v) for v in w[2:])))
        elif w[0] == "vec":
            rec["vec"][w[1]] = (int(w[2]), int(w[3]))
        elif w[0] == "blob_floats":
            rec["blob_floats"] = int(w[1])
        elif w[0] == "ws":
            rec["ws"][tuple(int(v) for v in w[1:4])] = int(w[4])
    return rec


@pytest.fixture(scope="module")
def described(driver):
    return {name: _describe(driver, _conf(name)) for name in CONFIGS}


# ---------------------------------------------------------------------------------------------------------------------
# weights: seeded, magnitudes from 1e-6 to 10, and in one layer the values that walk every branch of f16_bits
# ---------------------------------------------------------------------------------------------------------------------
EDGE_LAYER = "transformers.0.self_attn.out_proj.weight"
EDGE_VALUES = [70000.0, -65520.0, 65519.996, 65504.0,                                    # inf, the first value that rounds to inf, the last that does not
               2.0 ** -14, 2.0 ** -14 - 2.0 ** -26, 2.0 ** -15, -3e-6, 1e-7,             # the smallest normal half, a subnormal that rounds up to it, subnormals
               2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -26, 0.0,                # the subnormal step, its tie (to even: 0), just above the tie, below
               1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11 + 2.0 ** -20)]    # ties to even both ways, just past a tie


def _weights(specs, seed=20240):
    g = np.random.default_rng(seed)
    sd = {k: (g.standard_normal(shape) * 10.0 ** g.uniform(-6.0, 1.0, shape)).astype(np.float32) for k, shape in specs}
    sd[EDGE_LAYER].reshape(-1)[:len(EDGE_VALUES)] = np.asarray(EDGE_VALUES, np.float32)
    return sd


def _pack(driver, conf, specs, sd, tmp, tag, *extra):
    with open(tmp / f"w_{tag}.bin", "wb") as f:
        for k, shape in specs:
            assert sd[k].dtype == np.float32 and tuple(sd[k].shape) == shape
            f.write(np.ascontiguousarray(sd[k]).tobytes())
    out = tmp / f"blob_{tag}.bin"
    r = _run(driver, conf, *extra, "pack", tmp / f"w_{tag}.bin", out)
    return r, out


# ---------------------------------------------------------------------------------------------------------------------
# the numpy restatement
# ---------------------------------------------------------------------------------------------------------------------
def linear_pieces(conf, sd):
    """{packed layer: (W^T [K, n], bias [n])}: the matrix the layer multiplies a row of activations by, its columns in the
    order the kernels read them."""
    d, din, n, h = conf["descriptor_dim"], conf["input_dim"], conf["n_layers"], conf["num_heads"]
    hd = d // h
    plain = lambda p: (sd[p + ".weight"].T, sd[p + ".bias"])
    join = lambda *ps: (np.concatenate([sd[p + ".weight"] for p in ps], 0).T, np.concatenate([sd[p + ".bias"] for p in ps]))
    out = {}
    if din != d:
        out["input_proj"] = plain("input_proj")
    for i in range(n):
        s, c = f"transformers.{i}.self_attn", f"transformers.{i}.cross_attn"
        # lightglue.py:254-255: qkv.unflatten(-1, (heads, -1, 3)), so Wqkv's output channel is (head, dim, q|k|v); the
        # kernels read [q | k | v], each of them head-major
        w = sd[s + ".Wqkv.weight"].reshape(h, hd, 3, d).transpose(2, 0, 1, 3).reshape(3 * d, d)
        b = sd[s + ".Wqkv.bias"].reshape(h, hd, 3).transpose(2, 0, 1).reshape(3 * d)
        out[s + ".Wqkv"] = (w.T, b)
        out[s + ".out_proj"] = plain(s + ".out_proj")
        out[s + ".ffn.0"], out[s + ".ffn.3"] = plain(s + ".ffn.0"), plain(s + ".ffn.3")
        out[c + ".to_qk|to_v"] = join(c + ".to_qk", c + ".to_v")          # one layer: columns [qk | v]
        out[c + ".to_out"] = plain(c + ".to_out")
        out[c + ".ffn.0"], out[c + ".ffn.3"] = plain(c + ".ffn.0"), plain(c + ".ffn.3")
    # the LAST layer's MatchAssignment: both descriptor sets are projected and divided by d^0.25 (lightglue.py:389-390), so
    # the factor sits in the weights and the bias; column d is the matchability logit (:395-396)
    a = f"log_assignment.{n - 1}"
    scale = np.float32(1) / np.power(np.float32(d), np.float32(0.25))
    assert scale.dtype == np.float32
    w = np.concatenate([sd[a + ".final_proj.weight"] * scale, sd[a + ".matchability.weight"]], 0)
    b = np.concatenate([sd[a + ".final_proj.bias"] * scale, sd[a + ".matchability.bias"]])
    out["final"] = (w.T, b)
    return out


def vector_pieces(conf, sd):
    """{piece: vector}: LayerNorm gains and biases, the positional encoding's Wr, the pruning layers' matchability."""
    out = {"posenc.Wr.weight": sd["posenc.Wr.weight"].reshape(-1)}
    for i in range(conf["n_layers"]):
        for blk in ("self_attn", "cross_attn"):
            for t in ("weight", "bias"):
                out[f"transformers.{i}.{blk}.ffn.1.{t}"] = sd[f"transformers.{i}.{blk}.ffn.1.{t}"]
    for i in range(conf["n_layers"] - 1):       # get_matchability of every layer but the last: the weight, its bias behind
        q = f"log_assignment.{i}.matchability"
        out[f"prune_w.{i}"] = np.concatenate([sd[q + ".weight"].reshape(-1), sd[q + ".bias"]])
    return out


def operand_image(wt):
    """W^T [K, nout] float32 as it sits in the blob -> uint16 [tile, k step, hi | lo, lane, 8]: per (16-feature tile t, 32-wide
    k step s) lane l holds feature 16 t + l % 16 and, with g = l // 16, its element j the input feature 32 s + 4 g + j
    (j < 4) or 32 s + 16 + 4 g + (j - 4)."""
    K, nout = wt.shape
    t, s, lane, j = np.meshgrid(np.arange(nout // 16), np.arange(K // 32), np.arange(64), np.arange(8), indexing="ij")
    g = lane // 16
    w = wt[32 * s + np.where(j < 4, 4 * g + j, 16 + 4 * g + (j - 4)), 16 * t + lane % 16]
    with np.errstate(over="ignore", invalid="ignore"):
        hi = w.astype(np.float16)
        lo = (w - hi.astype(np.float32)).astype(np.float16)
    return np.stack([hi, lo], axis=2).view(np.uint16)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_described_tensors_are_the_module_state_dict(described, name):
    want = [(k, tuple(v.shape)) for k, v in LightGlue(CONFIGS[name]).state_dict().items()]
    assert described[name]["specs"] == want
    assert (name == "input_proj") == (want[0][0] == "input_proj.weight")


def _pieces(rec):
    """[(name, offset, floats)] of everything describe() placed"""
    out = []
    for name, l in rec["lin"].items():
        out += [(name + " w", l["w"], l["K"] * l["nout"]), (name + " b", l["b"], l["nout"])]
        assert (l["mf"] != 0) == (l["K"] % 32 == 0), name
        if l["mf"]:
            out.append((name + " mf", l["mf"], l["K"] * l["nout"]))       # K * nout * 4 bytes of halves
    return out + [(name, off, n) for name, (off, n) in rec["vec"].items()]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_layout_is_aligned_disjoint_and_ends_at_blob_floats(described, name):
    rec, conf = described[name], _conf(name)
    d, din, n = conf["descriptor_dim"], conf["input_dim"], conf["n_layers"]
    want = {"final": (d, d + 1)}      # packed layer -> (K, valid columns)
    if din != d:
        want["input_proj"] = (din, d)
    for i in range(n):
        for blk, first, w3 in (("self_attn", "Wqkv", 3 * d), ("cross_attn", "to_qk|to_v", 2 * d)):
            p = f"transformers.{i}.{blk}"
            want[f"{p}.{first}"] = (d, w3)
            want[f"{p}.{'out_proj' if blk == 'self_attn' else 'to_out'}"] = (d, d)
            want[f"{p}.ffn.0"], want[f"{p}.ffn.3"] = (2 * d, 2 * d), (2 * d, d)
    assert {k: (l["K"], l["nout"]) for k, l in rec["lin"].items()} == {k: (K, -(-nv // 32) * 32) for k, (K, nv) in want.items()}
    assert len([k for k in rec["vec"] if k.startswith("prune_w.")]) == n - 1
    pieces = sorted(_pieces(rec), key=lambda p: p[1])
    assert all(off % ALIGN_FLOATS == 0 for _, off, _ in pieces), [p for p in pieces if p[1] % ALIGN_FLOATS]
    assert pieces[0][1] == 0
    for (na, oa, sa), (nb, ob, _) in zip(pieces, pieces[1:]):
        assert sa > 0 and oa + sa <= ob, f"{na} [{oa}, {oa + sa}) overlaps {nb} at {ob}"
    end = pieces[-1][1] + pieces[-1][2]
    assert rec["blob_floats"] == -(-end // ALIGN_FLOATS) * ALIGN_FLOATS      # the end of the last piece, on the alignment
    if n > 1:      # the pruning vectors are appended: `final` sits where it sat before they existed
        assert pieces[-1][0] == f"prune_w.{n - 2}" and rec["vec"]["prune_w.0"][0] > rec["lin"]["final"]["mf"]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_packed_contents_and_operand_images(driver, described, tmp_path, name):
    rec, conf = described[name], _conf(name)
    sd = _weights(rec["specs"])
    assert np.abs(sd[EDGE_LAYER]).max() >= 65520 and (np.abs(sd[EDGE_LAYER][sd[EDGE_LAYER] != 0]) < 2.0 ** -14).any()
    digests = []
    for i in range(2):
        r, out = _pack(driver, conf, rec["specs"], sd, tmp_path, str(i))
        assert r.returncode == 0, (r.returncode, r.stdout[-300:])
        digests.append(hashlib.sha256(out.read_bytes()).hexdigest())
    assert digests[0] == digests[1]
    blob = np.fromfile(out, np.float32)
    assert blob.size == rec["blob_floats"]
    want = np.zeros_like(blob)      # everything that is not a piece, and every padded column, is zero
    lins, vecs = linear_pieces(conf, sd), vector_pieces(conf, sd)
    assert set(lins) == set(rec["lin"]) and set(vecs) == set(rec["vec"])
    for k, (wt, b) in lins.items():
        l = rec["lin"][k]
        assert wt.dtype == np.float32 and wt.shape[0] == l["K"] and wt.shape[1] == b.shape[0] <= l["nout"]
        m = np.zeros((l["K"], l["nout"]), np.float32)
        m[:, :wt.shape[1]] = wt
        want[l["w"]:l["w"] + m.size] = m.reshape(-1)
        want[l["b"]:l["b"] + b.size] = b
        got = blob[l["w"]:l["w"] + m.size].reshape(m.shape)
        assert np.array_equal(bits(got), bits(m)), f"{k}: W^T differs at {np.argwhere(bits(got) != bits(m))[:4].tolist()}"
        assert np.array_equal(bits(blob[l["b"]:l["b"] + l["nout"]]), bits(want[l["b"]:l["b"] + l["nout"]])), f"{k}: bias"
        # the operand images of every layer a tail kernel may run (K % 32 == 0 always holds there); input_proj only ever
        # runs as lg_linear on the fp32 matrix, and its image space stays reserved and zero
        if l["mf"] and k != "input_proj":
            img = operand_image(m)
            assert img.size == 2 * m.size
            got16 = blob[l["mf"]:l["mf"] + m.size].view(np.uint16).reshape(img.shape)
            assert np.array_equal(got16, img), f"{k}: operand image differs at (tile, k step, hi|lo, lane, j) {np.argwhere(got16 != img)[:4].tolist()}"
            want[l["mf"]:l["mf"] + m.size] = img.reshape(-1).view(np.float32)
    for k, v in vecs.items():
        off, nv = rec["vec"][k]
        assert v.dtype == np.float32 and v.shape == (nv,), k
        assert np.array_equal(bits(blob[off:off + nv]), bits(v)), k
        want[off:off + nv] = v
    assert np.array_equal(bits(blob), bits(want))
    if name == "S":      # the edge values reached both halves: an infinite hi with an infinite lo, subnormal halves
        l = rec["lin"]["transformers.0.self_attn.out_proj"]
        img = blob[l["mf"]:l["mf"] + l["K"] * l["nout"]].view(np.uint16).reshape(l["nout"] // 16, l["K"] // 32, 2, 64, 8)
        assert (img[:, :, 0] == 0x7c00).any() and (img[:, :, 1] == 0xfc00).any() and (img[:, :, 0] == 0x0001).any()
        assert ((img & 0x7c00) == 0).any() and (img[:, :, 0] == 0x0400).sum() >= 2


def test_missing_tensor_is_refused(driver, described, tmp_path):
    rec, conf = described["input_proj"], _conf("input_proj")
    sd = _weights(rec["specs"])
    for key in ("input_proj.bias", "posenc.Wr.weight", "token_confidence.0.token.0.weight"):
        r, out = _pack(driver, conf, rec["specs"], sd, tmp_path, "m", "drop", key)
        assert r.returncode == 1 and r.stdout.splitlines()[-1] == f"ERROR missing tensor '{key}'"
        assert not out.exists()


@pytest.mark.parametrize("change,message", [
    (dict(descriptor_dim=48), "descriptor_dim=48 (32 and 64 are built)"),
    (dict(descriptor_dim=16), "descriptor_dim=16 (32 and 64 are built)"),
    (dict(descriptor_dim=96), "descriptor_dim=96 (32 and 64 are built)"),
    (dict(descriptor_dim=0), "descriptor_dim=0 (32 and 64 are built)"),
    (dict(num_heads=0), "num_heads=0: head dim must be a multiple of 4, <= 16"),
    (dict(num_heads=3), "num_heads=3: head dim must be a multiple of 4, <= 16"),
    (dict(num_heads=16), "num_heads=16: head dim must be a multiple of 4, <= 16"),
    (dict(descriptor_dim=64, num_heads=2), "num_heads=2: head dim must be a multiple of 4, <= 16"),
    (dict(input_dim=0), "input_dim=0 (<= 128)"),
    (dict(input_dim=129), "input_dim=129 (<= 128)"),
    (dict(n_layers=0), "n_layers=0"),
    (dict(n_layers=33), "n_layers=33"),
])
def test_unbuilt_configurations_are_refused(driver, change, message):
    r = _run(driver, dict(_conf("S"), **change))
    assert r.returncode == 1 and r.stdout.strip() == "ERROR " + message


def test_accepted_edges_of_the_configuration(driver):
    for change in (dict(input_dim=128), dict(input_dim=1), dict(n_layers=32), dict(descriptor_dim=64, num_heads=16), dict(num_heads=2)):
        assert _run(driver, dict(_conf("S"), **change)).returncode == 0, change


def test_workspace_bytes_are_those_of_the_device_library(driver):
    """tests/golden/lg_workspace_bytes.json holds what kp2d_lg_workspace_bytes of a handle on the MI355X answered for the
    (B, M, N) of forms-table cases a, c, e, f, recorded from the commit BEFORE the workspace walk moved out of
    lightglue_api.cpp (LightGlue(conf).workspace_bytes(B, M, N, "cuda:0") per case); the walk is host arithmetic, and the
    same walk compiled here must give the same sizes."""
    with open(os.path.join(GOLDEN, "lg_workspace_bytes.json")) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted(WORKSPACE_CASES)
    for case, name in WORKSPACE_CASES.items():
        c = R.CASES[case]
        assert _module_conf(R.conf_in(case)) == _conf(name)
        shape = (c["B"], c["M"], c["N"])
        assert _describe(driver, _conf(name), "ws", *shape)["ws"][shape] == recorded[case], case
