"""LightGlue point pruning on the device (kp2d_lg_forward_pruned, width_confidence > 0) against the float64 restatement in
tests/lightglue_prune_ref.py.  Parity unpinned, as every LightGlue test: the oracle restates lightglue.py.

One flipped prune decision changes every later descriptor, so there is no per-point exemption: every case must have an
oracle MARGIN (smallest |score - (1 - width_confidence)| over all decisions) of at least 1e-3 — about ten times what the
2e-4 descriptor tolerance of tests/test_lightglue_gpu.py admits on a matchability logit — and the tests assert that on the
oracle before they compare anything.  Observed on an MI355X over the eight parity cases: max |s_device - s_oracle| of the
survivors' last-layer matchability scores (read back from the dustbin column) 3e-7 to 2.7e-6, every decision equal."""
import functools

import numpy as np
import pytest
import torch

import lightglue_prune_ref as ref
from oracle import lightglue_oracle as lg
from test_lightglue_gpu import product, to_dev
from test_lightglue_oracle import make_data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1e-3

# (M, N, seed, width_confidence, filter_threshold): oracle margin / survivors measured with the float64 oracle.
# filter_threshold = 0 keeps every mutual pair, but the seeded weights give some matching scores below 1e-4, which the
# existing threshold rule exempts (a score within 1e-4 of the threshold): on the oracle alone 3 of 52, 5 of 53, 4 of 142
# and 14 of 249 survivors below — and 3 of 9 for (33, 64, 5), which therefore runs at 0.1 (0 exempted, as every 0.1 case).
CASES_S = [(70, 45, 11, 0.6, 0.1),        # 2.6e-3, 38 / 2
           (70, 45, 3, 0.6, 0.0),         # 1.6e-3, 52 / 19, 5 matches at threshold 0
           (128, 128, 3, 0.6, 0.0),       # 1.3e-3, 53 / 24, 10 matches (M == N: both sets in one attention launch)
           (33, 64, 5, 0.55, 0.1),        # 2.3e-3, 9 / 39
           # more than one 256-row chunk per sequence in the compaction walk
           (260, 40, 4, 0.6, 0.0),        # 3.3e-3, 142 / 11: 260 -> 244 -> 202 -> 142, the first walk has a 4-row second chunk
           (300, 257, 5, 0.7, 0.0)]       # 1.7e-3, 249 / 198: set 0 walks two chunks after every layer, set 1 after the first
CASES_F = [(96, 50, 1, 0.85, 0.0),        # 2.7e-3, 26 / 14 (D = 64: lg_linear projections, the 64-wide compaction)
           (70, 45, 3, 0.8, 0.0)]         # 1.4e-3, 14 / 3, points dropped after each of the three layers
# threshold 0 and at least five oracle matches among the survivors
MIN_MATCHES = {("S", 70, 45, 3), ("S", 128, 128, 3), ("S", 260, 40, 4), ("S", 300, 257, 5)}


@functools.lru_cache(maxsize=None)
def setup(name, M, N, seed, wc, th):
    """(conf_in, conf, weights, float32 data, float64 oracle result or None where the oracle cannot run)"""
    from lightglue.lightglue_configs import get_light_glue_config
    conf_in = dict(get_light_glue_config(name), filter_threshold=th, width_confidence=wc)
    conf = lg.get_config(conf_in)
    sd = lg.seeded_state_dict(conf)
    data = make_data(1, M, N, conf["input_dim"], seed=seed)
    p64 = {k: v.astype(np.float64) for k, v in sd.items()}
    d64 = {k: ({"image_size": v["image_size"].astype(np.float64)} if isinstance(v, dict) else v.astype(np.float64))
           for k, v in data.items()}
    try:
        want = ref.forward_pruned(d64, p64, conf, wc)
    except ValueError:
        want = None
    return conf_in, conf, sd, data, want


@functools.lru_cache(maxsize=None)
def model_for(name, wc, th):
    from lightglue.lightglue_configs import get_light_glue_config
    conf_in = dict(get_light_glue_config(name), filter_threshold=th, width_confidence=wc)
    return product(conf_in, lg.seeded_state_dict(lg.get_config(conf_in)))


def run(model, data):
    with torch.no_grad():
        pred = model(data)
    return {k: v.cpu().numpy() for k, v in pred.items()}


def check_pruned(got, want, conf, th, min_matches=0):
    assert want["margin"] >= MARGIN, want["margin"]           # the condition under which decisions can be compared at all
    B, M = got["matches0"].shape
    N = got["matches1"].shape[1]
    for k in ("keep0", "keep1", "num_kept0", "num_kept1", "prune0", "prune1"):
        assert np.array_equal(got[k], want[k]), k
    assert got["prune0"].dtype == np.int64 and got["keep0"].dtype == np.int32
    exempt = total = 0
    for b in range(B):
        m, n = int(want["num_kept0"][b]), int(want["num_kept1"][b])
        la, rla = got["log_assignment"][b], want["log_assignment"][b]
        for a, r in ((la[:m, :n], rla[:m, :n]), (la[:m, N], rla[:m, N]), (la[M, :n], rla[M, :n])):
            assert np.max(np.abs(a - r) / (1.0 + np.abs(r))) < 5e-5
        assert np.all(np.isneginf(la[:M, :N][m:])) and np.all(np.isneginf(la[:M, :N][:, n:]))
        # the device's matchability scores of the survivors at the last layer (dustbin column = log(1 - s))
        s_dev, s_ref = 1.0 - np.exp(la[:m, N].astype(np.float64)), 1.0 - np.exp(rla[:m, N])
        print(f"pair {b}: margin {want['margin']:.2e}, survivors {m} / {n}, max |s_device - s_oracle| (last layer, set 0) "
              f"{np.max(np.abs(s_dev - s_ref)):.2e}")
        for k, c in (("ref_descriptors0", m), ("ref_descriptors1", n)):
            r = want[k][b, 0, :c]
            assert np.max(np.abs(got[k][b, 0, :c] - r)) < 2e-4 * max(1.0, float(np.abs(r).max()))
        # matches: identical wherever the oracle's decision is not within rounding of a tie / of the threshold
        # (the rule of tests/test_lightglue_gpu.py::check, on the survivors' block)
        inner = rla[:m, :n]
        i0, i1 = want["keep0"][b, :m], want["keep1"][b, :n]
        rs0 = want["matching_scores0"][b][i0]
        ok = ~((np.abs(rs0 - th) < 1e-4) & (rs0 > 0))
        if n > 1:
            top2 = np.sort(inner, axis=1)[:, -2:]
            ok &= (top2[:, 1] - top2[:, 0]) > 1e-3
        if m > 1:
            top2c = np.sort(inner, axis=0)[-2:, :]
            ok &= ((top2c[1] - top2c[0]) > 1e-3)[inner.argmax(1)]
        exempt += int((~ok).sum())
        total += m
        m0, s0 = got["matches0"][b], got["matching_scores0"][b]
        assert np.array_equal(m0[i0][ok], want["matches0"][b][i0][ok])
        assert np.max(np.abs(s0[i0][ok] - rs0[ok]), initial=0.0) < 1e-4
        dropped0, dropped1 = np.ones(M, bool), np.ones(N, bool)
        dropped0[i0], dropped1[i1] = False, False
        m1, s1 = got["matches1"][b], got["matching_scores1"][b]
        assert np.all(m0[dropped0] == -1) and np.all(s0[dropped0] == 0) and np.all(m1[dropped1] == -1) and np.all(s1[dropped1] == 0)
        assert (m1 == want["matches1"][b]).mean() > 0.97
        on = np.nonzero(m0 >= 0)[0]                               # the product's own outputs: mutual and one-to-one
        assert np.array_equal(m1[m0[on]], on) and len(set(m0[on].tolist())) == len(on)
        assert int((want["matches0"][b] >= 0).sum()) >= min_matches
    assert exempt <= 0.1 * total, (exempt, total)
    print(f"exempted by the tie / threshold rule: {exempt} of {total}")


def _parity(name, M, N, seed, wc, th):
    conf_in, conf, sd, data, want = setup(name, M, N, seed, wc, th)
    assert want is not None and want["margin"] >= MARGIN
    got = run(model_for(name, wc, th), to_dev(data))
    check_pruned(got, want, conf, th, 5 if (name, M, N, seed) in MIN_MATCHES else 0)


@pytest.mark.parametrize("M,N,seed,wc,th", CASES_S)
def test_pruned_forward_matches_oracle_config_s(M, N, seed, wc, th):
    """B = 1, D = 32: the fused path (tail kernel without its next projection, lg_prune, projection-only tail)."""
    _parity("S", M, N, seed, wc, th)


@pytest.mark.parametrize("M,N,seed,wc,th", CASES_F)
def test_pruned_forward_matches_oracle_config_f(M, N, seed, wc, th):
    """B = 1, D = 64: the unfused path (lg_linear projections around lg_prune)."""
    _parity("F", M, N, seed, wc, th)


def padded_batch(cases, M, N, wc, th):
    """The B = 1 inputs of `cases` in one batch of capacity M x N: garbage in the padding rows, num_keypoints0/1 set."""
    rng = np.random.default_rng(17)
    din = 32
    out = {"keypoints0": (rng.random((len(cases), M, 2)) * 300).astype(np.float32),
           "keypoints1": (rng.random((len(cases), N, 2)) * 300).astype(np.float32),
           "descriptors0": rng.standard_normal((len(cases), M, din)).astype(np.float32),
           "descriptors1": rng.standard_normal((len(cases), N, din)).astype(np.float32)}
    sizes = []
    for b, (m, n, seed) in enumerate(cases):
        data = setup("S", m, n, seed, wc, th)[3]
        out["keypoints0"][b, :m], out["keypoints1"][b, :n] = data["keypoints0"][0], data["keypoints1"][0]
        out["descriptors0"][b, :m], out["descriptors1"][b, :n] = data["descriptors0"][0], data["descriptors1"][0]
        sizes.append(data["view0"]["image_size"][0])
    out["view0"] = {"image_size": np.stack(sizes)}
    out["view1"] = {"image_size": np.stack(sizes)}
    dd = to_dev(out)
    dd["num_keypoints0"] = torch.tensor([c[0] for c in cases], dtype=torch.int32, device=DEV)
    dd["num_keypoints1"] = torch.tensor([c[1] for c in cases], dtype=torch.int32, device=DEV)
    return dd


def assert_pair_equals_single(got, b, one, m, n, exact_floats=False):
    """Pair b of a padded batch against the B = 1 run of its m x n rows: decisions exactly, floats to the summation-order
    tolerance of the padded-set test (5e-5 relative on the assignment, 2e-4 on the descriptors)."""
    M, N = got["matches0"].shape[1], got["matches1"].shape[1]
    km, kn = int(one["num_kept0"][0]), int(one["num_kept1"][0])
    assert got["num_kept0"][b] == km and got["num_kept1"][b] == kn
    assert np.array_equal(got["keep0"][b, :m], one["keep0"][0]) and np.all(got["keep0"][b, m:] == -1)
    assert np.array_equal(got["keep1"][b, :n], one["keep1"][0]) and np.all(got["keep1"][b, n:] == -1)
    assert np.array_equal(got["prune0"][b, :m], one["prune0"][0]) and np.all(got["prune0"][b, m:] == 0)
    assert np.array_equal(got["prune1"][b, :n], one["prune1"][0]) and np.all(got["prune1"][b, n:] == 0)
    assert np.array_equal(got["matches0"][b, :m], one["matches0"][0]) and np.all(got["matches0"][b, m:] == -1)
    assert np.array_equal(got["matches1"][b, :n], one["matches1"][0]) and np.all(got["matches1"][b, n:] == -1)
    assert np.all(got["matching_scores0"][b, m:] == 0) and np.all(got["matching_scores1"][b, n:] == 0)
    pairs = [(got["matching_scores0"][b, :m], one["matching_scores0"][0]), (got["matching_scores1"][b, :n], one["matching_scores1"][0]),
             (got["log_assignment"][b, :km, :kn], one["log_assignment"][0, :km, :kn]),
             (got["log_assignment"][b, :km, N], one["log_assignment"][0, :km, n]),
             (got["log_assignment"][b, M, :kn], one["log_assignment"][0, m, :kn]),
             (got["ref_descriptors0"][b, 0, :km], one["ref_descriptors0"][0, 0, :km]),
             (got["ref_descriptors1"][b, 0, :kn], one["ref_descriptors1"][0, 0, :kn])]
    for i, (a, r) in enumerate(pairs):
        assert np.all(np.isfinite(a))
        if exact_floats:
            assert np.array_equal(a, r), i
        elif i < 2:
            assert np.max(np.abs(a - r), initial=0.0) < 1e-4
        elif i < 5:
            assert np.max(np.abs(a - r) / (1.0 + np.abs(r)), initial=0.0) < 5e-5
        else:
            assert np.max(np.abs(a - r)) < 2e-4 * max(1.0, float(np.abs(r).max()))


def test_batch_of_padded_pairs_equals_the_single_pairs():
    """B = 3, padded to 128 x 128 with num_keypoints0/1: every pair is pruned on its own and equals its B = 1 run."""
    wc, th = 0.6, 0.0
    cases = [(70, 45, 11), (70, 45, 3), (128, 128, 3)]
    for m, n, seed in cases:
        assert setup("S", m, n, seed, wc, th)[4]["margin"] >= MARGIN
    model = model_for("S", wc, th)
    got = run(model, padded_batch(cases, 128, 128, wc, th))
    for b, (m, n, seed) in enumerate(cases):
        one = run(model, to_dev(setup("S", m, n, seed, wc, th)[3]))
        assert_pair_equals_single(got, b, one, m, n)
        want = setup("S", m, n, seed, wc, th)[4]
        assert np.array_equal(got["keep0"][b, :m], want["keep0"][0]) and np.array_equal(got["prune1"][b, :n], want["prune1"][0])


def test_pair_that_becomes_empty_stays_unmatched_and_alone():
    """(1, 40, seed 5, wc 0.6): the single point of set 0 is pruned after the second layer (float64 oracle scores 0.449 and
    0.364 against 0.4), every later attention of the pair has zero keys (NaN rows, an ordinary input of the counts path)
    and the oracle formulation cannot go on.  Beside
    a normal pair in one batch: the empty pair is unmatched, the normal pair is its B = 1 run."""
    wc, th = 0.6, 0.0
    assert setup("S", 1, 40, 5, wc, th)[4] is None                      # the oracle fails on the empty set
    assert setup("S", 70, 45, 3, wc, th)[4]["margin"] >= MARGIN
    model = model_for("S", wc, th)
    got = run(model, padded_batch([(1, 40, 5), (70, 45, 3)], 70, 45, wc, th))
    assert np.all(got["matches0"][0] == -1) and np.all(got["matches1"][0] == -1)
    assert np.all(got["matching_scores0"][0] == 0) and np.all(got["matching_scores1"][0] == 0)
    assert got["num_kept0"][0] == 0 and got["prune0"][0, 0] == 2 and np.all(got["prune0"][0, 1:] == 0)
    one = run(model, to_dev(setup("S", 70, 45, 3, wc, th)[3]))
    assert_pair_equals_single(got, 1, one, 70, 45, exact_floats=True)


def test_nothing_pruned_equals_the_unpruned_entry_point():
    """width_confidence = 0.95 prunes nothing with the seeded S weights (every score > 0.05, tests/test_lightglue_prune_cpu.py):
    the results are those of width_confidence = -1 on the same input."""
    M, N, seed, th = 70, 45, 11, 0.1
    data = to_dev(setup("S", M, N, seed, 0.6, th)[3])
    a, b = run(model_for("S", 0.95, th), data), run(model_for("S", -1, th), data)
    assert np.all(a["prune0"] == 4) and np.all(a["prune1"] == 4) and a["prune0"].dtype == np.int64
    assert np.array_equal(a["keep0"][0], np.arange(M)) and a["num_kept1"][0] == N
    assert np.array_equal(a["matches0"], b["matches0"]) and np.array_equal(a["matches1"], b["matches1"])
    assert np.max(np.abs(a["matching_scores0"] - b["matching_scores0"])) < 1e-6
    assert np.max(np.abs(a["log_assignment"] - b["log_assignment"]) / (1.0 + np.abs(b["log_assignment"]))) < 5e-5
    assert np.max(np.abs(a["ref_descriptors0"] - b["ref_descriptors0"])) < 2e-4


@pytest.mark.parametrize("wc", [0.6, 0.9])
def test_frame_stream_replays_the_pruned_matcher(wc):
    """FrameStream(match="lightglue") with a pruning matcher: the captured and replayed forward gives the matched rows of
    the eager call on the same selections (the slots' static rows; three frames in three slots: none is overwritten).
    (Seeded random weights on the extractor's descriptors: 0.6 prunes every point of these frames.)"""
    from conftest import product_model
    from nano_vs_slam_amd.matching import match_topk_pairs
    from nano_vs_slam_amd.pipeline import FrameStream
    from test_gpu_parity import _vo_frames
    net, _ = product_model("S", False, 28)
    lgm = model_for("S", wc, 0.0)
    H, W = 96, 128
    frames = _vo_frames(3, np.random.default_rng(6), (H, W))
    fs = FrameStream(net, (H, W), None, nn_thresh=0.5, top_k=200, device=DEV, slots=3, match="lightglue", matcher=lgm)
    got = list(fs.map(frames))
    assert got[0][0].shape == (0, 2)
    scale = fs.scale if fs.scale is not None else 1.0
    for i in (1, 2):
        k0, k1, sc, out = got[i]
        rp, rc = got[i - 1][3]["rows"], out["rows"]
        data = {"keypoints0": rp["pts"] * scale / fs._lg_wh, "keypoints1": rc["pts"] * scale / fs._lg_wh,
                "descriptors0": rp["desc"], "descriptors1": rc["desc"],
                "view0": {"image_size": fs._lg_size}, "view1": {"image_size": fs._lg_size},
                "num_keypoints0": rp["cnt"], "num_keypoints1": rc["cnt"]}
        with torch.no_grad():
            eager = lgm(data)
        torch.cuda.synchronize()
        for k in ("matches0", "matches1", "matching_scores0", "keep0", "keep1", "num_kept0", "num_kept1", "prune0", "prune1"):
            assert torch.equal(eager[k], out["match"][k]), (i, k)
        po = match_topk_pairs(0, rp["pts"], rc["pts"], matches0=eager["matches0"], scores0=eager["matching_scores0"])
        cnt = int(po["count"][0])
        pr = po["pairs"][0, :cnt].cpu().numpy()
        assert cnt == len(sc) and np.array_equal(pr[:, :2], k0) and np.array_equal(pr[:, 2:], k1)
        print(f"frame {i}: {int(rp['cnt'][0])} / {int(rc['cnt'][0])} keypoints, {int(eager['num_kept0'][0])} / "
              f"{int(eager['num_kept1'][0])} survivors, {cnt} matches")
        assert int(eager["num_kept0"][0]) <= int(rp["cnt"][0]) and int(eager["prune0"].max()) <= 4


def test_refusals():
    from lightglue.lightglue import LightGlue
    from nano_vs_slam_amd import _dev, _lib
    from nano_vs_slam_amd._dev import ptr as P
    conf_in, conf, sd, data, _ = setup("S", 70, 45, 11, 0.6, 0.1)
    dd = to_dev(data)
    with pytest.raises(NotImplementedError):
        product(dict(conf_in, depth_confidence=0.9), sd)(dd)
    model = model_for("S", 0.6, 0.1)
    lib, h = model._engine(torch.device(DEV))
    B, M, N, d = 1, 70, 45, 32
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=DEV)
    o = {"la": z(B, M + 1, N + 1), "m0": z(B, M, dtype=torch.int64), "m1": z(B, N, dtype=torch.int64), "s0": z(B, M), "s1": z(B, N),
         "k0": z(B, M, dtype=torch.int32), "k1": z(B, N, dtype=torch.int32), "n0": z(B, dtype=torch.int32), "n1": z(B, dtype=torch.int32),
         "p0": z(B, M, dtype=torch.int64), "p1": z(B, N, dtype=torch.int64)}
    need, plain = int(lib.kp2d_lg_workspace_bytes_pruned(h, B, M, N)), int(lib.kp2d_lg_workspace_bytes(h, B, M, N))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(wc, nbytes, k0="k0"):
        return lib.kp2d_lg_forward_pruned(h, P(dd["keypoints0"]), P(dd["keypoints1"]), P(dd["descriptors0"]), P(dd["descriptors1"]),
                                          None, None, None, None, B, M, N, 0.1, wc, P(o["la"]), P(o["m0"]), P(o["m1"]), P(o["s0"]),
                                          P(o["s1"]), None, None, P(o[k0]) if k0 else None, P(o["k1"]), P(o["n0"]), P(o["n1"]),
                                          P(o["p0"]), P(o["p1"]), P(ws), nbytes, _dev.stream(torch.device(DEV)))

    assert call(1.5, need) == -1 and call(0.0, need) == -1 and call(float("nan"), need) == -1      # KP2D_ERR_ARG
    assert call(0.6, need, k0=None) == -1                                                          # a null output
    assert need >= plain
    assert call(0.6, need - 256) == -5                                                             # KP2D_ERR_WORKSPACE
    if plain < need:
        assert call(0.6, plain) == -5
    assert call(0.6, need) == 0 and call(1.0, need) == 0
    torch.cuda.synchronize()
    assert int(o["n0"][0]) == 70 and int(o["p0"].min()) == 4            # width_confidence = 1: score > 0 keeps every point
