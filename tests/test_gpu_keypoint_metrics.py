"""Keypoint scores (csrc/keypoint_metrics.hip, nano_vs_slam_amd.keypoint_metrics) on the MI355X against the float64 oracle of
tests/keypoint_ref.py and the reference's own outputs (tests/golden/keypoints/rep_*.npz): every count exactly, the two
distance sums to 1e-9 absolute (include/kp2d.h derives the bound: n <= 1000 float64 terms, each <= distance_thresh, so any
order of summation is within n^2 eps distance_thresh = 3e-10), the bit identities, the tie rule, the empty cases, the Python
surface, and evaluate_keypoint_net end to end on the model's own outputs.  The generator's margins (no decision within 1e-6 of
its threshold, every nearest descriptor clear by 1e-3) give every count one right answer."""
import functools
import glob
import math
import os

import numpy as np
import pytest
import torch

import keypoint_ref as kr
from conftest import GOLDEN, product_model
from nano_vs_slam_amd import _lib
from nano_vs_slam_amd import keypoint_metrics as km

pytestmark = pytest.mark.gpu
LE_TOL = 1e-9
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "keypoints", "rep_*.npz")))
# name -> (k0, k1, C, image_shape, keep_k below and above the surviving counts); three pairs with different counts per batch.
# 37 / 53 rows and >= 256 rows: both forms of the matcher (VALU, and matrix core from 256 train rows)
BATCHES = {
    "0x40": (0, 40, 32, (240, 320), (7, 300)),
    "40x0": (40, 0, 64, (240, 320), (7, 300)),
    "1x1": (1, 1, 128, (240, 320), (1, 300)),
    "37x53": (37, 53, 32, (240, 320), (10, 300)),
    "37x53_odd_box": (37, 53, 64, (37, 53), (10, 300)),
    "37x53_C128": (37, 53, 128, (240, 320), (10, 300)),
    "300x257": (300, 257, 64, (240, 320), (100, 1000)),
    "300x257_odd_box": (300, 257, 32, (37, 53), (100, 1000)),
    "300x257_C128": (300, 257, 128, (240, 320), (256, 300)),
    "1000x1000": (1000, 1000, 32, (240, 320), (300, 2000)),
}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # a copy: the shared inputs are read-only


def bits(t):
    return t.cpu().numpy().view(np.int64)


@functools.lru_cache(maxsize=None)
def batch(name, ties=False):
    """Three pairs of (k0, k1), 2/3 and 1/3 of it rows, padded to [3, k, .]: the padding rows carry the highest probability
    and points inside the box, so reading one would show.  -> (cases, arrays); computed once and left unchanged."""
    k0, k1, C, shape, keep_ks = BATCHES[name]
    seed = sorted(BATCHES).index(name) * 10 + (500 if ties else 0)
    counts = [(k0, k1), ((2 * k0 + 2) // 3, (2 * k1 + 2) // 3), (k0 // 3, (k1 + 2) // 3)]
    cases = [kr.make_case(seed + i, n0, n1, C, shape, keep_ks, ties=ties) for i, (n0, n1) in enumerate(counts)]
    rng = np.random.default_rng(seed)
    arr = {"pts0": np.empty((3, k0, 3), np.float32), "pts1": np.empty((3, k1, 3), np.float32),
           "desc0": kr._unit(rng.standard_normal((3, k0, C))).astype(np.float32),
           "desc1": kr._unit(rng.standard_normal((3, k1, C))).astype(np.float32)}
    for key, k in (("pts0", k0), ("pts1", k1)):
        arr[key][:] = np.concatenate([rng.uniform(0.3, 0.7, (3, k, 2)) * shape, np.full((3, k, 1), 2.0)], 2)
    for i, c in enumerate(cases):
        n0, n1 = counts[i]
        arr["pts0"][i, :n0], arr["pts1"][i, :n1] = c["prob"], c["warped_prob"]
        arr["desc0"][i, :n0], arr["desc1"][i, :n1] = c["desc"], c["warped_desc"]
    arr["cnt0"] = np.array([c[0] for c in counts], np.int32)
    arr["cnt1"] = np.array([c[1] for c in counts], np.int32)
    arr["hom"] = np.stack([c["homography"] for c in cases])
    for a in arr.values():
        a.setflags(write=False)
    return cases, arr


def run_rep(arr, shape, keep_k, thresh=3, rows=slice(None)):
    return km.repeatability_stats(dev(arr["pts0"][rows]), dev(arr["cnt0"][rows]), dev(arr["pts1"][rows]), dev(arr["cnt1"][rows]),
                                  dev(arr["hom"][rows]), shape, keep_k, thresh)


def run_ms(arr, shape, keep_k, rows=slice(None)):
    return km.matching_score_stats(dev(arr["pts0"][rows]), dev(arr["cnt0"][rows]), dev(arr["desc0"][rows]), dev(arr["pts1"][rows]),
                                   dev(arr["cnt1"][rows]), dev(arr["desc1"][rows]), dev(arr["hom"][rows]), shape, keep_k)


def check_batch(name, ties=False):
    cases, arr = batch(name, ties)
    shape, keep_ks = BATCHES[name][3], BATCHES[name][4]
    for keep_k in keep_ks:
        counts, le = run_rep(arr, shape, keep_k)
        ms = run_ms(arr, shape, keep_k)
        assert counts.dtype == torch.int64 and le.dtype == torch.float64 and ms.dtype == torch.int64
        assert tuple(counts.shape) == (3, 4) and tuple(le.shape) == (3, 2) and tuple(ms.shape) == (3, 4)
        counts, le, ms = counts.cpu().numpy(), le.cpu().numpy(), ms.cpu().numpy()
        assert np.all(np.isfinite(le))
        for i, c in enumerate(cases):
            want = kr.repeatability_stats(c["prob"], c["warped_prob"], c["homography"], shape, keep_k)
            wm = kr.matching_score_stats(c["prob"], c["warped_prob"], c["desc"], c["warped_desc"], c["homography"], shape, keep_k)
            assert kr.margins_hold(want) and kr.margins_hold(wm)
            print(f"{name} keep_k {keep_k} pair {i}: counts {counts[i].tolist()} le {le[i].tolist()} against "
                  f"{[want[k] for k in ('N1', 'N2', 'count1', 'count2', 'le1', 'le2')]}; ms {ms[i].tolist()} against "
                  f"{[wm[k] for k in ('vis1', 'hit1', 'vis2', 'hit2')]}")
            assert counts[i].tolist() == [want["N1"], want["N2"], want["count1"], want["count2"]], (name, keep_k, i)
            assert abs(le[i, 0] - want["le1"]) <= LE_TOL and abs(le[i, 1] - want["le2"]) <= LE_TOL, (name, keep_k, i)
            assert ms[i].tolist() == [wm["vis1"], wm["hit1"], wm["vis2"], wm["hit2"]], (name, keep_k, i)


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_counts_are_exact_and_sums_within_the_bound(name):
    check_batch(name)


@pytest.mark.parametrize("name", ["37x53", "300x257"])
def test_tie_rule_keeps_the_lower_rows(name):
    cases, _ = batch(name, True)
    keep_k = BATCHES[name][4][0]
    p = cases[0]["prob"][:, 2]
    kept = kr.select_k_best(p, keep_k)
    assert np.sum(p == p[kept[-1]]) > np.sum(p[kept] == p[kept[-1]])          # the cut runs through equal probabilities
    check_batch(name, True)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[4:-4] for f in FIXTURES])
def test_reference_fixtures_are_reproduced(path):
    z = np.load(path)
    data = {"prob": z["prob"], "warped_prob": z["warped_prob"], "homography": z["homography"], "image_shape": tuple(z["image_shape"])}
    keep_k, thresh = int(z["keep_k"]), float(z["distance_thresh"])
    n1, n2, rep, loc = km.compute_repeatability(data, keep_k, thresh)
    print(f"N1 {n1} N2 {n2} repeatability {rep!r} against {float(z['repeatability'])!r} loc_err {loc!r} against {float(z['loc_err'])!r}")
    assert (n1, n2) == (int(z["N1"]), int(z["N2"])) and type(n1) is int
    want = kr.repeatability_stats(z["prob"], z["warped_prob"], z["homography"], data["image_shape"], keep_k, thresh)
    counts, le = km.repeatability_stats(dev(z["prob"][None]), dev(np.array([len(z["prob"])], np.int32)), dev(z["warped_prob"][None]),
                                        dev(np.array([len(z["warped_prob"])], np.int32)), dev(z["homography"][None]),
                                        data["image_shape"], keep_k, thresh)
    assert counts[0].tolist() == [want["N1"], want["N2"], want["count1"], want["count2"]]
    if z["repeatability"] == -1:
        assert rep == -1 and loc == -1
    else:
        assert abs(rep - float(z["repeatability"])) <= 1e-9 and abs(loc - float(z["loc_err"])) <= 1e-9
        assert counts[0, 2].item() + counts[0, 3].item() == round(float(z["repeatability"]) * (n1 + n2))


@pytest.mark.parametrize("name", ["37x53", "1000x1000"])
def test_bit_identical_alone_in_a_batch_and_across_runs(name):
    _, arr = batch(name)
    shape, keep_ks = BATCHES[name][3], BATCHES[name][4]
    for keep_k in keep_ks:
        counts, le = run_rep(arr, shape, keep_k)
        ms = run_ms(arr, shape, keep_k)
        again = run_rep(arr, shape, keep_k)
        assert np.array_equal(bits(counts), bits(again[0])) and np.array_equal(bits(le), bits(again[1]))
        assert np.array_equal(bits(ms), bits(run_ms(arr, shape, keep_k)))
        for i in range(3):
            n0, n1 = int(arr["cnt0"][i]), int(arr["cnt1"][i])
            alone = {k: (v[i:i + 1, :n0] if k in ("pts0", "desc0") else v[i:i + 1, :n1] if k in ("pts1", "desc1") else v[i:i + 1])
                     for k, v in arr.items()}                                     # no padding either
            c1, l1 = run_rep(alone, shape, keep_k)
            assert np.array_equal(bits(c1)[0], bits(counts)[i]) and np.array_equal(bits(l1)[0], bits(le)[i]), (keep_k, i)
            assert np.array_equal(bits(run_ms(alone, shape, keep_k))[0], bits(ms)[i]), (keep_k, i)


def test_empty_and_degenerate_pairs():
    none3, none32 = np.zeros((0, 3), np.float32), np.zeros((0, 32), np.float32)
    data = {"prob": none3, "warped_prob": none3, "desc": none32, "warped_desc": none32, "homography": np.eye(3), "image_shape": (240, 320)}
    assert km.compute_repeatability(data) == (0, 0, -1, -1)
    assert km.compute_matching_score(data) == 0
    counts = km.matching_score_stats(dev(none3[None]), dev(np.zeros(1, np.int32)), dev(none32[None]), dev(none3[None]),
                                     dev(np.zeros(1, np.int32)), dev(none32[None]), dev(np.eye(3)[None]), (240, 320))
    assert counts.tolist() == [[0, 0, 0, 0]]
    # rows that exist in the tensors but not in the counts: the same
    case = kr.make_case(77, 37, 53, 32, (240, 320), (300,))
    zero = dev(np.zeros(1, np.int32))
    counts, le = km.repeatability_stats(dev(case["prob"][None]), zero, dev(case["warped_prob"][None]), zero, dev(case["homography"][None]),
                                        (240, 320))
    assert counts.tolist() == [[0, 0, 0, 0]] and bits(le).tolist() == [[0, 0]]
    counts = km.matching_score_stats(dev(case["prob"][None]), zero, dev(case["desc"][None]), dev(case["warped_prob"][None]), zero,
                                     dev(case["warped_desc"][None]), dev(case["homography"][None]), (240, 320))
    assert counts.tolist() == [[0, 0, 0, 0]]
    # every point of image 0 warped out of the box
    away = dict(case, homography=np.array([[1, 0, 1000.0], [0, 1, 0], [0, 0, 1]]))
    n1, n2, rep, loc = km.compute_repeatability(away)
    want = kr.compute_repeatability(away)
    assert n1 == 0 and (n1, n2, rep, loc) == want and n2 == 0
    ms = km.compute_matching_score(away)
    assert ms == kr.compute_matching_score(away) == 0.0
    # a singular homography: inv(H) does not exist (numpy raises); the device gives counts and no NaN
    flat = dict(case, homography=np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0.0]]))
    got = km.compute_repeatability(flat)
    assert got[0] == 0 and got[1] == 0 and got[2:] == (-1, -1)
    assert km.compute_matching_score(flat) == 0.0


@pytest.mark.parametrize("name", sorted(kr.known_cases()))
def test_hand_computed_matching_scores(name):
    data, keep_k, counts, ms = kr.known_cases()[name]
    got = km.compute_matching_score(data, keep_k)
    assert isinstance(got, float) and abs(got - ms) <= 1e-15
    if len(data["prob"]):
        n0, n1 = len(data["prob"]), len(data["warped_prob"])
        c = km.matching_score_stats(dev(data["prob"][None]), dev(np.array([n0], np.int32)), dev(data["desc"][None]),
                                    dev(data["warped_prob"][None]), dev(np.array([n1], np.int32)), dev(data["warped_desc"][None]),
                                    dev(data["homography"][None]), data["image_shape"], keep_k)
        assert tuple(c[0].tolist()) == counts


def test_python_surface():
    case = kr.make_case(78, 37, 53, 32, (240, 320), (300,))
    want = kr.compute_repeatability(case)
    got = km.compute_repeatability(case)                                   # numpy in: Python numbers out
    assert [type(v) for v in got] == [int, int, float, float] and got[:2] == want[:2]
    assert abs(got[2] - want[2]) <= 1e-12 and abs(got[3] - want[3]) <= 1e-9
    ms = km.compute_matching_score(case)
    assert type(ms) is float and abs(ms - kr.compute_matching_score(case)) <= 1e-12
    on_dev = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    assert km.compute_repeatability(on_dev) == got and km.compute_matching_score(on_dev) == ms
    on_cpu = {k: (torch.from_numpy(np.array(v)) if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    with pytest.raises(RuntimeError, match="CPU tensors are not supported"):
        km.compute_repeatability(on_cpu)
    with pytest.raises(RuntimeError, match="CPU tensors are not supported"):
        km.compute_matching_score(on_cpu)
    with pytest.raises(NotImplementedError):
        km.compute_homography(case)
    # bad shapes: KP2D_ERR_ARG with kp2d_last_error's text
    p0, p1 = dev(case["prob"][None]), dev(case["warped_prob"][None])
    c0, c1, hom = dev(np.array([37], np.int32)), dev(np.array([53], np.int32)), dev(case["homography"][None])
    with pytest.raises(_lib.Kp2dError, match="keep_k = 0") as e:
        km.repeatability_stats(p0, c0, p1, c1, hom, (240, 320), keep_k=0)
    assert e.value.code == -1
    with pytest.raises(_lib.Kp2dError, match="descriptor width 48") as e:
        km.matching_score_stats(p0, c0, dev(np.zeros((1, 37, 48), np.float32)), p1, c1, dev(np.zeros((1, 53, 48), np.float32)), hom, (240, 320))
    assert e.value.code == -1
    with pytest.raises(_lib.Kp2dError, match="bounds"):
        km.repeatability_stats(p0, c0, p1, c1, hom, (float("nan"), 320))
    with pytest.raises(ValueError, match=r"\[B, k, 3\]"):
        km.repeatability_stats(p0[:, :, :2], c0, p1, c1, hom, (240, 320))
    lib = _lib.load()
    assert lib.kp2d_kp_scratch_bytes(0, 37, 53, 0, 300) == 0 and lib.kp2d_kp_scratch_bytes(1, 37, 53, 48, 300) == 0
    assert lib.kp2d_kp_scratch_bytes(1, 37, 53, 32, 300) > lib.kp2d_kp_scratch_bytes(1, 37, 53, 0, 300) > 0
    small = torch.empty(256, dtype=torch.uint8, device="cuda")
    counts, le = torch.empty(1, 4, dtype=torch.int64, device="cuda"), torch.empty(1, 2, dtype=torch.float64, device="cuda")
    rc = lib.kp2d_kp_repeatability(km._ptr(p0), km._ptr(c0), km._ptr(p1), km._ptr(c1), km._ptr(hom), 1, 37, 53, 240.0, 320.0, 300, 3.0,
                                   km._ptr(counts), km._ptr(le), km._ptr(small), small.numel(), None)
    assert rc == -1 and b"kp2d_kp_scratch_bytes" in lib.kp2d_last_error()


# ---- end to end -------------------------------------------------------------------------------------------------------
# One sample of B = 2 pairs.  On the model's own descriptors a nearest neighbour that is clear by 1e-3 for EVERY query is rare:
# of 16 seeds scanned (21 ... 36) none had it for both pairs at top_k = 300, 100 or 50 and only seed 26 at top_k = 20 (the
# device equalled the oracle on all 128 scanned pairs and sizes all the same; the margin only decides what may be asserted).
E2E_SEEDS = (26,)
E2E_TOP_K = 20


@functools.lru_cache(maxsize=None)
def end_to_end():
    """tiny_factory("S") on the seeded synthetic weights, samples of B = 2 synthetic homography pairs at 120 x 160 ->
    (model, samples, per pair the host copies of the rows evaluate_keypoint_net builds from the model's outputs)."""
    from nano_vs_slam_amd.synthetic import homography_pairs
    model, _ = product_model("S", False, 28)
    model.device = "cuda:0"
    samples, pairs = [], []
    with torch.no_grad():
        for seed in E2E_SEEDS:
            image, hom, warped = homography_pairs(2, 120, 160, seed=seed)
            samples.append({"image": image.cpu(), "image_aug": warped.cpu(), "homography": hom.cpu()})
            out = model.post_processing(model(image), 120, 160)
            p0, d0, c0 = (t.cpu().numpy() for t in km.keypoint_rows(out["score"], out["coord"], out["feat"]))
            out = model.post_processing(model(warped), 120, 160)
            p1, d1, c1 = (t.cpu().numpy() for t in km.keypoint_rows(out["score"], out["coord"], out["feat"]))
            for b in range(2):
                pairs.append({"prob": p0[b, :c0[b]], "warped_prob": p1[b, :c1[b]], "desc": d0[b, :c0[b]], "warped_desc": d1[b, :c1[b]],
                              "homography": hom[b].cpu().numpy(), "image_shape": (120, 160)})
    return model, samples, pairs


def test_evaluate_keypoint_net_end_to_end():
    model, samples, pairs = end_to_end()
    reps, locs, mss, skipped = [], [], [], 0
    per_sample = []
    for s, sample in enumerate(samples):
        mine = pairs[2 * s:2 * s + 2]
        stats = [(kr.repeatability_stats(p["prob"], p["warped_prob"], p["homography"], (120, 160), E2E_TOP_K),
                  kr.matching_score_stats(p["prob"], p["warped_prob"], p["desc"], p["warped_desc"], p["homography"], (120, 160), E2E_TOP_K))
                 for p in mine]
        for p, (r, m) in zip(mine, stats):
            print(f"sample {s}: rows {len(p['prob'])} / {len(p['warped_prob'])}, oracle {kr.scores_from_repeatability(r)} ms "
                  f"{kr.score_from_matching(m)!r}, margins dist {min(r['margin_dist'], m['margin_dist']):.3g} box "
                  f"{min(r['margin_box'], m['margin_box']):.3g} nn {m['margin_nn']:.3g}")
        if not all(kr.margins_hold(r) and kr.margins_hold(m) for r, m in stats):
            skipped += 1                                                  # a decision within its margin: no single right answer
            continue
        per_sample.append((sample, stats))
    assert 4 * skipped <= len(samples), f"{skipped} of {len(samples)} samples violate a margin"
    for sample, stats in per_sample:
        got = km.evaluate_keypoint_net([sample], model, output_shape=(160, 120), top_k=E2E_TOP_K)
        want = [kr.scores_from_repeatability(r) for r, _ in stats]
        valid = [w for w in want if w[2] != -1]
        want_ms = float(np.mean([kr.score_from_matching(m) for _, m in stats]))
        print(f"evaluate_keypoint_net {got} against repeatability {[w[2] for w in want]} loc_err {[w[3] for w in want]} ms {want_ms!r}")
        assert len(got) == 7 and all(isinstance(v, float) for v in got) and all(math.isnan(got[i]) for i in (2, 3, 4, 6))
        assert valid and all(math.isfinite(got[i]) for i in (0, 1, 5))
        assert abs(got[0] - float(np.mean([w[2] for w in valid]))) <= 1e-9
        assert abs(got[1] - float(np.mean([w[3] for w in valid]))) <= 1e-9
        assert abs(got[5] - want_ms) <= 1e-9
        # exact counts on the same rows
        for b, (r, m) in enumerate(stats):
            p = pairs[2 * samples.index(sample) + b]
            one = lambda a: dev(np.ascontiguousarray(a)[None])
            n0, n1 = dev(np.array([len(p["prob"])], np.int32)), dev(np.array([len(p["warped_prob"])], np.int32))
            counts, _ = km.repeatability_stats(one(p["prob"]), n0, one(p["warped_prob"]), n1, one(p["homography"]), (120, 160), E2E_TOP_K)
            assert counts[0].tolist() == [r["N1"], r["N2"], r["count1"], r["count2"]]
            ms = km.matching_score_stats(one(p["prob"]), n0, one(p["desc"]), one(p["warped_prob"]), n1, one(p["warped_desc"]),
                                         one(p["homography"]), (120, 160), E2E_TOP_K)
            assert ms[0].tolist() == [m["vis1"], m["hit1"], m["vis2"], m["hit2"]]
    both = km.evaluate_keypoint_net(samples, model, output_shape=(160, 120), top_k=E2E_TOP_K)
    assert all(math.isfinite(both[i]) for i in (0, 1, 5))


def test_identity_pair_is_perfectly_repeatable():
    from nano_vs_slam_amd.synthetic import homography_pairs
    model, _, _ = end_to_end()
    image, hom, same = homography_pairs(2, 120, 160, seed=E2E_SEEDS[0], identity=True)
    got = km.evaluate_keypoint_net([{"image": image, "image_aug": same, "homography": hom}], model, output_shape=(160, 120), top_k=300)
    assert got[0] == 1.0 and got[1] == 0.0 and 0.0 < got[5] <= 1.0
