"""keypoint_shapes_ref held to itself without a device: the scratch walk against the library's own sizes, the geometry each
case was chosen for, the seed rule for the constants kept there, the placed patterns on the oracle, the bounds (from the
oracle's float32 run alone), and the very evaluate() that test_gpu_keypoint_shapes.py calls accepting that float32 run and
refusing every wrong walk of MUTANTS."""
import numpy as np
import pytest

import keypoint_shapes_ref as ks

kr = ks.kr


# ---- 1. scratch ----------------------------------------------------------------------------------------------------------------
def test_scratch_walk_is_the_library_s():
    from nano_vs_slam_amd import _lib
    lib = _lib.load()
    assert len(ks.PIECE_NAMES) == len(ks.pieces(1, 10, 10, 16)) == len(ks.PIECE_DTYPES) == 23
    for case in ks.CASES:
        B, Hc, Wc, cell, C, Hf, Wf = ks.shape_of(case)
        pieces = ks.pieces(B, Hc, Wc, C)
        got, raw = int(lib.kp2d_keypoint_loss_scratch_bytes(B, Hc, Wc, C, Hf, Wf)), sum(n * s for n, s in pieces)
        assert got == ks.carve(pieces) and raw <= got < raw + ks.ALIGN * len(pieces), (case, got)
        assert all(np.dtype(ks.PIECE_DTYPES[k]).itemsize in (size, size // 2, size // 4) for k, (_, size) in zip(ks.PIECE_NAMES, pieces))
    # fewer than 20 interior cells: the descriptor pieces are empty
    assert int(lib.kp2d_keypoint_loss_scratch_bytes(2, 6, 6, 16, 12, 12)) == ks.carve(ks.pieces(2, 6, 6, 16))
    for bad in ((1, 10, 10, 272, 20, 20), (1, 10, 10, 24, 20, 20), (1, 1, 65537, 16, 20, 20)):
        assert int(lib.kp2d_keypoint_loss_scratch_bytes(*bad)) == 0, bad


# ---- 2. what each case reaches ---------------------------------------------------------------------------------------------------
def test_geometry_of_the_cases():
    g = {c: ks.geometry(c) for c in ks.CASES}
    C = {c: ks.shape_of(c)[4] for c in ks.CASES}
    k1 = g["K1"]
    assert (k1["N"], k1["n"]) == (324, 256) and C["K1"] == 128 and (k1["chunks"], k1["kc"]) == (2, 64)
    assert (k1["anchor_tiles"], k1["last_anchor_tile"], k1["passes"], k1["ballots"]) == (4, 64, 1, 4) and ks.shape_of("K1")[0] == 2
    k2 = g["K2"]
    assert (k2["N"], k2["n"], k2["cell_tiles"], k2["last_cell_tile"]) == (256, 196, 1, 256) and (k2["chunks"], k2["kc"]) == (2, 16) and k2["feat_groups"] == 1
    assert ks.shape_of("K2")[5] * ks.shape_of("K2")[6] == 256
    k3 = g["K3"]
    assert (k3["N"], k3["n"], k3["cell_tiles"], k3["last_cell_tile"]) == (600, 504, 3, 88)
    assert (k3["anchor_tiles"], k3["last_anchor_tile"], k3["passes"], k3["chunks"], k3["kc"]) == (8, 56, 2, 4, 64) and C["K3"] == 256
    k4 = g["K4"]
    assert (k4["N"], k4["n"], k4["cell_tiles"], k4["anchor_tiles"], k4["passes"]) == (1056, 930, 5, 15, 4) and ks.shape_of("K4")[5] == ks.shape_of("K4")[1]
    k5 = g["K5"]
    assert (k5["N"], k5["n"], k5["cell_tiles"], k5["last_cell_tile"]) == (512, 420, 2, 256) and ks.shape_of("K5")[3] == 8
    k6 = g["K6"]
    assert (k6["N"], k6["n"], k6["chunks"], k6["kc"]) == (168, 120, 2, 16) and ks.STRONG == {"K6": (1,)} and ks.shape_of("K6")[0] == 2
    sweep = [g[f"S{c}"] for c in ks.SWEEP + (96,)]
    assert all((s["N"], s["n"], s["anchor_tiles"], s["last_anchor_tile"]) == (100, 64, 1, 64) for s in sweep)
    assert {s["chunks"] for s in sweep} == {1, 2, 3, 4} and {s["kc"] for s in sweep} == {16, 32, 48, 64}
    assert {(s["chunks"], s["kc"]) for s in sweep} == {(1, 48), (2, 16), (2, 32), (2, 48), (2, 64), (3, 16), (3, 64), (4, 16), (4, 64)}
    t = g["Ta"]
    assert (t["N"], t["n"], t["cell_tiles"], t["anchor_tiles"], t["last_anchor_tile"], t["ballots"]) == (300, 230, 2, 4, 38, 4)
    # the tied columns against kd_search's layout: candidate jl of a tile sits in lane group (jl % 16) / 4, register jl % 4 of
    # product tile jl / 16
    where = lambda k: (k // 64, k % 64 // 16, k % 16 // 4, k % 4)
    assert where(5) == (0, 0, 1, 1) and where(6) == (0, 0, 1, 2) and where(9) == (0, 0, 2, 1) and where(21) == (0, 1, 1, 1)
    assert where(69) == (1, 0, 1, 1) and where(229) == (3, 2, 1, 1) and 229 == t["n"] - 1
    assert all(where(a)[2] <= where(b)[2] for a, b in ks.TIES)                   # the lower index never in the higher lane group ...
    assert where(16) == (0, 1, 0, 0) and where(13) == (0, 0, 3, 1) and ks.LANE_TIES == ((5, 16), (13, 16))      # ... but here
    assert max(v["n"] for v in g.values()) == 930 and max(C.values()) == 256


def test_k6_taps_leave_both_maps():
    o = ks.oracle("K6")
    Hf, Wf = ks.shape_of("K6")[5:]
    p = o["stages"]["pairs"][1]
    for pts in p["pts"][1:]:                                    # the target map at the warped points
        out = sum(int((~inside).sum()) for _, _, _, inside in kr._taps(pts[0], pts[1], Hf, Wf))
        assert out >= 100
    assert (np.abs(o["q"]["wn"][:, 1]) > 1).any(axis=0).sum() >= 30 and (o["d"][1] >= kr.VALID_DIST).sum() >= 30


# ---- 3. seeds and placed patterns ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ks.CASES)
def test_seed_meets_the_generator_s_conditions(case):
    assert (ks.SEEDS[case] - ks.BASE_SEED[case]) % 1000 == 0 and ks.SEEDS[case] < ks.BASE_SEED[case] + 1000 * 1000
    assert ks.refusal(case, ks.SEEDS[case]) is None
    o64, o32 = ks.oracle(case), ks.oracle(case, np.float32)
    for a, b in zip(o64["stages"]["pairs"], o32["stages"]["pairs"]):
        assert np.array_equal(a["neg"], b["neg"]) and np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["hinge"] > 0, b["hinge"] > 0)
    for k in kr.GRADS:                                              # the float32 run is float32 throughout
        assert o32[k].dtype == np.float32 and o64[k].dtype == np.float64, k
    for p in o32["stages"]["pairs"]:
        assert all(p[k].dtype == np.float32 for k in ("r", "t", "hinge", "cn", "g_pos", "g_neg"))
    on = np.concatenate([p["hinge"] > 0 for p in o64["stages"]["pairs"]])
    assert on.any() and (case in ks.PLACED or not on.all())


def test_conditions_refuse_and_exempt():
    case = "Tb5-6"
    inp = ks.inputs(case)
    o64, o32 = ks.oracle(case), ks.oracle(case, np.float32)
    assert kr.conditions(o64, o32, ks.exemptions(case, o64)) is None
    assert "negative's gap" in kr.conditions(o64, o32)                  # without the exemption the tie itself is refused
    o = ks.oracle("Ta")
    assert "gap behind a_i" in kr.conditions(o, ks.oracle("Ta", np.float32))
    assert o["gaps"]["a"][0, 255] == 0.0 and inp["cell"] == 5 and inp["H"] == inp["W"] == 129


@pytest.mark.parametrize("case", ks.PLACED)
def test_placed_patterns_on_the_oracle(case):
    o = ks.oracle(case)
    assert ks.check_placed(case, o) is None
    if case == "Ta":
        return
    k1, k2 = ks.tie_of(case)
    p = o["stages"]["pairs"][0]
    mine = np.flatnonzero((p["neg"] == k1) & (p["cn"] != 0))
    per = np.bincount(mine // ks.BALLOT, minlength=4)
    print(f"{case}: k1 is the negative of {mine.size} active anchors, per ballot chunk {per.tolist()}")
    assert mine.size >= 65 and (per > 0).sum() >= 3 and per.max() >= 2
    assert int(p["hit"].sum()) >= 1 and p["hit"][k1] and (p["neg"] == k2).sum() >= 1
    # the coordinates are exact: the float32 run's equal the float64 run's
    for k in ("w", "u"):
        assert np.array_equal(ks.oracle(case, np.float32)["q"][k].astype(np.float64), o["q"][k]), k


# ---- 4. one set of evaluate functions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ks.CASES)
def test_evaluate_accepts_the_float32_run(case):
    fails, ratios = ks.evaluate(case, ks.emulate(case))
    b = ks.bounds(case)
    assert set(b) == set(ks.QUANTITIES) == set(ratios) and all(ks.FLOOR <= v < 1e-3 for v in b.values())
    print(f"{case}: bounds " + ", ".join(f"{k} {v:.2e}" for k, v in b.items() if v > ks.FLOOR))
    if case in ks.PLACED:           # the floor alone is asked of the device, whose per-anchor reductions are float64
        assert all(v == ks.FLOOR for k, v in b.items() if k not in ks.WIDENED or case == "Ta")
        assert not [f for f in fails if "above its bound" not in f], fails
        return
    assert not fails and max(ratios.values()) <= 0.125 + 1e-12, (fails, ratios)
    fails, ratios = ks.evaluate(case, ks.as_got(ks.oracle(case)))
    assert not fails and max(ratios.values()) == 0.0


@pytest.mark.parametrize("mut", ks.MUTANTS)
def test_wrong_walks_are_refused(mut):
    assert set(ks.MUTANT_CASES) == set(ks.MUTANTS) and not ks.UNDETECTED
    for case in ks.MUTANT_CASES[mut]:
        base = ks.evaluate(case, ks.emulate(case))[0]
        fails = [f for f in ks.evaluate(case, ks.emulate(case, mut))[0] if f not in base]
        print(f"{mut} on {case}: {fails[:3] or 'not detected'}")
        assert fails, (mut, case)
        want = {"first_chunk_products": "neg", "stale_anchor_chunk": "neg", "first_pass_rows": "r:", "no_ragged_cell_tile": "a differs",
                "higher_index_a": "a differs", "higher_index_neg": "neg", "plain_less_merge": "neg", "first_feat_pass": "dfeat", "first_ballot_chunk": "dfeat_t",
                "one_bit_per_ballot": "dfeat_t"}[mut]
        assert any(f.startswith(want) for f in fails), fails


# ---- 5. the one widened bound ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ks.PLACED)
def test_device_order_restatement(case):
    """dfeat of the tied cases is bounded by the float32 restatement of the device's own order, not by the floor: the
    restatement, put in the place of the float32 run's stages, passes evaluate with every widened quantity at 1 / 8; on Ta,
    where no column collects more than a few anchors, it stays below 16 x 2^-24 and nothing is widened."""
    own, b = ks.errors(case, ks.device_order32(case)), ks.bounds(case)
    print(f"{case}: device order in float32, E " + ", ".join(f"{k} {v:.2e}" for k, v in own.items()))
    assert set(own) == {"dfeat_t", "dfeat_s", "r", "t", "hinge"} and all(own[k] <= ks.FLOOR for k in ("r", "t", "hinge"))
    if case == "Ta":
        assert all(v <= ks.FLOOR for v in own.values()) and all(v == ks.FLOOR for v in b.values())
        return
    assert ks.FLOOR < own["dfeat_t"] < 3e-5 and own["dfeat_s"] < 3e-6               # a lost anchor of a column: 1 / 228 = 4e-3
    assert all(b[k] == max(8.0 * own[k], ks.FLOOR) for k in ks.WIDENED)
    got = {**ks.as_got(ks.oracle(case)), **ks.device_order32(case)}
    fails, ratios = ks.evaluate(case, got)
    assert not fails and ratios["dfeat_t"] == 0.125 and ratios["dfeat_s"] <= 0.125, (fails, ratios)


def test_plain_less_merge_needs_the_lane_ties():
    """take_lower as a plain "<" changes nothing at the five ties whose lower index sits in the same or a lower lane group:
    stated, not hidden (the mutated kernel passes them on the device too); the two lane ties refuse it."""
    for a, b in ks.TIES:
        case = f"Tb{a}-{b}"
        got = ks.emulate(case, "plain_less_merge")
        assert np.array_equal(got["neg"], ks.emulate(case)["neg"]) and np.array_equal(got["hit"], ks.emulate(case)["hit"]), case
