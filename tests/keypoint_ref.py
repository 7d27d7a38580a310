"""Float64 numpy oracle of the keypoint scores (nano_vs_slam_amd/keypoint_metrics.py, csrc/keypoint_metrics.hip) and the
generator of their test cases.

``repeatability_stats`` restates the reference's compute_repeatability (src/evaluation/detector.py:67-113),
``matching_score_stats`` its compute_matching_score (src/evaluation/descriptor.py:112-170) with a brute-force nearest
neighbour in float64 in place of cv2.BFMatcher (lowest index on ties), ``warp_keypoints`` its utils/keypoints.py:7-25.
Selection follows the library's tie rule: among equal probabilities the lower row is kept (the reference's argsort is
unstable and defines none).  The repeatability half is pinned by the reference's own code: tests/golden/keypoints/rep_*.npz
(tools/make_keypoint_golden.py).  Every stats function also reports how close any of its decisions came to its threshold,
so that a test can tell a case with one right answer from one without.
"""
import numpy as np

MARGIN_DIST = 1e-6        # no distance within this of its threshold
MARGIN_BOX = 1e-6         # no warped coordinate within this of a box / visibility bound
MARGIN_NN = 1e-3          # every query's second-nearest descriptor distance exceeds its nearest by more than this


def warp_keypoints(keypoints, H):
    n = keypoints.shape[0]
    hp = np.concatenate([keypoints, np.ones((n, 1))], axis=1)
    wp = np.dot(hp, np.transpose(H))
    with np.errstate(divide="ignore", invalid="ignore"):
        return wp[:, :2] / wp[:, 2:]


def select_k_best(prob, k):
    """Rows of the k most probable entries, most probable first; equal probabilities: lower row first."""
    order = np.lexsort((np.arange(prob.shape[0]), -prob.astype(np.float64)))
    return order[:min(k, prob.shape[0])]


def _box_margin(w, bounds):
    """Smallest distance of any coordinate of w [n,2] to 0 or to its bound."""
    if w.shape[0] == 0:
        return np.inf
    b = np.asarray(bounds, np.float64)
    return float(min(np.abs(w).min(), np.abs(w - b).min()))


def repeatability_stats(prob, warped_prob, H, shape, keep_k=300, distance_thresh=3):
    """-> dict N1, N2, count1, count2 (int), le1, le2 (float64), margin_dist, margin_box."""
    prob = np.asarray(prob, np.float64).reshape(-1, 3)
    warped_prob = np.asarray(warped_prob, np.float64).reshape(-1, 3)
    H = np.asarray(H, np.float64).reshape(3, 3)
    b0, b1 = float(shape[0]), float(shape[1])

    def inside(w):
        return (w[:, 0] >= 0) & (w[:, 0] < b0) & (w[:, 1] >= 0) & (w[:, 1] < b1)

    w1 = warp_keypoints(warped_prob[:, :2], np.linalg.inv(H))
    set1 = warped_prob[inside(w1)]
    w0 = warp_keypoints(prob[:, :2], H)
    in0 = inside(w0)
    set0 = np.concatenate([w0[in0], prob[in0, 2:3]], axis=1)
    set1 = set1[select_k_best(set1[:, 2], keep_k), :2]
    set0 = set0[select_k_best(set0[:, 2], keep_k), :2]
    N1, N2 = set0.shape[0], set1.shape[0]
    norm = np.linalg.norm(set0[:, None, :] - set1[None, :, :], axis=2)
    out = {"N1": N1, "N2": N2, "count1": 0, "count2": 0, "le1": 0.0, "le2": 0.0,
           "margin_box": min(_box_margin(w1, (b0, b1)), _box_margin(w0, (b0, b1))), "margin_dist": np.inf}
    if N1 and N2:
        for name, mins in (("1", norm.min(axis=1)), ("2", norm.min(axis=0))):
            ok = mins <= distance_thresh
            out["count" + name] = int(ok.sum())
            out["le" + name] = float(mins[ok].sum())
            out["margin_dist"] = min(out["margin_dist"], float(np.abs(mins - distance_thresh).min()))
    return out


def scores_from_repeatability(st):
    """-> (N1, N2, repeatability, loc_err) as the reference returns them."""
    n, c = st["N1"] + st["N2"], st["count1"] + st["count2"]
    if n > 0 and c > 0:
        return st["N1"], st["N2"], c / n, (st["le1"] + st["le2"]) / c
    return st["N1"], st["N2"], -1, -1


def compute_repeatability(data, keep_k_points=300, distance_thresh=3):
    return scores_from_repeatability(repeatability_stats(data["prob"], data["warped_prob"], data["homography"], data["image_shape"],
                                                         keep_k_points, distance_thresh))


def nearest(query, train):
    """Brute force in float64 -> (index of the nearest train row [nq] (lowest on ties), second-nearest minus nearest [nq])."""
    q, t = np.asarray(query, np.float64), np.asarray(train, np.float64)
    d2 = np.maximum((q * q).sum(1)[:, None] - 2.0 * q @ t.T + (t * t).sum(1)[None, :], 0.0)
    idx = d2.argmin(axis=1)
    if t.shape[0] < 2:
        return idx, np.full(q.shape[0], np.inf)
    two = np.sqrt(np.partition(d2, 1, axis=1)[:, :2])
    return idx, two[:, 1] - two[:, 0]


def matching_score_stats(prob, warped_prob, desc, warped_desc, H, shape, keep_k=1000):
    """-> dict vis1, hit1, vis2, hit2 (int), margin_dist, margin_box, margin_nn, bad0 / bad1 (selected rows of set 0 / set 1,
    as rows of the inputs, whose nearest neighbour is not clear by MARGIN_NN)."""
    prob = np.asarray(prob, np.float64).reshape(-1, 3)
    warped_prob = np.asarray(warped_prob, np.float64).reshape(-1, 3)
    H = np.asarray(H, np.float64).reshape(3, 3)
    out = {"vis1": 0, "hit1": 0, "vis2": 0, "hit2": 0, "margin_dist": np.inf, "margin_box": np.inf, "margin_nn": np.inf,
           "bad0": np.zeros(0, np.int64), "bad1": np.zeros(0, np.int64)}
    if prob.shape[0] == 0 or warped_prob.shape[0] == 0:
        return out
    s0, s1 = select_k_best(prob[:, 2], keep_k), select_k_best(warped_prob[:, 2], keep_k)
    kp0, kp1 = prob[s0, :2], warped_prob[s1, :2]
    d0, d1 = np.asarray(desc)[s0], np.asarray(warped_desc)[s1]
    vis_max = np.asarray(shape, np.float64) - 1.0
    for name, q, t, dq, dt, M, sel in (("1", kp0, kp1, d0, d1, np.linalg.inv(H), s0), ("2", kp1, kp0, d1, d0, H, s1)):
        idx, gap = nearest(dq, dt)
        w = warp_keypoints(t[idx], M)
        vis = np.all((w >= 0) & (w <= vis_max), axis=-1)
        norm = np.linalg.norm(w - q, axis=-1)
        out["vis" + name] = int(vis.sum())
        out["hit" + name] = int(((norm < 3) & vis).sum())
        out["margin_dist"] = min(out["margin_dist"], float(np.abs(norm - 3.0).min()))
        out["margin_box"] = min(out["margin_box"], _box_margin(w, vis_max))
        out["margin_nn"] = min(out["margin_nn"], float(gap.min()))
        out["bad0" if name == "1" else "bad1"] = sel[gap <= MARGIN_NN]
    return out


def score_from_matching(st):
    return (st["hit1"] / max(st["vis1"], 1.0) + st["hit2"] / max(st["vis2"], 1.0)) / 2


def compute_matching_score(data, keep_k_points=1000):
    return score_from_matching(matching_score_stats(data["prob"], data["warped_prob"], data["desc"], data["warped_desc"],
                                                    data["homography"], data["image_shape"], keep_k_points))


def margins_hold(st):
    return (st["margin_dist"] > MARGIN_DIST and st["margin_box"] > MARGIN_BOX and st.get("margin_nn", np.inf) > MARGIN_NN)


# ---- case generator ---------------------------------------------------------------------------------------------------
def random_homography(rng, shape):
    """Bounded perspective, rotation, scale and translation about the middle of the box [0, b0) x [0, b1), float64."""
    b0, b1 = float(shape[0]), float(shape[1])
    a = rng.uniform(-0.25, 0.25)
    s = rng.uniform(0.85, 1.2)
    c = np.array([[1, 0, b0 / 2], [0, 1, b1 / 2], [0, 0, 1.0]])
    r = np.array([[s * np.cos(a), -s * np.sin(a), rng.uniform(-0.12, 0.12) * b0],
                  [s * np.sin(a), s * np.cos(a), rng.uniform(-0.12, 0.12) * b1],
                  [rng.uniform(-0.2, 0.2) / b0, rng.uniform(-0.2, 0.2) / b1, 1.0]])
    return c @ r @ np.linalg.inv(c)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make_case(seed, k0, k1, C=32, shape=(240, 320), keep_ks=(300, 1000), ties=False, distance_thresh=3):
    """One pair: points drawn in the box (the reference's convention: x in [0, b0), y in [0, b1)); a bounded homography, so
    some points leave the box in each direction; a share of set 1 planted as warped set-0 points plus noise below and above
    the threshold, their descriptors planted as near-copies; distinct probabilities (``ties``: drawn from five values, so the
    keep_k cut runs through equal ones); unit-norm float32 descriptors.  Draws again until the three margins hold for every
    keep_k in ``keep_ks`` (descriptor rows whose nearest neighbour is not clear are drawn again on their own).
    -> dict prob [k0,3], warped_prob [k1,3], desc [k0,C], warped_desc [k1,C] float32, homography [3,3] float64, image_shape."""
    b0, b1 = float(shape[0]), float(shape[1])
    for attempt in range(64):
        rng = np.random.default_rng([seed, attempt])
        H = random_homography(rng, shape)
        xy0 = rng.uniform(0, 1, (k0, 2)) * (b0, b1)
        xy1 = rng.uniform(0, 1, (k1, 2)) * (b0, b1)
        d0 = _unit(rng.standard_normal((k0, C)))
        d1 = _unit(rng.standard_normal((k1, C)))
        planted = (min(k0, k1) + 1) // 2
        if planted:
            src = rng.permutation(k0)[:planted]
            dst = rng.permutation(k1)[:planted]
            radius = np.where(rng.random(planted) < 0.7, rng.uniform(0.1, 2.6, planted), rng.uniform(3.4, 6.0, planted))
            ang = rng.uniform(0, 2 * np.pi, planted)
            xy1[dst] = warp_keypoints(xy0[src], H) + radius[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
            d1[dst] = _unit(d0[src] + rng.standard_normal((planted, C)) * (0.1 / np.sqrt(C)))
        if ties:
            p0 = rng.choice([0.75, 0.8, 0.85, 0.9, 0.95], k0)
            p1 = rng.choice([0.75, 0.8, 0.85, 0.9, 0.95], k1)
        else:
            p0 = 0.7 + 0.29 * (rng.permutation(k0) + rng.uniform(0.1, 0.9, k0)) / max(k0, 1)
            p1 = 0.7 + 0.29 * (rng.permutation(k1) + rng.uniform(0.1, 0.9, k1)) / max(k1, 1)
        case = {"prob": np.concatenate([xy0, p0[:, None]], 1).astype(np.float32),
                "warped_prob": np.concatenate([xy1, p1[:, None]], 1).astype(np.float32),
                "desc": d0.astype(np.float32), "warped_desc": d1.astype(np.float32),
                "homography": H, "image_shape": tuple(shape)}
        if not ties and (np.unique(case["prob"][:, 2]).size != k0 or np.unique(case["warped_prob"][:, 2]).size != k1):
            continue
        ok = True
        for keep_k in keep_ks:
            ok = ok and margins_hold(repeatability_stats(case["prob"], case["warped_prob"], H, shape, keep_k, distance_thresh))
        for _ in range(200):                                           # unclear nearest neighbours: those rows again
            bad0, bad1 = [], []
            for keep_k in keep_ks:
                st = matching_score_stats(case["prob"], case["warped_prob"], case["desc"], case["warped_desc"], H, shape, keep_k)
                bad0.append(st["bad0"])
                bad1.append(st["bad1"])
            bad0, bad1 = np.unique(np.concatenate(bad0)), np.unique(np.concatenate(bad1))
            if bad0.size == 0 and bad1.size == 0:
                break
            case["desc"][bad0] = _unit(rng.standard_normal((bad0.size, C))).astype(np.float32)
            case["warped_desc"][bad1] = _unit(rng.standard_normal((bad1.size, C))).astype(np.float32)
        for keep_k in keep_ks:
            st = matching_score_stats(case["prob"], case["warped_prob"], case["desc"], case["warped_desc"], H, shape, keep_k)
            ok = ok and margins_hold(st)
        if ok:
            return case
    raise AssertionError(f"make_case(seed={seed}, k0={k0}, k1={k1}): the margins did not hold in 64 draws")


# ---- hand-computed cases ----------------------------------------------------------------------------------------------
ONE_HOT = np.eye(4, 32, dtype=np.float32)               # one-hot descriptors e0 .. e3
SHIFT = [[1, 0, 2], [0, 1, 0], [0, 0, 1]]               # x -> x + 2
MIXED = (ONE_HOT[2] + 0.1 * ONE_HOT[1]) / np.linalg.norm(ONE_HOT[2] + 0.1 * ONE_HOT[1])


def pair(prob, warped, desc, wdesc, H, shape):
    return {"prob": np.array(prob, np.float32).reshape(-1, 3), "warped_prob": np.array(warped, np.float32).reshape(-1, 3),
            "desc": np.array(desc, np.float32).reshape(len(prob), 32), "warped_desc": np.array(wdesc, np.float32).reshape(len(warped), 32),
            "homography": np.array(H, np.float64), "image_shape": shape}


def known_cases():
    """name -> (pair, keep_k, (vis1, hit1, vis2, hit2), ms): matching scores worked out by hand."""
    E = ONE_HOT
    three = [(0, 0, .9), (4, 4, .8), (7, 7, .75)], [(2, 0, .9), (6.5, 4, .8)], E[:3], [E[0], MIXED], SHIFT, (8, 8)
    return {
        # matches 0 -> 0, 1 -> 1 both ways.  Direction 1: (1,2) visible, 1 px from (1,1): hit; (9.5,5) has x > 9: not visible.
        # Direction 2: (1,1) visible, hit; (5,5) visible, 4.5 px from (9.5,5): no hit.
        "identity": (pair([(1, 1, .9), (5, 5, .8)], [(1, 2, .9), (9.5, 5, .8)], E[:2], E[:2], np.eye(3), (10, 10)), 1000, (1, 1, 2, 1), 0.75),
        # Direction 1: rows 0, 1, 2 match rows 0, 1, 1 (e1 is nearer to MIXED than to e0); warped back (0,0), (4.5,4), (4.5,4), all
        # visible; distances 0, 0.5, sqrt(6.25 + 9) -> 2 hits.  Direction 2: rows 0, 1 match rows 0, 2; warped (2,0): visible, hit;
        # (9,7): x > 7, not visible.
        "shift": (pair(*three), 1000, (3, 2, 1, 1), 5.0 / 6.0),
        # keep_k = 1: only row 0 of each set
        "shift_keep1": (pair(*three), 1, (1, 1, 1, 1), 1.0),
        # the distance is exactly 3: `< 3` is strict
        "strict": (pair([(1, 1, .9)], [(4, 1, .9)], E[:1], E[:1], np.eye(3), (10, 10)), 1000, (1, 0, 1, 0), 0.0),
        "empty": (pair([], [(4, 1, .9)], np.zeros((0, 32)), E[:1], np.eye(3), (10, 10)), 1000, (0, 0, 0, 0), 0.0),
    }
