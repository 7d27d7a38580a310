"""References of the triplet mining (nano_vs_slam_amd.mining, csrc/mining.hip) and the conditions under which its tests
compare exactly.

(a) ``ref_init`` / ``ref_getitem``: the reference's own steps with sklearn, restated line by line from
    src/data/pittsburgh.py:260-289 and :303-333 — the features come from an array instead of an HDF5 file and the result
    of ``np.random.choice`` (``negSample``) is passed in.
(b) ``radius_member`` / ``masked_topk`` / ``draws`` / ``mine_oracle``: float64 numpy, the device's conventions: closed ball
    with separately rounded operations, top-k over vpr_ref.distances64 with non-members at +inf and ties by lower row, the
    device's draw function restated in Python integers, rank-select over set bits, the violation rule in float64.
tests/test_mining_cpu.py holds (a) and (b) to each other; tests/test_gpu_mining.py holds the device to (b).

Exact comparison (``exactness``).  With u = 2^-24 the search's returned squared distance is within
e(d2) = vpr_ref.eps_dist(d2) of float64.  In Euclidean terms that is band(d) = d - sqrt(d^2 - e(d^2)) (the larger of the
two sides).  The device classifies candidate j as float64 does unless |dNeg_j - (dPos + sqrt(margin))| <= band(dNeg_j) +
band(dPos); it picks the float64 positive unless the two nearest positives are within 2 eps_key; it orders two violators as
float64 does unless their squared distances are within e + e; and the nNeg-th and the next candidate keep their sides
unless they are within 2 max(eps_key, e).  ``exactness`` counts the queries that meet any of these; the mining tests
require zero, so the comparison needs no exemption.
"""
from __future__ import annotations

import numpy as np

import vpr_ref as vr

MASK64 = (1 << 64) - 1


# ---- masks -----------------------------------------------------------------------------------------------------------
def pack_bits(member):
    """bool [nq, ndb] -> uint32 words [nq, ceil(ndb / 32)], bit by bit (the format's definition)."""
    member = np.asarray(member, bool)
    nq, ndb = member.shape
    out = np.zeros((nq, (ndb + 31) // 32), np.uint32)
    for i in range(nq):
        for r in np.flatnonzero(member[i]):
            out[i, r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    return out


def unpack_bits(words, ndb):
    words = np.asarray(words).view(np.uint32)
    out = np.zeros((words.shape[0], ndb), bool)
    for r in range(ndb):
        out[:, r] = (words[:, r >> 5] >> np.uint32(r & 31)) & 1
    return out


def radius_member(utmDb, utmQ, radius, invert=False):
    """bool [nq, ndb]: dx dx + dy dy <= radius radius in float64, every operation rounded on its own."""
    db, q = np.asarray(utmDb, np.float64), np.asarray(utmQ, np.float64)
    dx = db[None, :, 0] - q[:, None, 0]
    dy = db[None, :, 1] - q[:, None, 1]
    inside = dx * dx + dy * dy <= np.float64(radius) * np.float64(radius)
    return ~inside if invert else inside


def radius_gap(utmDb, utmQ, radius):
    """Smallest | distance - radius | over all pairs (metres): the radius tests' precondition."""
    db, q = np.asarray(utmDb, np.float64), np.asarray(utmQ, np.float64)
    d = np.sqrt(((db[None] - q[:, None]) ** 2).sum(-1))
    return float(np.abs(d - radius).min()) if d.size else np.inf


# ---- (a) the reference, restated -------------------------------------------------------------------------------------
def ref_init(utmDb, utmQ, posDistThr, nonTrivPosDistSqThr):
    """pittsburgh.py:260-289 -> (nontrivial_positives, queries, potential_negatives)."""
    from sklearn.neighbors import NearestNeighbors
    numDb = len(utmDb)
    knn = NearestNeighbors(n_jobs=1)
    knn.fit(utmDb)
    nontrivial_positives = list(knn.radius_neighbors(utmQ, radius=nonTrivPosDistSqThr ** 0.5, return_distance=False))
    for i, posi in enumerate(nontrivial_positives):
        nontrivial_positives[i] = np.sort(posi)
    queries = np.where(np.array([len(x) for x in nontrivial_positives]) > 0)[0]
    potential_positives = knn.radius_neighbors(utmQ, radius=posDistThr, return_distance=False)
    potential_negatives = []
    for pos in potential_positives:
        potential_negatives.append(np.setdiff1d(np.arange(numDb), pos, assume_unique=True))
    return nontrivial_positives, queries, potential_negatives


def ref_getitem(index, h5feat, numDb, nontrivial_positives, negCache, negSample, nNeg, nNegFactor, margin):
    """pittsburgh.py:296-333 for query number ``index`` (already re-mapped through ``queries``) -> None, or
    (posIndex, negIndices, dPos); ``negCache`` is updated as there.  ``h5feat``: [numDb + numQ, d], the cache layout.
    One departure: sklearn refuses n_neighbors above the number of fitted rows, so the count is clamped to it (the device
    pads its list instead)."""
    from sklearn.neighbors import NearestNeighbors
    qOffset = numDb
    qFeat = h5feat[index + qOffset]
    posFeat = h5feat[nontrivial_positives[index].tolist()]
    knn = NearestNeighbors(n_jobs=1)
    knn.fit(posFeat)
    dPos, posNN = knn.kneighbors(qFeat.reshape(1, -1), 1)
    dPos = dPos.item()
    posIndex = nontrivial_positives[index][posNN[0]].item()
    negSample = np.unique(np.concatenate([negCache[index], negSample]))
    negFeat = h5feat[list(map(int, negSample))]
    knn.fit(negFeat)
    dNeg, negNN = knn.kneighbors(qFeat.reshape(1, -1), min(nNeg * nNegFactor, len(negSample)))
    dNeg = dNeg.reshape(-1)
    negNN = negNN.reshape(-1)
    violatingNeg = dNeg < dPos + margin ** 0.5
    if np.sum(violatingNeg) < 1:
        return None
    negNN = negNN[violatingNeg][:nNeg]
    negIndices = negSample[negNN].astype(np.int32)
    negCache[index] = negIndices
    return posIndex, negIndices, dPos


# ---- (b) the float64 oracle with the device's conventions --------------------------------------------------------------
def mix(z):
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw(seed, rnd, qid, j):
    return mix(mix(mix((seed + 0x9E3779B97F4A7C15) & MASK64) ^ (((rnd & 0xFFFFFFFF) << 32) | (qid & 0xFFFFFFFF))) ^ (j & 0xFFFFFFFF))


def draws(neg_member_row, seed, rnd, qid, n_sample):
    """The rows the n_sample draws of one query select (with repetitions, in draw order): rank u among the set bits."""
    rows = np.flatnonzero(neg_member_row)
    if len(rows) == 0:
        return np.zeros(0, np.int64)
    return np.array([rows[draw(seed, rnd, qid, j) % len(rows)] for j in range(n_sample)], np.int64).reshape(-1)


def masked_topk(d64, member, k):
    """float64 top-k over the member rows: ascending distance, ties by lower row, padding (inf, -1)."""
    D, I = vr.topk64(np.where(member, d64, np.inf), k)
    I = np.where(np.isfinite(D), I, -1)
    return D, I


def margin64(margin):
    return np.sqrt(np.float64(np.float32(margin)))      # the C ABI takes a float: sqrt((double)margin)


def mine_oracle(dbFeat, qFeat, pos_member, neg_member, cache, n_sample, nNeg, nNegFactor, margin, seed, rnd, qid=None):
    """One round -> dict(pos_idx [nq] int64, neg_idx [nq, nNeg] int32, neg_cnt [nq], d_pos [nq] float64 (NaN: none),
    cand bool [nq, ndb], d64 [nq, ndb], dneg / ineg: the ascending candidate lists [nq, K])."""
    nq, ndb = pos_member.shape
    K = nNeg * nNegFactor
    qid = np.arange(nq) if qid is None else np.asarray(qid)
    d64 = vr.distances64(dbFeat, qFeat)
    cand = np.zeros((nq, ndb), bool)
    for i in range(nq):
        if cache is not None:
            c = np.asarray(cache[i])
            cand[i, c[(c >= 0) & (c < ndb)].astype(np.int64)] = True
        cand[i, draws(neg_member[i], seed, rnd, int(qid[i]), n_sample)] = True
    dp, ip = masked_topk(d64, pos_member, 1)
    dn, ineg = masked_topk(d64, cand, K)
    pos_idx = ip[:, 0]
    neg_idx = np.full((nq, nNeg), -1, np.int32)
    neg_cnt = np.zeros(nq, np.int32)
    d_pos = np.full(nq, np.nan)
    for i in range(nq):
        if pos_idx[i] < 0:
            continue
        d_pos[i] = np.sqrt(dp[i, 0])
        viol = (ineg[i] >= 0) & (np.sqrt(dn[i]) < d_pos[i] + margin64(margin))
        take = ineg[i][viol][:nNeg]
        neg_idx[i, :len(take)] = take
        neg_cnt[i] = len(take)
    return dict(pos_idx=pos_idx, neg_idx=neg_idx, neg_cnt=neg_cnt, d_pos=d_pos, cand=cand, d64=d64, dneg=dn, ineg=ineg)


def band(d):
    """The search's re-score bound on a squared distance, in Euclidean terms (the larger side)."""
    d = np.asarray(d, np.float64)
    return d - np.sqrt(np.maximum(d * d - vr.eps_dist(d * d), 0.0))


def exactness(o, dbFeat, qFeat, pos_member, nNeg, margin, split):
    """Number of queries of a mine_oracle result ``o`` whose device answer may differ from float64 (module docstring)."""
    ek = vr.eps_key(dbFeat, qFeat, split)
    d64 = o["d64"]
    bad = 0
    for i in range(len(d64)):
        if o["pos_idx"][i] < 0:
            continue
        hit = False
        pos = np.flatnonzero(pos_member[i])
        dps = np.sort(d64[i, pos])
        if len(dps) > 1 and dps[1] - dps[0] <= 2 * ek[i, pos].max():
            hit = True
        ok = o["ineg"][i] >= 0
        rows, dn = o["ineg"][i][ok], o["dneg"][i][ok]
        thr = o["d_pos"][i] + margin64(margin)
        if np.any(np.abs(np.sqrt(dn) - thr) <= band(np.sqrt(dn)) + band(o["d_pos"][i])):
            hit = True
        n = int(o["neg_cnt"][i])
        e = vr.eps_dist(dn)
        if n > 1 and np.any(np.diff(dn[:n]) <= e[:n - 1] + e[1:n]):
            hit = True
        if n == nNeg and len(dn) > n and dn[n] - dn[n - 1] <= 2 * max(ek[i, rows[:n + 1]].max(), e[n]):
            hit = True
        if len(dn) == o["dneg"].shape[1] and n > 0 and dn[-1] - dn[n - 1] <= 2 * ek[i, rows].max():
            hit = True                                   # a violator near the K-th boundary of the key ranking
        bad += hit
    return bad


def classes(o, nNeg):
    """(queries without a positive, with neg_cnt 0, with a partial list, with a full list)."""
    has = o["pos_idx"] >= 0
    c = o["neg_cnt"]
    return int((~has).sum()), int((has & (c == 0)).sum()), int((has & (c > 0) & (c < nNeg)).sum()), int((has & (c == nNeg)).sum())


# ---- masked search contract: vpr_ref.check_contract on the member rows of each query -----------------------------------
def check_masked_contract(D, I, db, q, member, k, split, label):
    """The set contract of kp2d_vpr_search_masked against float64: query i's answer must be kp2d_vpr_search's contract on
    the database made of its member rows alone.  -> uses of the 2 eps band."""
    D, I = np.asarray(D), np.asarray(I)
    d64 = vr.distances64(db, q)
    used = 0
    for i in range(len(q)):
        rows = np.flatnonzero(member[i])
        if len(rows) == 0:
            assert np.all(I[i] == -1) and np.all(D[i] == np.float32(np.finfo(np.float32).max)), (label, i, "padding")
            continue
        got = I[i]
        assert np.all(np.isin(got[got >= 0], rows)), (label, i, "row outside the mask")
        local = np.where(got >= 0, np.searchsorted(rows, np.maximum(got, 0)), -1)[None]
        sub = d64[i:i + 1, rows]
        eps = vr.eps_set(db[rows], q[i:i + 1], sub, k, split)
        used += vr.check_contract(D[i:i + 1], local, sub, k, eps, f"{label}:q{i}")
    return used


# ---- the mining tests' inputs (shared by the CPU precondition test and the GPU comparison) ----------------------------
# (numDb, numQ, dim, route seed, descriptor seed).  Random Fourier descriptors at a length scale of 60 m; database noise 0.3,
# query noise spread over 0.05 ... 2.5 per query: a clean query keeps its negatives beyond the margin (neg_cnt = 0), a noisy
# one sees every distance near sqrt(2) and gets a full list.  Seeds chosen so that all four classes of `classes` occur and
# `exactness` is zero in both precisions and both rounds (tests/test_mining_cpu.py asserts all of it).
MINING_CASES = [(700, 150, 768, 1, 4), (300, 70, 1536, 2, 4)]
MINING_ARGS = dict(n_sample=200, nNeg=10, nNegFactor=10, margin=0.1, seed=1234)
_INPUTS = {}


def mining_inputs(numDb, numQ, dim, route_seed, desc_seed):
    """-> (struct, dbFeat, qFeat, pos_member, neg_member), computed once per case and shared (treat as read-only)."""
    key = (numDb, numQ, dim, route_seed, desc_seed)
    if key not in _INPUTS:
        import importlib
        syn = importlib.import_module("nano_vs_slam_amd.synthetic")
        st = syn.vpr_struct(numDb, numQ, route_seed)
        qnoise = np.random.default_rng(desc_seed).uniform(0.05, 2.5, numQ)
        dbFeat = syn.place_descriptors(st.utmDb, dim, desc_seed, 60.0, 0.3, noise_seed=0)
        qFeat = syn.place_descriptors(st.utmQ, dim, desc_seed, 60.0, qnoise, noise_seed=1)
        pos = radius_member(st.utmDb, st.utmQ, st.nonTrivPosDistSqThr ** 0.5)
        neg = radius_member(st.utmDb, st.utmQ, st.posDistThr, invert=True)
        _INPUTS[key] = (st, dbFeat, qFeat, pos, neg)
    return _INPUTS[key]


_ROUNDS = {}


def mining_rounds(case):
    """The oracle's two rounds of a case: round 0 without a cache, round 1 with round 0's (kept where neg_cnt = 0, i.e.
    still empty).  -> (o0, cache1 [nq, nNeg] int32, o1)"""
    if case not in _ROUNDS:
        st, dbFeat, qFeat, pos, neg = mining_inputs(*case)
        a = MINING_ARGS
        o0 = mine_oracle(dbFeat, qFeat, pos, neg, None, a["n_sample"], a["nNeg"], a["nNegFactor"], a["margin"], a["seed"], 0)
        cache = np.where((o0["neg_cnt"] > 0)[:, None], o0["neg_idx"], -1).astype(np.int32)
        o1 = mine_oracle(dbFeat, qFeat, pos, neg, cache, a["n_sample"], a["nNeg"], a["nNegFactor"], a["margin"], a["seed"], 1)
        _ROUNDS[case] = (o0, cache, o1)
    return _ROUNDS[case]
