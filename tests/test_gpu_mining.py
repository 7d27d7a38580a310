"""Triplet mining on the MI355X (csrc/mining.hip, the masked search of csrc/vpr.hip, nano_vs_slam_amd.mining) against
sklearn and the float64 oracle of tests/mining_ref.py.  The masked search's set contract records its uses of the 2 eps band
through conftest.note_boundary_exempt; the mining comparison is exact (its inputs' preconditions: test_mining_cpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

import mining_ref as mr
import vpr_ref as vr
from conftest import note_boundary_exempt, product_model
from nano_vs_slam_amd import _lib, mining, synthetic
from nano_vs_slam_amd._dev import ptr, stream
from nano_vs_slam_amd.vpr import FlatL2Index, evaluate_global_descriptor, recall_at_n

pytestmark = pytest.mark.gpu
PRECS = ["f16x3", "fp32"]
FLT_MAX = np.float32(np.finfo(np.float32).max)
ERR_ARG, ERR_UNSUPPORTED = -1, -2


def unit(rng, n, dim):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def words(member, dirty=False):
    """bool [nq, ndb] -> device mask words; dirty: the bits at or past ndb set (they must be ignored)."""
    w = mining.pack_mask(member)
    ndb = member.shape[1]
    if dirty and ndb % 32:
        w[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(ndb % 32)
    return torch.from_numpy(w.view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bytes(a, b):
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    return torch.equal(bits(a), bits(b))


# ---- 1. radius ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numDb,numQ,seed", [(700, 150, 1), (300, 70, 2), (37, 1, 3), (130, 65, 4)])
def test_radius_equals_sklearn(numDb, numQ, seed):
    from sklearn.neighbors import NearestNeighbors
    st = synthetic.vpr_struct(numDb, numQ, seed)
    knn = NearestNeighbors(n_jobs=1).fit(st.utmDb)
    W = (numDb + 31) // 32
    for radius in (10, 25):
        assert mr.radius_gap(st.utmDb, st.utmQ, radius) >= 1e-6
        ref = knn.radius_neighbors(st.utmQ, radius=radius, return_distance=False)
        for invert in (False, True):
            want = [np.setdiff1d(np.arange(numDb), r) if invert else np.sort(r) for r in ref]
            rm = mining.radius_neighbors(st.utmDb, st.utmQ, radius, invert=invert)
            assert rm.mask.shape == (numQ, W) and rm.mask.dtype == torch.int32 and rm.count.dtype == torch.int32
            w = host(rm.mask).view(np.uint32)
            member = mining.unpack_mask(w, numDb)
            assert np.array_equal(w, mr.pack_bits(member))               # bits at or past ndb are zero
            assert np.array_equal(host(rm.count), [len(x) for x in want])
            lims, idx = rm.lists()
            assert isinstance(idx, np.ndarray) and idx.dtype == np.int64 and lims.dtype == np.int64 and lims[0] == 0
            for i in range(numQ):
                assert np.array_equal(np.flatnonzero(member[i]), want[i]), (radius, invert, i)
                assert np.array_equal(idx[lims[i]:lims[i + 1]], want[i]), (radius, invert, i)
    # device tensors in -> device tensors out, the same bits
    rt = mining.radius_neighbors(torch.from_numpy(st.utmDb).cuda(), torch.from_numpy(st.utmQ).cuda(), 25, invert=True)
    lims_t, idx_t = rt.lists()
    assert idx_t.is_cuda and lims_t.is_cuda and torch.equal(rt.mask, rm.mask) and np.array_equal(host(idx_t), idx)


def test_radius_extremes_and_lists_check():
    st = synthetic.vpr_struct(130, 65, 4)
    utmQ = st.utmQ.copy()
    utmQ[3] += 1e5                                               # a query with no neighbour
    rm = mining.radius_neighbors(st.utmDb, utmQ, 25)
    assert int(rm.count[3]) == 0 and not host(rm.mask)[3].any()
    every = mining.radius_neighbors(st.utmDb, utmQ, 1e7)         # a radius covering every row
    assert np.all(host(every.count) == 130)
    assert np.array_equal(host(every.mask).view(np.uint32), mr.pack_bits(np.ones((65, 130), bool)))
    none = mining.radius_neighbors(st.utmDb, utmQ, 1e7, invert=True)
    assert not host(none.mask).any() and not host(none.count).any() and len(none.lists()[1]) == 0
    # lims that disagree with a query's popcount: KP2D_ERR_ARG, nothing written outside the spans
    lims = torch.zeros(66, dtype=torch.int64, device="cuda")
    lims[1:] = torch.cumsum(rm.count, 0)
    lims[10:] += 1
    total = int(lims[-1])
    idx = torch.full((total,), -7, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = _lib.load().kp2d_mask_lists(ptr(rm.mask), 65, 130, ptr(lims), ptr(idx), total, ptr(status), stream(idx.device))
    assert rc == ERR_ARG
    with pytest.raises(RuntimeError):
        mining.radius_neighbors(torch.from_numpy(st.utmDb), torch.from_numpy(utmQ), 25)      # CPU tensors raise


class _Places(torch.utils.data.Dataset):
    """numDb frames along a line, then queries that are noisy copies of database frames taken a few metres beside them;
    the ground truth comes from the positions alone."""

    def __init__(self, num_db=24, num_q=10, H=64, W=96):
        rng = np.random.default_rng(0)
        self.frames = rng.uniform(0, 1, (num_db + num_q, 3, H, W)).astype(np.float32)
        src = rng.integers(0, num_db, num_q)
        for i, s in enumerate(src):
            self.frames[num_db + i] = np.clip(self.frames[s] + rng.normal(0, 0.05, (3, H, W)), 0, 1)
        utmDb = np.stack([585000.0 + 20.0 * np.arange(num_db), np.full(num_db, 4477000.0)], 1)
        utmQ = utmDb[src] + rng.uniform(-3, 3, (num_q, 2))
        utmQ[-1] += 5000.0                                        # a query without positives
        self.dbStruct = synthetic.vpr_struct(1, 1, 0)
        self.dbStruct.utmDb, self.dbStruct.utmQ, self.dbStruct.numDb, self.dbStruct.numQ = utmDb, utmQ, num_db, num_q

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return torch.from_numpy(self.frames[i]), i

    def getPositives(self):
        return mining.get_positives(self.dbStruct.utmDb, self.dbStruct.utmQ, self.dbStruct.posDistThr)


def test_get_positives_feeds_evaluation():
    from sklearn.neighbors import NearestNeighbors
    ds = _Places()
    gt = ds.getPositives()
    ref = NearestNeighbors(n_jobs=1).fit(ds.dbStruct.utmDb).radius_neighbors(ds.dbStruct.utmQ, radius=25, return_distance=False)
    assert len(gt) == len(ref) == 10 and len(gt[-1]) == 0 and all(len(g) in (1, 2, 3) for g in gt[:-1])
    for a, b in zip(gt, ref):
        assert np.array_equal(a, np.sort(b))
    model, _ = product_model("S", False, 28)
    res = evaluate_global_descriptor(model, ds, batch_size=4, device="cuda:0", num_workers=0)
    with torch.no_grad():
        v = host(model(torch.from_numpy(ds.frames).cuda())["vlad"].reshape(len(ds), -1))
    _, pred = vr.topk64(vr.distances64(v[:24], v[24:]), 20)
    want = recall_at_n(pred, ref, 10)
    for key in ("Recall", "AUC", "MatchRatio"):
        for n in (1, 5, 10, 20):
            assert res[key][n] == want[key][n], (key, n)


# ---- 2. masked search: exact identities ----------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("dim,ndb,nq,k", [(768, 700, 150, 100), (1536, 517, 1, 1), (4096, 300, 70, 10), (1552, 130, 65, 1024)])
def test_masked_identities(prec, dim, ndb, nq, k):
    rng = np.random.default_rng(dim + ndb + nq + k)
    db, q = unit(rng, ndb, dim), unit(rng, nq, dim)
    ix = FlatL2Index(dim, precision=prec)
    ix.add(db)
    qt = torch.from_numpy(q).cuda()
    D, I = ix.search(qt, k)
    # all ones (with the bits past ndb set too) is the plain search, bit for bit
    Dm, Im = ix.search(qt, k, mask=words(np.ones((nq, ndb), bool), dirty=True))
    assert torch.equal(Dm, D) and torch.equal(Im, I)
    if k > ndb:
        assert bool((I[:, ndb:] == -1).all()) and bool((D[:, ndb:] == float(FLT_MAX)).all())
    # a prefix mask is limit
    lim = rng.integers(0, ndb + 1, nq)
    lim[0] = ndb // 2
    Dl, Il = ix.search(qt, k, limit=lim)
    Dp, Ip = ix.search(qt, k, mask=words(np.arange(ndb)[None, :] < lim[:, None]))
    assert torch.equal(Dp, Dl) and torch.equal(Ip, Il)
    # a query's answer does not depend on its company: alone, in the batch, or with every other mask empty (tile skip)
    member = rng.random((nq, ndb)) < 0.3
    j = nq // 2
    member[j] = False
    member[j, rng.integers(0, ndb, 3)] = True                    # three rows: most of its tiles are empty
    Da, Ia = ix.search(qt, k, mask=words(member))
    D1, I1 = ix.search(qt[j:j + 1], k, mask=words(member[j:j + 1]))
    only = np.zeros_like(member)
    only[j] = member[j]
    Dz, Iz = ix.search(qt, k, mask=words(only))
    assert torch.equal(Da[j], D1[0]) and torch.equal(Ia[j], I1[0]) and torch.equal(Dz[j], D1[0]) and torch.equal(Iz[j], I1[0])
    rows = np.flatnonzero(member[j])
    if len(rows) <= k:
        assert sorted(host(I1[0][I1[0] >= 0]).tolist()) == rows.tolist()
    others = np.arange(nq) != j
    assert bool((Iz[torch.from_numpy(others).cuda()] == -1).all())
    # a RowMask, a uint32 view and numpy queries are accepted; limit and mask together are not
    rm = mining.RowMask(words(member), torch.from_numpy(member.sum(1).astype(np.int32)).cuda(), ndb)
    Dr, Ir = ix.search(q, k, mask=rm)
    assert np.array_equal(Dr, host(Da)) and np.array_equal(Ir, host(Ia))
    with pytest.raises(ValueError):
        ix.search(qt, k, limit=lim, mask=rm)
    with pytest.raises(ValueError):
        ix.search(qt, k, mask=words(member)[:, :-1].contiguous() if member.shape[1] > 32 else words(member)[:0])


# ---- 3. masked search: the set contract against float64 --------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_masked_contract(prec):
    rng = np.random.default_rng(31)
    dim, ndb, nq, k = 768, 700, 40, 20
    db, q = unit(rng, ndb, dim), unit(rng, nq, dim)
    q[:10] = db[rng.integers(0, ndb, 10)] + 0.3 * q[:10]
    db[5] *= np.float32(2.0 ** 45)                               # rows outside the range guard: their tiles take fp32 products
    db[300] *= np.float32(2.0 ** -45)
    member = rng.random((nq, ndb)) < 0.5
    member[20:] = rng.random((nq - 20, ndb)) < 0.01
    member[0] = False                                            # an empty mask: every slot is padding
    member[1] = False
    member[1, 128:256] = True                                    # one 128-row tile
    member[2] = False
    member[2, 640:] = True                                       # the last, partial tile
    member[3] = False
    member[3, 256:384] = rng.random(128) < 0.5                   # the tile holding guard row 300
    member[3, 300] = True
    member[4] = False
    member[4, :128] = True                                       # the tile holding guard row 5
    ix = FlatL2Index(dim, precision=prec)
    ix.add(db)
    D, I = ix.search(q, k, mask=words(member, dirty=True))
    assert np.all(I[0] == -1) and np.all(D[0] == FLT_MAX)
    assert np.all(I[20:][np.arange(k)[None, :] >= member[20:].sum(1)[:, None]] == -1)      # sparse masks: padded lists
    used = mr.check_masked_contract(D, I, db, q, member, k, prec == "f16x3", f"{prec}:masked")
    note_boundary_exempt(f"vpr-masked:{prec}", used, int((I >= 0).sum()))


# ---- 4. sampling -------------------------------------------------------------------------------------------------------------
def _sampling_inputs():
    rng = np.random.default_rng(41)
    dim, ndb, nq, n_neg = 64, 300, 70, 10
    db, q = unit(rng, ndb, dim), unit(rng, nq, dim)
    pos = rng.random((nq, ndb)) < 0.02
    neg = rng.random((nq, ndb)) < 0.6
    neg[0] = False
    neg[0, 17] = True                                            # nPot = 1
    neg[1] = True                                                # nPot = ndb
    neg[2] = False                                               # nPot = 0: the cache rows alone
    cache = np.full((nq, n_neg), -1, np.int32)
    cache[:, :3] = rng.integers(0, ndb, (nq, 3))                 # three cached rows and -1 padding
    cache[5] = -1
    return db, q, pos, neg, cache, n_neg


@pytest.mark.parametrize("n_sample", [1, 200])
def test_sampling_equals_oracle(n_sample):
    db, q, pos, neg, cache, n_neg = _sampling_inputs()
    ix = FlatL2Index(db.shape[1])
    ix.add(db)
    qt, ct = torch.from_numpy(q).cuda(), torch.from_numpy(cache).cuda()
    args = dict(n_sample=n_sample, n_neg=n_neg, n_neg_factor=4, margin=0.1, seed=77, want_cand=True)
    out = mining.mine_round(ix, qt, words(pos), words(neg, dirty=True), ct, round=3, **args)
    o = mr.mine_oracle(db, q, pos, neg, cache, n_sample, n_neg, 4, 0.1, 77, 3)
    cand = host(out[4]).view(np.uint32)
    assert np.array_equal(cand, mr.pack_bits(o["cand"]))
    assert 1 <= o["cand"][2].sum() <= 3 and o["cand"][0].sum() <= 4 and (n_sample == 1 or o["cand"][1].sum() > 100)
    again = mining.mine_round(ix, qt, words(pos), words(neg, dirty=True), ct, round=3, **args)
    for a, b in zip(out, again):                                 # the same (seed, round): the same bytes
        assert same_bytes(a, b)
    other = mining.mine_round(ix, qt, words(pos), words(neg, dirty=True), ct, round=4, **args)
    assert not torch.equal(other[4], out[4])
    # a subset mined under its query numbers draws what the whole set draws
    sub = np.array([1, 9, 30, 69])
    st = torch.from_numpy(sub).cuda()
    part = mining.mine_round(ix, qt[st], words(pos[sub]), words(neg[sub]), ct[st].contiguous(), qid=st, round=3, **args)
    for a, b in zip(out, part):
        a = a[st]
        assert same_bytes(a, b)


def test_sampling_large_database():
    """More than 131072 rows: the popcount prefix in LDS is over groups of several mask words (another path of the draw)."""
    rng = np.random.default_rng(43)
    dim, ndb, nq, n_neg = 16, 2 * 131072 + 77, 3, 10
    db, q = unit(rng, ndb, dim), unit(rng, nq, dim)
    pos = np.zeros((nq, ndb), bool)
    pos[:, rng.integers(0, ndb, 5)] = True
    neg = rng.random((nq, ndb)) < 0.5
    neg[1] = True
    neg[2] = False
    neg[2, [ndb - 1, 131072, 5]] = True
    ix = FlatL2Index(dim)
    ix.add(db)
    out = mining.mine_round(ix, torch.from_numpy(q).cuda(), words(pos), words(neg, dirty=True), None, n_sample=200, n_neg=n_neg,
                            n_neg_factor=10, margin=0.1, seed=7, round=2, want_cand=True)
    want = np.zeros((nq, ndb), bool)
    for i in range(nq):
        want[i, mr.draws(neg[i], 7, 2, i, 200)] = True
    assert np.array_equal(mining.unpack_mask(host(out[4]), ndb), want)
    assert want[2].sum() == 3 and want[0].sum() > 190
    assert np.all(np.isin(host(out[0]), np.flatnonzero(pos[0])))


# ---- 5. mining end to end ------------------------------------------------------------------------------------------------------
def _check_round(o, got, nNeg, label):
    pos_idx, neg_idx, neg_cnt, d_pos = (host(t) for t in got)
    assert pos_idx.dtype == np.int64 and neg_idx.dtype == np.int32 and neg_cnt.dtype == np.int32 and d_pos.dtype == np.float32
    assert np.array_equal(pos_idx, o["pos_idx"]), label
    assert np.array_equal(neg_cnt, o["neg_cnt"]), label
    assert np.array_equal(neg_idx, o["neg_idx"]), label
    has = o["pos_idx"] >= 0
    assert np.all(np.isnan(d_pos[~has])) and np.all(neg_cnt[~has] == 0) and np.all(neg_idx[~has] == -1)
    d = o["d_pos"][has]
    assert np.all(np.abs(d_pos[has].astype(np.float64) - d) <= mr.band(d) + 2.0 ** -24 * d), label


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", mr.MINING_CASES)
def test_mining_end_to_end(case, prec):
    st, dbFeat, qFeat, pos, neg = mr.mining_inputs(*case)
    a = mr.MINING_ARGS
    nNeg = a["nNeg"]
    o0, cache1, o1 = mr.mining_rounds(case)
    # preconditions, on the oracle: all four classes occur and nothing sits within rounding of a decision
    for o in (o0, o1):
        assert min(mr.classes(o, nNeg)) > 0
        assert mr.exactness(o, dbFeat, qFeat, pos, nNeg, a["margin"], prec == "f16x3") == 0
    miner = mining.TripletMiner(st.utmDb, st.utmQ, st.posDistThr, st.nonTrivPosDistSqThr, nNegSample=a["n_sample"], nNeg=nNeg,
                                margin=a["margin"], nNegFactor=a["nNegFactor"], seed=a["seed"], precision=prec)
    assert np.array_equal(miner.queries, np.flatnonzero(pos.any(1)))
    assert all(np.array_equal(x, np.flatnonzero(m)) for x, m in zip(miner.nontrivial_positives, pos))
    assert all(np.array_equal(x, np.flatnonzero(m)) for x, m in zip(miner.potential_negatives, neg))
    assert miner.negCache.shape == (st.numQ, nNeg) and miner.negCache.dtype == torch.int32 and bool((miner.negCache == -1).all())
    db_t, q_t = torch.from_numpy(dbFeat).cuda(), torch.from_numpy(qFeat).cuda()
    got0 = miner.mine(db_t, q_t, want_cand=True)
    _check_round(o0, got0, nNeg, f"{case}:{prec}:round0")
    assert np.array_equal(host(miner.last_cand).view(np.uint32), mr.pack_bits(o0["cand"]))
    assert np.array_equal(host(miner.negCache), cache1) and miner.round == 1          # replaced only where neg_cnt > 0
    trip = list(miner.triplets())
    keep = np.flatnonzero(o0["neg_cnt"] > 0)
    assert [t[0] for t in trip] == keep.tolist()
    assert all(t[1] == o0["pos_idx"][i] and t[2:] == o0["neg_idx"][i, :o0["neg_cnt"][i]].tolist() for t, i in zip(trip, keep))
    got1 = miner.mine(db_t, q_t, want_cand=True)
    _check_round(o1, got1, nNeg, f"{case}:{prec}:round1")
    cand1 = mining.unpack_mask(host(miner.last_cand), st.numDb)
    assert np.array_equal(cand1, o1["cand"])
    for i in range(st.numQ):                                      # last round's negatives are candidates again
        assert cand1[i, cache1[i][cache1[i] >= 0]].all()
    cache2 = np.where((o1["neg_cnt"] > 0)[:, None], o1["neg_idx"], cache1)
    assert np.array_equal(host(miner.negCache), cache2)
    # the reference's cache layout, queries after the database, and a subset of queries
    single = mining.TripletMiner(st.utmDb, st.utmQ, st.posDistThr, st.nonTrivPosDistSqThr, nNegSample=a["n_sample"], nNeg=nNeg,
                                 margin=a["margin"], nNegFactor=a["nNegFactor"], seed=a["seed"], precision=prec)
    both = single.mine(torch.cat([db_t, q_t]))
    for x, y in zip(both, got0):
        assert same_bytes(x, y)
    single.round = 0
    single.negCache.fill_(-1)
    sub = miner.queries[::7]
    part = single.mine(db_t, q_t, queries=sub)
    st_idx = torch.from_numpy(sub).cuda()
    for x, y in zip(part, got0):
        y = y[st_idx]
        assert same_bytes(x, y)
    with pytest.raises(RuntimeError):
        single.mine(torch.from_numpy(dbFeat), torch.from_numpy(qFeat))


# ---- 6. scratch and arguments ----------------------------------------------------------------------------------------------------
def test_scratch_and_arguments():
    lib = _lib.load()
    rng = np.random.default_rng(61)
    dim, ndb, nq, n_neg, fac = 64, 200, 9, 4, 5
    db, q = unit(rng, ndb, dim), unit(rng, nq, dim)
    ix = FlatL2Index(dim)
    ix.add(db)
    qt = torch.from_numpy(q).cuda()
    pos, neg = words(rng.random((nq, ndb)) < 0.05), words(rng.random((nq, ndb)) < 0.7)
    dev = qt.device
    pos_idx = torch.empty(nq, dtype=torch.int64, device=dev)
    neg_idx = torch.empty(nq, n_neg, dtype=torch.int32, device=dev)
    neg_cnt = torch.empty(nq, dtype=torch.int32, device=dev)
    d_pos = torch.empty(nq + 1, dtype=torch.float32, device=dev)
    need = int(lib.kp2d_vpr_mine_scratch_bytes(nq, ndb, dim, n_neg, fac))
    assert need > 0
    scratch = torch.empty(need + 64, dtype=torch.uint8, device=dev)

    def call(dim_=dim, n_neg_=n_neg, fac_=fac, q_=None, scratch_=None, nbytes=need, pos_=None, d_pos_=None):
        return lib.kp2d_vpr_mine(ptr(ix._p), ptr(ix._x), ndb, dim_, ptr(qt) if q_ is None else q_, nq, None,
                                 ptr(pos) if pos_ is None else pos_, ptr(neg), None, 50, n_neg_, fac_, 0.1, 5, 0, 0, ptr(pos_idx),
                                 ptr(neg_idx), ptr(neg_cnt), ptr(d_pos) if d_pos_ is None else d_pos_, None,
                                 ptr(scratch) if scratch_ is None else scratch_, nbytes, stream(dev))

    assert call() == 0                                           # exactly kp2d_vpr_mine_scratch_bytes
    torch.cuda.synchronize()
    first = (host(pos_idx).copy(), host(neg_idx).copy(), host(neg_cnt).copy())
    assert call(nbytes=need - 1) == ERR_ARG and b"scratch" in lib.kp2d_last_error()
    assert lib.kp2d_vpr_mine_scratch_bytes(nq, ndb, dim, 33, 32) == 0 and call(n_neg_=33, fac_=32) == ERR_ARG       # 1056 > 1024
    assert lib.kp2d_vpr_mine_scratch_bytes(nq, ndb, dim, 32, 32) > 0
    assert lib.kp2d_vpr_mine_scratch_bytes(nq, ndb, 24, n_neg, fac) == 0 and call(dim_=24) == ERR_UNSUPPORTED
    off = lambda t, b: ctypes.c_void_p(t.data_ptr() + b)
    assert call(q_=off(qt, 4)) == ERR_ARG and call(scratch_=off(scratch, 8), nbytes=need) == ERR_ARG
    assert call(pos_=off(pos, 2)) == ERR_ARG and call(d_pos_=off(d_pos, 2)) == ERR_ARG
    assert call() == 0
    torch.cuda.synchronize()
    assert all(np.array_equal(x, y) for x, y in zip(first, (host(pos_idx), host(neg_idx), host(neg_cnt))))
    # the other entry points
    xy = torch.zeros(4, 2, dtype=torch.float64, device=dev)
    m = torch.zeros(4, 1, dtype=torch.int32, device=dev)
    c = torch.zeros(4, dtype=torch.int32, device=dev)
    assert lib.kp2d_geo_radius_mask(ptr(xy), 4, ptr(xy), 4, -1.0, 0, ptr(m), ptr(c), stream(dev)) == ERR_ARG
    assert lib.kp2d_geo_radius_mask(ptr(xy), 4, ptr(xy), 4, float("nan"), 0, ptr(m), ptr(c), stream(dev)) == ERR_ARG
    assert lib.kp2d_geo_radius_mask(ptr(xy), 4, ptr(xy), 4, 1.0, 2, ptr(m), ptr(c), stream(dev)) == ERR_ARG
    assert lib.kp2d_geo_radius_mask(off(xy, 4), 3, ptr(xy), 4, 1.0, 0, ptr(m), ptr(c), stream(dev)) == ERR_ARG
    D = torch.empty(nq, 3, dtype=torch.float32, device=dev)
    I = torch.empty(nq, 3, dtype=torch.int64, device=dev)
    sb = int(lib.kp2d_vpr_scratch_bytes(nq, ndb, dim, 3))
    sc = torch.empty(max(sb, 256), dtype=torch.uint8, device=dev)
    masked = lambda mk: lib.kp2d_vpr_search_masked(ptr(ix._p), ptr(ix._x), ndb, dim, ptr(qt), nq, mk, 3, 0, ptr(D), ptr(I), ptr(sc),
                                                   sc.numel(), stream(dev))
    assert masked(None) == ERR_ARG and masked(off(pos, 2)) == ERR_ARG and masked(ptr(pos)) == 0
    with pytest.raises(RuntimeError):
        mining.mine_round(ix, torch.from_numpy(q), pos, neg)     # CPU tensors raise
    with pytest.raises(RuntimeError):
        ix.search(qt, 3, mask=torch.zeros(nq, (ndb + 31) // 32, dtype=torch.int32))
