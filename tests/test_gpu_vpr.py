"""FlatL2Index (csrc/vpr.hip) on the MI355X against float64 numpy, in both precisions, with the bound of
tests/vpr_ref.py.  Every comparison records its uses of the 2 eps band through conftest.note_boundary_exempt."""
import numpy as np
import pytest
import torch

import vpr_ref as vr
from conftest import note_boundary_exempt, product_model
from nano_vs_slam_amd.vpr import FlatL2Index, evaluate_global_descriptor, recall_at_n

pytestmark = pytest.mark.gpu
PRECS = ["f16x3", "fp32"]


def unit(rng, n, dim):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def run(db, q, k, prec, label, limit=None):
    ix = FlatL2Index(db.shape[1], precision=prec)
    ix.add(db)
    D, I = ix.search(q, k, limit=limit)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == (len(q), k)
    d64 = vr.distances64(db, q)
    eps = vr.eps_set(db, q, d64, k, prec == "f16x3", limit)
    used = vr.check_contract(D, I, d64, k, eps, label, limit)
    note_boundary_exempt(f"vpr:{label}", used, int((I >= 0).sum()))
    return D, I


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("dim,n,nq,k", [(768, 1000, 300, 20), (1536, 517, 1, 100), (4096, 2999, 1, 20),
                                        (4096, 130, 200, 1), (768, 700, 3, 1024), (1536, 37, 5, 100)])
def test_contract(prec, dim, n, nq, k):
    rng = np.random.default_rng(dim + n + nq + k)
    db = unit(rng, n, dim)
    q = unit(rng, nq, dim)
    q[: nq // 2] = db[rng.integers(0, n, nq // 2)] + 0.3 * q[: nq // 2]      # some queries near database rows
    run(db, q, k, prec, f"{prec}:{dim}x{n}x{nq}:k{k}")


@pytest.mark.parametrize("prec", PRECS)
def test_duplicates_and_self_match(prec):
    rng = np.random.default_rng(5)
    db = unit(rng, 300, 1536)
    db[[40, 7, 250]] = db[120]
    q = np.stack([db[120], db[3], unit(rng, 1, 1536)[0]])
    D, I = run(db, q, 8, prec, f"{prec}:duplicates")
    assert I[0, :4].tolist() == [7, 40, 120, 250] and np.all(D[0, :4] == 0)
    assert I[1, 0] == 3 and D[1, 0] == 0 and np.all(D >= 0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", ["1e5", "1e-6", "gem", "guard"])
def test_range(prec, kind):
    rng = np.random.default_rng(11)
    if kind == "gem":        # GeM-like: non-negative, unnormalised, norms spread over two decades
        db = (np.abs(rng.standard_normal((900, 768))) * rng.uniform(0.1, 10, (900, 1))).astype(np.float32)
        q = (np.abs(rng.standard_normal((40, 768))) * rng.uniform(0.1, 10, (40, 1))).astype(np.float32)
    else:
        s = {"1e5": 1e5, "1e-6": 1e-6, "guard": 1.0}[kind]
        db = unit(rng, 900, 768) * np.float32(s)
        q = unit(rng, 40, 768) * np.float32(s)
        if kind == "guard":  # rows outside [2^-40, 2^40): their 128-row blocks take the fp32 products
            db[5] *= np.float32(2.0 ** 45)
            db[300] *= np.float32(2.0 ** -45)
    run(db, q, 20, prec, f"{prec}:range-{kind}")


@pytest.mark.parametrize("prec", PRECS)
def test_bit_identity(prec):
    rng = np.random.default_rng(21)
    db = unit(rng, 5000, 1536)
    q = unit(rng, 150, 1536)
    ix = FlatL2Index(1536, precision=prec)
    ix.add(db)
    D, I = ix.search(q, 20)
    Da, Ia = ix.search(q[:70], 20)
    Db, Ib = ix.search(q[70:], 20)
    assert np.array_equal(D, np.concatenate([Da, Db])) and np.array_equal(I, np.concatenate([Ia, Ib]))
    D1, I1 = ix.search(q[9:10], 20)                      # one query: the sliced path
    assert np.array_equal(D1, D[9:10]) and np.array_equal(I1, I[9:10])
    ix3 = FlatL2Index(1536, precision=prec)
    for part in (db[:1000], db[1000:1001], db[1001:]):
        ix3.add(part)
    assert ix3.ntotal == 5000
    D3, I3 = ix3.search(q, 20)
    assert np.array_equal(D3, D) and np.array_equal(I3, I)
    m = 2345
    ixm = FlatL2Index(1536, precision=prec)
    ixm.add(db[:m])
    Dm, Im = ixm.search(q, 20)
    Dl, Il = ix.search(q, 20, limit=np.full(len(q), m))
    assert np.array_equal(Dm, Dl) and np.array_equal(Im, Il)
    lim = rng.integers(-5, 5000, len(q))
    lim[:3] = [0, -1, 19]
    Dl, Il = ix.search(q, 20, limit=lim)
    d64 = vr.distances64(db, q)
    used = vr.check_contract(Dl, Il, d64, 20, vr.eps_set(db, q, d64, 20, prec == "f16x3", lim), f"{prec}:limit", lim)
    note_boundary_exempt(f"vpr:{prec}:limit", used, int((Il >= 0).sum()))
    # device tensors in -> device tensors out
    Dt, It = ix.search(torch.from_numpy(q).cuda(), 20)
    assert Dt.is_cuda and It.dtype == torch.int64 and np.array_equal(Dt.cpu().numpy(), D)


class _Db:
    def __init__(self, num_db, num_q):
        self.numDb, self.numQ = num_db, num_q


class SyntheticPlaces(torch.utils.data.Dataset):
    """In-memory frames: numDb database frames, then numQ queries that are noisy copies of hand-picked database frames."""

    def __init__(self, seed=0, num_db=24, num_q=10, H=64, W=96):
        rng = np.random.default_rng(seed)
        self.frames = rng.uniform(0, 1, (num_db + num_q, 3, H, W)).astype(np.float32)
        self.src = rng.integers(0, num_db, num_q)
        for i, s in enumerate(self.src):
            self.frames[num_db + i] = np.clip(self.frames[s] + rng.normal(0, 0.05, (3, H, W)), 0, 1)
        self.dbStruct = _Db(num_db, num_q)
        self.pos = [np.array(sorted({int(s), int((s + 1) % num_db)})) for s in self.src]
        self.pos[-1] = np.array([], np.int64)            # a query without positives

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return torch.from_numpy(self.frames[i]), i

    def getPositives(self):
        return self.pos


def test_end_to_end_product_model():
    model, _ = product_model("S", False, 28)
    ds = SyntheticPlaces()
    x = torch.from_numpy(ds.frames).cuda()
    with torch.no_grad():
        vlad = model(x)["vlad"].reshape(len(ds), -1).contiguous()
    v = vlad.cpu().numpy()
    for prec in PRECS:
        ix = FlatL2Index(v.shape[1], precision=prec)
        ix.add(vlad)
        D, I = ix.search(vlad, 5)
        assert torch.equal(I[:, 0].cpu(), torch.arange(len(ds))) and bool((D[:, 0] == 0).all()), prec
    for prec in PRECS:
        res = evaluate_global_descriptor(model, ds, batch_size=4, device="cuda:0", num_workers=0, precision=prec)
        nd = ds.dbStruct.numDb
        _, pred = vr.topk64(vr.distances64(v[:nd], v[nd:]), 20)
        ref = recall_at_n(pred, ds.getPositives(), ds.dbStruct.numQ)
        for key in ("Recall", "AUC", "MatchRatio"):
            for n in (1, 5, 10, 20):
                a, b = res[key][n], ref[key][n]
                assert (np.isnan(a) and np.isnan(b)) or a == b, (prec, key, n, a, b)
