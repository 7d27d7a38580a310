"""Device k-means (csrc/kmeans.hip, nano_vs_slam_amd.clustering) on the MI355X against float64 numpy, in both
precisions, with the bounds of tests/kmeans_ref.py.  Assignments are compared through the search's set contract and
record their uses of the 2 eps band through conftest.note_boundary_exempt; the trajectory tests take no exemption."""
import functools

import numpy as np
import pytest
import torch

import kmeans_ref as kr
import vpr_ref as vr
from conftest import note_boundary_exempt, product_model
from nano_vs_slam_amd import clustering as cl
from nano_vs_slam_amd.clustering import KMEANS_NO_SPLIT, Kmeans, kmeans_step, kmeans_train
from nano_vs_slam_amd.vpr import PRECISIONS

pytestmark = pytest.mark.gpu
PRECS = ["f16x3", "fp32"]
U = kr.U


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(*ts):
    return [t.cpu().numpy() for t in ts]


def check_step(x, c, prec, label):
    """One step with KP2D_KMEANS_NO_SPLIT against float64: assignment contract, counts, centroid and objective bounds,
    empty clusters unchanged -> the host copies of the outputs."""
    k = len(c)
    cout, assign, dist, counts, obj = host(*kmeans_step(dev(x), dev(c), PRECISIONS[prec] | KMEANS_NO_SPLIT))
    d64 = vr.distances64(c, x)
    eps = vr.eps_set(c, x, d64, 1, prec == "f16x3")
    used = vr.check_contract(dist[:, None], assign[:, None], d64, 1, eps, label)
    print(f"{label}: {used} uses of the 2 eps band")
    note_boundary_exempt(f"kmeans:{label}", used, len(x))
    assert np.array_equal(counts, np.bincount(assign, minlength=k)) and counts.sum() == len(x)
    c64, _ = kr.means64(x, assign, k, c)
    bound = kr.centroid_bound(x, assign, k, c64)
    err = np.abs(cout.astype(np.float64) - c64)
    print(f"{label}: centroid error uses {float((err / np.maximum(bound, 1e-300)).max()):.3f} of its bound")
    assert np.all(err <= bound), (label, "centroid")
    assert np.array_equal(cout[counts == 0], c[counts == 0]), (label, "empty clusters must keep their centroid")
    dmin = d64.min(1)
    print(f"{label}: objective error {abs(float(obj[0]) - dmin.sum()):.3e}, bound {kr.obj_bound(dmin):.3e}")
    assert abs(float(obj[0]) - dmin.sum()) <= kr.obj_bound(dmin), (label, "objective")
    return cout, assign, dist, counts, obj


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n,d,k", [(1000, 16, 3), (4099, 64, 64), (2053, 128, 65), (257, 4096, 5), (64, 64, 64), (513, 32, 1),
                                   (777, 48, 32)])
def test_step_contract(prec, n, d, k):
    rng = np.random.default_rng(n + d + k)
    x = rng.standard_normal((n, d)).astype(np.float32)
    c = (x[rng.choice(n, k, replace=False)] + 0.3 * rng.standard_normal((k, d))).astype(np.float32)
    check_step(x, c, prec, f"{prec}:{n}x{d}x{k}")


@pytest.mark.parametrize("prec", PRECS)
def test_all_points_in_one_cluster(prec):
    """n = 4099 rows in one list: nine chunks of the sum kernel, partials added in chunk order."""
    rng = np.random.default_rng(3)
    x = (1.0 + 0.5 * rng.standard_normal((4099, 64))).astype(np.float32)
    c = np.empty((4, 64), np.float32)
    c[0], c[1], c[2], c[3] = 100.0, -100.0, 1.0, 200.0
    _, assign, _, counts, _ = check_step(x, c, prec, f"{prec}:one-cluster")
    assert counts.tolist() == [0, 0, 4099, 0] and np.all(assign == 2)


@pytest.mark.parametrize("prec", PRECS)
def test_ties_go_to_the_lower_index(prec):
    rng = np.random.default_rng(4)
    x = (0.1 * rng.standard_normal((100, 16))).astype(np.float32)
    x[:, 0] = 0.0                      # equidistant from +e0 and -e0, exactly, in every arithmetic involved
    x[90:95, 0], x[95:, 0] = 0.5, -0.5
    c = np.zeros((3, 16), np.float32)
    c[0] = 50.0
    c[1, 0], c[2, 0] = 1.0, -1.0
    _, assign, dist, counts, _ = host(*kmeans_step(dev(x), dev(c), PRECISIONS[prec] | KMEANS_NO_SPLIT))
    assert np.all(assign[:90] == 1) and np.all(assign[90:95] == 1) and np.all(assign[95:] == 2)
    assert counts.tolist() == [0, 95, 5]
    c[[1, 2]] = c[[2, 1]]              # the same two centroids the other way round: still the lower index
    _, assign, *_ = host(*kmeans_step(dev(x), dev(c), PRECISIONS[prec] | KMEANS_NO_SPLIT))
    assert np.all(assign[:90] == 1) and np.all(assign[90:95] == 2) and np.all(assign[95:] == 1)


@pytest.mark.parametrize("prec", PRECS)
def test_one_empty_cluster_is_split_from_one_donor(prec):
    rng = np.random.default_rng(5)
    centre = 4.0 * rng.standard_normal((3, 32))
    x = (centre[np.arange(600) % 3] + 0.2 * rng.standard_normal((600, 32))).astype(np.float32)
    c = np.concatenate([centre, np.full((1, 32), 300.0)]).astype(np.float32)
    flags, seed, it = PRECISIONS[prec], 99, 6
    mean, _, _, counts, _ = host(*kmeans_step(dev(x), dev(c), flags | KMEANS_NO_SPLIT, seed, it))
    got, _, _, counts2, _ = host(*kmeans_step(dev(x), dev(c), flags, seed, it))
    assert counts.tolist() == [200, 200, 200, 0] and np.array_equal(counts, counts2)
    changed = [j for j in range(3) if not np.array_equal(got[j], mean[j])]
    assert len(changed) == 1, "exactly one donor"
    cj = changed[0]
    _, _, pairs = kr.split_ref(mean, counts, seed, it)
    assert pairs == [(3, cj)], "the donor the restated draw picks"
    even = np.arange(32) % 2 == 0
    m64 = mean[cj].astype(np.float64)
    want_new = m64 * np.where(even, 1 + 1 / 1024, 1 - 1 / 1024)
    want_donor = m64 * np.where(even, 1 - 1 / 1024, 1 + 1 / 1024)
    assert np.all(np.abs(got[3] - want_new) <= 2 * U * np.abs(want_new))
    assert np.all(np.abs(got[cj] - want_donor) <= 2 * U * np.abs(want_donor))
    for j in range(3):
        if j != cj:
            assert np.array_equal(got[j], mean[j])
    # another (seed, iteration) is another draw, the same one the same split
    again = host(*kmeans_step(dev(x), dev(c), flags, seed, it))[0]
    assert np.array_equal(again, got)


@pytest.mark.parametrize("prec", PRECS)
def test_many_empty_clusters(prec):
    """5 distinct rows x 60 copies, k = 8, init = the first 8 points: rows 0-2 appear twice among the centroids, ties go
    to the lower index, so three clusters are empty in every iteration and are split from donors again and again.
    Bound of the final objective around 0 (the float64 objective of centroids that sit on their rows): a centroid is its
    row's mean (within the mean bound b) times at most three split factors (three empty clusters per iteration, each
    1 +- 1/1024), so per component it is within ((1 + 1/1024)^3 - 1) |r_j| + b_j of the row, and every distance within
    the sum of those squares, times (1 + 34 u) for the fp32 re-score."""
    rng = np.random.default_rng(6)
    rows = rng.standard_normal((5, 64)).astype(np.float32)
    x = np.tile(rows, (60, 1))
    cent, obj, assign, dist, counts = host(*kmeans_train(dev(x), dev(x[:8]), 10, PRECISIONS[prec], 5))
    assert np.all(np.isfinite(cent)) and np.all(np.isfinite(obj)) and np.all(np.isfinite(dist))
    assert counts.sum() == len(x) and int((counts > 0).sum()) == 5
    assert np.array_equal(counts, np.bincount(assign, minlength=8))
    per_comp = ((1 + 1 / 1024) ** 3 - 1) * np.abs(x.astype(np.float64)) + (kr.ALPHA + 2) * U * np.abs(x.astype(np.float64))
    bound = (per_comp ** 2).sum() * (1 + (kr.ALPHA + 2) * U)
    print(f"{prec}: final objective {float(obj[-1]):.3e}, bound {bound:.3e}")
    assert 0 <= obj[-1] <= bound


@functools.lru_cache(maxsize=None)
def trajectory(n, d, k, sigma):
    x, label = kr.blobs(n, d, k, sigma)
    return x, label, kr.lloyd64(x, x[:k], 10)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n,d,k,sigma", [(4099, 64, 64, 0.3), (1000, 16, 3, 0.3), (2053, 128, 65, 0.3), (4099, 64, 64, 0.6)])
def test_trajectory_on_blobs(prec, n, d, k, sigma):
    """Margins of the recipe are four orders above eps (tests/test_kmeans_cpu.py), so no exemption applies."""
    x, label, traj = trajectory(n, d, k, sigma)
    cent, obj, assign, dist, counts = host(*kmeans_train(dev(x), dev(x[:k]), 10, PRECISIONS[prec]))
    assert np.array_equal(assign, label)
    assert np.array_equal(counts, np.bincount(label, minlength=k))
    c64 = traj[-1][1]
    err = np.abs(cent.astype(np.float64) - c64)
    bound = kr.centroid_bound(x, label, k, c64)
    print(f"{prec}:{n}x{d}x{k}: centroid error uses {float((err / bound).max()):.3f} of its bound")
    assert np.all(err <= bound)
    for i in range(10):
        assert abs(float(obj[i]) - traj[i][2]) <= kr.obj_bound(traj[i][4]), (i, float(obj[i]), traj[i][2])


@pytest.mark.parametrize("prec", PRECS)
def test_bit_identity(prec):
    flags = PRECISIONS[prec]
    x, _, _ = trajectory(4099, 64, 64, 0.6)
    rng = np.random.default_rng(8)
    tiled = np.tile(rng.standard_normal((5, 64)).astype(np.float32), (60, 1))
    for data, init, niter in ((x, x[:64], 4), (tiled, tiled[:8], 4)):       # the second one splits in every iteration
        xd, c0 = dev(data), dev(init)
        a = kmeans_train(xd, c0, niter, flags, 11)
        b = kmeans_train(xd, c0, niter, flags, 11)
        for p, q in zip(a, b):
            assert torch.equal(p, q)
        c, objs = c0, []
        for i in range(niter):
            c, assign, dist, counts, o = kmeans_step(xd, c, flags, 11, i)
            objs.append(o)
        assert torch.equal(c, a[0]) and torch.equal(torch.cat(objs), a[1])
        assert torch.equal(assign, a[2]) and torch.equal(dist, a[3]) and torch.equal(counts, a[4])


def test_kmeans_surface():
    rng = np.random.default_rng(9)
    centre = 3.0 * rng.standard_normal((8, 32))
    x = (centre[rng.integers(0, 8, 1500)] + rng.standard_normal((1500, 32))).astype(np.float32)
    km = Kmeans(32, 8, niter=10, seed=3)
    final = km.train(x)
    assert isinstance(km.centroids, np.ndarray) and km.centroids.shape == (8, 32) and km.centroids.dtype == np.float32
    assert isinstance(km.obj, np.ndarray) and km.obj.shape == (10,) and final == float(km.obj[-1])
    assert np.all(np.diff(km.obj) <= 1e-4 * km.obj[:-1])                  # Lloyd never raises the objective
    D, I = km.assign(x)
    Ds, Is = km.index.search(x, 1)
    assert D.shape == (1500,) and I.dtype == np.int64 and np.array_equal(D, Ds[:, 0]) and np.array_equal(I, Is[:, 0])
    xt = dev(x)
    kt = Kmeans(32, 8, niter=10, seed=3)
    assert kt.train(xt) == final and kt.centroids.is_cuda and np.array_equal(kt.centroids.cpu().numpy(), km.centroids)
    Dt, It = kt.assign(xt)
    assert Dt.is_cuda and np.array_equal(It.cpu().numpy(), I)
    # nredo: the best of the runs a single-run object makes from the same initial points and seeds
    singles = []
    for r in range(3):
        init = x[cl._permutation(1500, 3 + 1 + r * 15486557)[:8].numpy()]
        singles.append(Kmeans(32, 8, niter=10, seed=3 + r).train(x, init_centroids=init))
    assert singles[0] == final
    assert Kmeans(32, 8, niter=10, seed=3, nredo=3).train(x) == min(singles)
    # n == k copies the points; spherical centroids have unit rows
    kk = Kmeans(32, 8)
    assert kk.train(x[:8]) == 0.0 and np.array_equal(kk.centroids, x[:8])
    ks = Kmeans(32, 8, niter=3, spherical=True)
    ks.train(x)
    assert np.all(np.abs(np.linalg.norm(ks.centroids.astype(np.float64), axis=1) - 1) <= 4 * U)


def test_kmeans_subsample_and_warning():
    x, _, _ = trajectory(1000, 16, 3, 0.3)
    km = Kmeans(16, 3, niter=5, max_points_per_centroid=100, seed=21)
    km.train(x)
    sub = x[cl._permutation(1000, 21)[:300].numpy()]
    direct = Kmeans(16, 3, niter=5, seed=21)
    direct.train(sub)
    assert np.array_equal(km.centroids, direct.centroids) and np.array_equal(km.obj, direct.obj)
    with pytest.warns(UserWarning, match="at least"):
        Kmeans(16, 3, niter=1).train(x[:50])


class _Frames(torch.utils.data.Dataset):
    def __init__(self, frames):
        self.frames = frames

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return {"image": torch.from_numpy(self.frames[i])}


@pytest.mark.filterwarnings("ignore:clustering 2000 points")
def test_end_to_end_netvlad_initialisation():
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import _NetVLAD
    from nano_vs_slam_amd.synthetic import synthetic_frames
    model, _ = product_model("S", False, 28)
    ds = _Frames(synthetic_frames(8, 64, 96, seed=12))
    x = torch.from_numpy(ds.frames[:2]).cuda()
    with torch.no_grad():
        before = model(x)["vlad"].clone()
    sampling = dict(nDescriptors=2000, nPerImage=250)
    np.random.seed(1)
    torch.manual_seed(1)
    cl.init_netvlad(model, ds, num_clusters=64, device="cuda:0", **sampling)
    np.random.seed(1)
    torch.manual_seed(1)
    clsts, descs = cl.get_clusters(model, ds, None, device="cuda:0", num_clusters=64, **sampling)
    assert clsts.is_cuda and descs.is_cuda and clsts.shape == (64, model.encoder_dim) and descs.shape == (2000, model.encoder_dim)
    nv = model.vlad_head.netvlad
    assert torch.equal(nv.centroids.data, clsts)            # the same draws, the same bits
    with torch.no_grad():
        after = model(x)["vlad"]
    assert bool(torch.isfinite(after).all()) and not torch.equal(after, before)       # the engine took the new tensors
    rows = after.reshape(2, -1).double().norm(dim=1).cpu().numpy()
    assert np.all(np.abs(rows - 1) < 1e-5)
    # the numpy init_params on the device's own centroids and samples
    c, d = clsts.cpu().numpy(), descs.cpu().numpy()
    ref = _NetVLAD(64, model.encoder_dim)
    ref.init_params(c.copy(), d.copy())
    unit = c.astype(np.float64) / np.linalg.norm(c.astype(np.float64), axis=1, keepdims=True)
    D = np.sort(vr.distances64(unit, d), axis=1)[:, :2]
    rel = ((kr.ALPHA + 2) * U * (D[:, 0] + D[:, 1])).mean() / (D[:, 1] - D[:, 0]).mean()
    print(f"alpha {nv.alpha} (device) {ref.alpha} (numpy), relative bound {rel:.3e}")
    assert abs(nv.alpha - ref.alpha) <= rel * abs(ref.alpha)
    assert np.array_equal(nv.centroids.detach().cpu().numpy(), ref.centroids.detach().numpy())
    w, w_ref = nv.conv.weight.detach().cpu().numpy().astype(np.float64), ref.conv.weight.detach().numpy().astype(np.float64)
    assert w.shape == w_ref.shape == (64, model.encoder_dim, 1, 1) and nv.conv.bias is None
    assert np.all(np.abs(w - w_ref) <= rel * np.abs(w_ref))
