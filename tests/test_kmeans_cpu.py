"""Host-side checks of the device k-means' reference and bounds (tests/kmeans_ref.py), of Kmeans' argument checks and
of get_clusters' sampling.  No GPU involved."""
from math import ceil

import numpy as np
import pytest
import torch

import kmeans_ref as kr
from nano_vs_slam_amd.clustering import Kmeans, sample_descriptors


def clustered(rng, m, d):
    """One cluster's rows as k-means sees them: a unit centre plus noise (a non-zero mean is the hard case for a sum)."""
    c = rng.standard_normal(d)
    c /= np.linalg.norm(c)
    return (c[None, :] + 0.3 * rng.standard_normal((m, d)) / np.sqrt(d)).astype(np.float32)


def ratio(got, rows):
    """max over components of |got - float64 mean| / bound."""
    rows64 = rows.astype(np.float64)
    c64 = rows64.mean(0)
    bound = kr.ALPHA * kr.U * np.abs(rows64).mean(0) + 2 * kr.U * np.abs(c64)
    return float((np.abs(got.astype(np.float64) - c64) / bound).max())


@pytest.mark.parametrize("d", [16, 64, 256])
@pytest.mark.parametrize("m", [1, 63, 512, 513, 4099])
def test_sum_order_is_pinned_from_both_sides(m, d):
    rng = np.random.default_rng(1000 * d + m)
    for rows in (clustered(rng, m, d), rng.standard_normal((m, d)).astype(np.float32)):
        r = ratio(kr.emulate_mean(rows), rows)
        print(f"m={m} d={d}: faithful order uses {r:.3f} of the bound")
        assert r <= 0.25
    rows = clustered(rng, m, d)
    victim = int(rng.integers(0, m))
    assert ratio(kr.emulate_mean(rows, drop_row=victim), rows) > 4
    assert ratio(kr.emulate_mean(rows, twice_row=victim), rows) > 4
    assert ratio(kr.emulate_mean(rows, count_off=1), rows) > 4
    if m > 1:
        assert ratio(kr.emulate_mean(rows, count_off=-1), rows) > 4


@pytest.mark.parametrize("n,d,k,sigma", [(1000, 16, 3, 0.3), (2053, 128, 65, 0.3), (4099, 64, 64, 0.6)])
def test_lloyd64_agrees_with_sklearn(n, d, k, sigma):
    from sklearn.cluster import KMeans
    x, label = kr.blobs(n, d, k, sigma)
    x64 = x.astype(np.float64)
    traj = kr.lloyd64(x, x[:k], 10)
    sk = KMeans(n_clusters=k, init=x64[:k].copy(), n_init=1, algorithm="lloyd", tol=0, max_iter=10).fit(x64)
    assert np.abs(sk.cluster_centers_ - traj[-1][1]).max() <= 1e-9
    assert np.array_equal(sk.labels_, traj[-1][0])
    assert abs(sk.inertia_ - kr.assign64(x, traj[-1][1])[1].sum()) <= 1e-9 * sk.inertia_
    # what the issue states about the recipe, and the GPU trajectory test relies on
    assert all(np.array_equal(a, label) for a, *_ in traj)
    assert min(t[3] for t in traj) > 0.3
    assert all(abs(t[2] - traj[1][2]) <= 1e-12 * traj[1][2] for t in traj[1:])


def test_split_restatement_on_a_hand_made_case():
    c = np.arange(1, 4 * 6 + 1, dtype=np.float32).reshape(4, 6)
    counts = np.array([3, 0, 1, 0])
    out, run, pairs = kr.split_ref(c, counts, seed=1, iteration=0)
    # only cluster 0 has two points or more: it is the donor of both, and its centroid is perturbed twice
    assert pairs == [(1, 0), (3, 0)]
    up, dn = np.float32(1 + 1 / 1024), np.float32(1 - 1 / 1024)
    f = np.where(np.arange(6) % 2 == 0, up, dn).astype(np.float32)
    g = np.where(np.arange(6) % 2 == 0, dn, up).astype(np.float32)
    assert np.array_equal(out[1], c[0] * f)
    assert np.array_equal(out[3], (c[0] * g) * f)
    assert np.array_equal(out[0], (c[0] * g) * g)
    assert np.array_equal(out[2], c[2])
    assert run.tolist() == [1, 1, 1, 1] and run.sum() == counts.sum()
    # the donor follows the draw: weights (count - 1) = [3, 0, 6]; r = draw % 9 picks cluster 0 below 3, cluster 2 from 3 on
    c3 = np.ones((4, 2), np.float32)
    for seed in range(20):
        _, _, pairs = kr.split_ref(c3, np.array([4, 1, 7, 0]), seed=seed, iteration=2)
        r = kr.draw(seed, 2, 3) % 9
        assert pairs == [(3, 0 if r < 3 else 2)]
    picks = [kr.split_ref(c3, np.array([4, 1, 7, 0]), seed=s, iteration=0)[2][0][1] for s in range(300)]
    assert 60 < picks.count(0) < 140 and picks.count(1) == 0           # about a third of the draws
    assert kr.draw(1, 2, 3) != kr.draw(1, 3, 2) and kr.draw(1, 2, 3) == kr.draw(1, 2, 3)
    # nobody can give: the centroids stay
    out, run, pairs = kr.split_ref(c3, np.array([1, 1, 1, 0]), seed=0, iteration=0)
    assert pairs == [] and np.array_equal(out, c3)


def test_kmeans_argument_checks_need_no_device():
    with pytest.raises(ValueError, match="dim"):
        Kmeans(20, 4)
    with pytest.raises(ValueError, match="precision"):
        Kmeans(64, 4, precision="bf16")
    with pytest.raises(ValueError, match="k ="):
        Kmeans(64, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Kmeans(64, 4, device="cpu")
    km = Kmeans(64, 4)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        km.train(torch.zeros(100, 64))
    with pytest.raises(ValueError, match="at least as large"):
        km.train(np.zeros((3, 64), np.float32))
    with pytest.raises(ValueError, match=r"\[n, 64\]"):
        km.train(np.zeros((100, 32), np.float32))
    with pytest.raises(TypeError):
        km.train([[0.0] * 64] * 8)
    with pytest.raises(RuntimeError, match="train"):
        km.assign(np.zeros((3, 64), np.float32))


class _Frames(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return {"image": torch.full((3, 8, 8), float(i))}


class _Encoder:
    """Stands in for the model: channel 0 of a descriptor names its image, channel 1 its location."""
    encoder_dim = 16

    def eval(self):
        return self

    def to(self, device):
        return self

    def only_encoder(self, x):
        out = torch.zeros(x.shape[0], self.encoder_dim, 4, 6)
        out[:, 0] = x[:, 0, 0, 0][:, None, None]
        out[:, 1] = torch.arange(24.0).reshape(4, 6)
        return out


def test_get_clusters_draws_what_the_reference_draws():
    from torch.utils.data import DataLoader, SubsetRandomSampler
    ds, n_per, n_desc, batch = _Frames(40), 5, 52, 4
    np.random.seed(3)
    torch.manual_seed(5)
    got = sample_descriptors(_Encoder(), ds, nPerImage=n_per, cacheBatchSize=batch, device="cpu", nDescriptors=n_desc)
    assert got.shape == (n_desc, 16)
    # the reference's lines (utils/netvlad_utils.py:27-72) under the same seeds
    np.random.seed(3)
    torch.manual_seed(5)
    n_im = ceil(n_desc / n_per)
    sampler = SubsetRandomSampler(np.random.choice(len(ds), n_im, replace=False))
    loader = DataLoader(dataset=ds, num_workers=0, batch_size=batch, shuffle=False, pin_memory=False, sampler=sampler)
    want = np.zeros((n_im * n_per, 2))
    for iteration, sample in enumerate(loader, 1):
        images = sample["image"][:, 0, 0, 0].numpy()
        for ix in range(len(images)):
            loc = np.random.choice(24, n_per, replace=False)
            startix = (iteration - 1) * batch * n_per + ix * n_per
            want[startix:startix + n_per, 0] = images[ix]
            want[startix:startix + n_per, 1] = loc
    assert np.array_equal(got[:, :2].numpy(), want[:n_desc])      # rows past nDescriptors are dropped
    assert len(set(want[:, 0].tolist())) == n_im
