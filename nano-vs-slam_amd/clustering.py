"""k-means on the device and the NetVLAD cluster initialisation built on it.

* ``Kmeans`` — faiss.Kmeans' surface (``train``, ``assign``, ``centroids``, ``obj``, ``index``) on the HIP kernels of
  csrc/kmeans.hip (kp2d_kmeans_train, include/kp2d.h): Lloyd iterations whose assignment is the flat index's own search,
  bit-reproducible per-cluster sums, faiss's empty-cluster split.  faiss's algorithm, not faiss's random stream.
* ``get_clusters`` / ``init_netvlad`` — the reference's fit of NetVLAD's centroids (utils/netvlad_utils.py:15-120) with
  the descriptors resident in HBM from the encoder to ``model.init_netvlad``.

There is no CPU path: CPU tensors raise, like the rest of the product.
"""
from __future__ import annotations

import warnings
from math import ceil

import numpy as np
import torch

from . import _dev, _lib
from ._dev import ptr as _ptr, stream as _stream
from .vpr import PRECISIONS, FlatL2Index, check_dim

KMEANS_SPHERICAL = 2
KMEANS_NO_SPLIT = 4
MAX_K = 65536


def _permutation(n: int, seed: int) -> torch.Tensor:
    """Seeded permutation of range(n): host-side plumbing, an index tensor for a device gather."""
    return torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))


def _outputs(x, centroids, nobj):
    if not (x.is_cuda and centroids.is_cuda and x.dtype == centroids.dtype == torch.float32 and x.dim() == centroids.dim() == 2
            and x.shape[1] == centroids.shape[1] and x.is_contiguous() and centroids.is_contiguous()):
        raise ValueError("x [n, d] and centroids [k, d] must be contiguous float32 device tensors")
    n, k, dev = x.shape[0], centroids.shape[0], x.device
    lib = _lib.load()
    nbytes = int(lib.kp2d_kmeans_scratch_bytes(n, x.shape[1], k))
    return (lib, torch.empty(nobj, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
            torch.empty(n, dtype=torch.float32, device=dev), torch.empty(k, dtype=torch.int64, device=dev),
            _dev.scratch(nbytes, dev), _stream(dev))


def kmeans_step(x, centroids, flags=0, seed=1234, iteration=0):
    """kp2d_kmeans_step on device tensors -> (new centroids, assign [n], dist [n], counts [k], obj [1]); nothing is
    synchronised.  ``flags``: PRECISIONS[...] | KMEANS_SPHERICAL | KMEANS_NO_SPLIT."""
    lib, obj, assign, dist, counts, scratch, stream = _outputs(x, centroids, 1)
    out = torch.empty_like(centroids)
    _lib.check(lib.kp2d_kmeans_step(_ptr(x), x.shape[0], x.shape[1], _ptr(centroids), centroids.shape[0], flags, seed, iteration,
                                    _ptr(out), _ptr(assign), _ptr(dist), _ptr(counts), _ptr(obj), _ptr(scratch),
                                    scratch.numel(), stream))
    return out, assign, dist, counts, obj


def kmeans_train(x, init_centroids, niter, flags=0, seed=1234):
    """kp2d_kmeans_train on device tensors -> (final centroids, obj [niter], assign, dist, counts of the last iteration)."""
    lib, obj, assign, dist, counts, scratch, stream = _outputs(x, init_centroids, niter)
    cent = init_centroids.clone()
    _lib.check(lib.kp2d_kmeans_train(_ptr(x), x.shape[0], x.shape[1], _ptr(cent), cent.shape[0], niter, flags, seed, _ptr(obj),
                                     _ptr(assign), _ptr(dist), _ptr(counts), _ptr(scratch), scratch.numel(), stream))
    return cent, obj, assign, dist, counts


class Kmeans:
    """faiss.Kmeans on the MI355X.  ``train(x)`` fits ``k`` centroids to x [n, d] in ``niter`` Lloyd iterations and
    returns the final objective; afterwards ``centroids`` [k, d], ``obj`` [niter] (sum of squared distances at the start
    of every iteration) and ``index`` (a FlatL2Index over the centroids) are set.  numpy in -> numpy out, device tensors
    in -> device tensors out.  faiss semantics kept: n < k raises, n == k copies the points, more than
    ``k * max_points_per_centroid`` points are subsampled (seeded), fewer than ``k * min_points_per_centroid`` warn, the
    initial centroids are k distinct points of a seeded permutation, ``nredo`` > 1 keeps the run with the lowest final
    objective, ``spherical`` normalises the centroids after every update."""

    def __init__(self, d: int, k: int, niter: int = 25, nredo: int = 1, verbose: bool = False, spherical: bool = False,
                 seed: int = 1234, max_points_per_centroid: int = 256, min_points_per_centroid: int = 39, device="cuda:0",
                 precision: str = "f16x3"):
        self.d = check_dim(d)
        self.k = int(k)
        if self.k < 1 or self.k > MAX_K:
            raise ValueError(f"k = {k} outside [1, {MAX_K}]")
        if int(niter) < 1 or int(nredo) < 1:
            raise ValueError("niter and nredo must be at least 1")
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Kmeans runs on the HIP device only (no CPU fallback)")
        self.niter, self.nredo, self.verbose, self.spherical, self.seed = int(niter), int(nredo), verbose, spherical, int(seed)
        self.max_points_per_centroid, self.min_points_per_centroid = int(max_points_per_centroid), int(min_points_per_centroid)
        self.precision = precision
        self.centroids = self.obj = self.index = None

    @property
    def flags(self) -> int:
        return PRECISIONS[self.precision] | (KMEANS_SPHERICAL if self.spherical else 0)

    def _check(self, x, what):
        """-> input was numpy; shape and placement checked before anything touches the device."""
        if isinstance(x, np.ndarray):
            is_np = True
        elif isinstance(x, torch.Tensor):
            _dev.require_device(what, x, "pass numpy or a device tensor")
            is_np = False
        else:
            raise TypeError(f"{what} must be a numpy array or a torch tensor")
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"{what} must be [n, {self.d}], got {tuple(x.shape)}")
        return is_np

    def _device(self, x):
        if isinstance(x, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
        return x.detach().to(self.device, torch.float32).contiguous()

    def train(self, x, init_centroids=None) -> float:
        is_np = self._check(x, "train")
        n = x.shape[0]
        if n < self.k:
            raise ValueError(f"number of training points ({n}) should be at least as large as the number of clusters ({self.k})")
        if init_centroids is not None:
            self._check(init_centroids, "init_centroids")
            if init_centroids.shape[0] != self.k:
                raise ValueError(f"init_centroids must be [{self.k}, {self.d}]")
        x = self._device(x)
        if n == self.k:                                  # faiss: as many points as centroids, the points are the centroids
            best = (x.clone(), torch.zeros(0, dtype=torch.float32, device=self.device))
            final = 0.0
        else:
            if n > self.k * self.max_points_per_centroid:
                n = self.k * self.max_points_per_centroid
                if self.verbose:
                    print(f"Sampling a subset of {n} / {x.shape[0]} for training")
                x = x[_permutation(x.shape[0], self.seed)[:n].to(self.device)]
            elif n < self.k * self.min_points_per_centroid:
                warnings.warn(f"clustering {n} points to {self.k} centroids: please provide at least "
                              f"{self.k * self.min_points_per_centroid} training points")
            best, final = None, None
            for redo in range(self.nredo):
                if init_centroids is not None:
                    init = self._device(init_centroids)
                else:
                    init = x[_permutation(n, self.seed + 1 + redo * 15486557)[:self.k].to(self.device)]
                cent, obj, *_ = kmeans_train(x, init, self.niter, self.flags, self.seed + redo)
                if self.nredo == 1:
                    best = (cent, obj)
                    break
                last = float(obj[-1])                    # comparing runs needs their objectives on the host
                if self.verbose:
                    print(f"Outer iteration {redo} / {self.nredo}: objective {last:g}")
                if final is None or last < final:
                    best, final = (cent, obj), last
            if final is None:
                final = float(best[1][-1])
        cent, obj = best
        if self.verbose:
            for i, v in enumerate(obj.tolist()):
                print(f"  Iteration {i}: objective {v:g}")
        self.index = FlatL2Index(self.d, device=self.device, precision=self.precision)
        self.index.add(cent)
        self.centroids = cent.cpu().numpy() if is_np else cent
        self.obj = obj.cpu().numpy() if is_np else obj
        return final

    def assign(self, x):
        """-> (D [n] squared L2 distance to the nearest centroid, I [n] its index)."""
        if self.index is None:
            raise RuntimeError("should train k-means first")
        D, I = self.index.search(x, 1)
        return D.reshape(-1), I.reshape(-1)


def sample_descriptors(model, cluster_set, nPerImage=100, cacheBatchSize=32, device="cuda", nDescriptors=50000):
    """Steps 1 of the reference's get_clusters (utils/netvlad_utils.py:27-81): ``ceil(nDescriptors / nPerImage)`` images
    drawn with ``np.random.choice`` (no replacement), visited in SubsetRandomSampler order in batches of ``cacheBatchSize``,
    ``nPerImage`` locations per image drawn with ``np.random.choice`` -> descriptors [nDescriptors, encoder_dim] on the
    device the encoder answers on."""
    from torch.utils.data import DataLoader, SubsetRandomSampler
    nIm = ceil(nDescriptors / nPerImage)
    sampler = SubsetRandomSampler(np.random.choice(len(cluster_set), nIm, replace=False))
    loader = DataLoader(dataset=cluster_set, num_workers=0, batch_size=cacheBatchSize, shuffle=False, pin_memory=False,
                        sampler=sampler)
    feats = None
    with torch.no_grad():
        model.eval()
        model = model.to(device)
        for iteration, sample in enumerate(loader, 1):
            x = sample["image"].to(device)
            desc = model.only_encoder(x).view(x.size(0), model.encoder_dim, -1).permute(0, 2, 1)
            if feats is None:
                feats = torch.empty(nIm * nPerImage, model.encoder_dim, dtype=torch.float32, device=desc.device)
            batchix = (iteration - 1) * cacheBatchSize * nPerImage
            for ix in range(desc.size(0)):
                loc = np.random.choice(desc.size(1), nPerImage, replace=False)      # different locations for each image
                startix = batchix + ix * nPerImage
                feats[startix:startix + nPerImage] = desc[ix, torch.from_numpy(loc).to(desc.device)]
    return feats[:nDescriptors]


def get_clusters(model, cluster_set, initcache=None, nPerImage=100, threads=8, cacheBatchSize=32, device="cuda",
                 num_clusters=64, nDescriptors=50000, cacheDir=None):
    """The reference's get_clusters (utils/netvlad_utils.py:15-92) with its signature and sequence: sample ``nPerImage``
    encoder descriptors from each of ``ceil(nDescriptors / nPerImage)`` random images, cluster them with 100 k-means
    iterations.  Three deviations: the result is returned as device tensors ``(centroids [num_clusters, encoder_dim],
    descriptors [nDescriptors, encoder_dim])`` instead of being written to an HDF5 cache; ``initcache`` / ``cacheDir``
    are accepted and unused; and when ``nPerImage`` does not divide ``nDescriptors`` the rows sampled past
    ``nDescriptors`` are dropped (the reference's fixed-size dataset fails on that slice)."""
    descriptors = sample_descriptors(model, cluster_set, nPerImage, cacheBatchSize, device, nDescriptors)
    kmeans = Kmeans(model.encoder_dim, num_clusters, niter=100, verbose=False, device=descriptors.device)
    kmeans.train(descriptors)
    return kmeans.centroids, descriptors


def init_netvlad(model, cluster_set, num_clusters=64, device="cuda", cacheDir=None, **sampling):
    """The reference's init_netvlad (utils/netvlad_utils.py:95-120): get_clusters, then model.init_netvlad on the centroids
    and the sampled descriptors — all of it on the device, no cache file.  ``sampling``: get_clusters' ``nPerImage``,
    ``cacheBatchSize`` and ``nDescriptors`` for image sets smaller than the reference's defaults need."""
    clsts, traindescs = get_clusters(model, cluster_set, None, device=device, num_clusters=num_clusters, cacheDir=cacheDir,
                                     **sampling)
    model.init_netvlad(clsts, traindescs)
