"""Float64 reference of the device k-means (nano_vs_slam_amd.clustering.Kmeans, csrc/kmeans.hip) and the bounds its
tests use.  faiss is not installed here: the oracle is float64 Lloyd, cross-checked against sklearn in
tests/test_kmeans_cpu.py.

Bounds (u = 2^-24, ALPHA = 32: the project's accumulation constant, tests/vpr_ref.py and tests/layer_ref.py)
------------------------------------------------------------------------------------------------------------
* Assignment and dist: the search's own contract with k = 1 (vpr_ref.eps_set / check_contract, imported by the tests).
* Centroid, GIVEN an assignment (the tests pass the device's own, which isolates the sum kernels): per component
  |c - c64| <= ALPHA u mean_i |x_i| + 2 u |c64|, the mean over the cluster's rows of that component's magnitude; the
  second term is the rounding of 1 / count and of the product.  A worst-case bound would grow with the list length and
  hide a lost row in a list of thousands; this one does not.  ``emulate_mean`` restates the kernel's summation order in
  fp32 (chunks of 512 rows, row groups by dim, 8 accumulators per lane, the two trees, chunk partials in order);
  tests/test_kmeans_cpu.py shows it stays 4x inside the bound at list lengths 1, 63, 512, 513 and 4099 and that a
  dropped row, a row added twice and a count off by one each exceed it 4x.
* Objective: |obj - obj64| <= sum_i eps_dist(d64_i) + ALPHA u obj64 (every dist within its own bound, then the sum).
* Split: ``split_ref`` restates the rule and the counter-based draw (``draw``) of csrc/kmeans.hip.
"""
from __future__ import annotations

import numpy as np

from vpr_ref import ALPHA, U, distances64, eps_dist

CHUNK, UNR = 512, 8
SPLIT_EPS = 1.0 / 1024.0
M64 = (1 << 64) - 1


def assign64(x, c):
    """-> (assign [n], d64 [n], margin [n]: second nearest minus nearest); ties go to the lower index (argmin's rule)."""
    x = np.asarray(x, np.float64)
    c = np.asarray(c, np.float64)
    d = distances64(c, x)
    a = d.argmin(1)
    dmin = d[np.arange(len(x)), a]
    if c.shape[0] > 1:
        d2 = d.copy()
        d2[np.arange(len(x)), a] = np.inf
        margin = d2.min(1) - dmin
    else:
        margin = np.full(len(x), np.inf)
    return a, dmin, margin


def means64(x, assign, k, c_in):
    """Float64 mean of every cluster's rows under ``assign``; an empty cluster keeps its input centroid."""
    x = np.asarray(x, np.float64)
    c = np.asarray(c_in, np.float64).copy()
    counts = np.bincount(assign, minlength=k)
    sums = np.zeros((k, x.shape[1]))
    np.add.at(sums, assign, x)
    nz = counts > 0
    c[nz] = sums[nz] / counts[nz, None]
    return c, counts


def lloyd64(x, c0, niter):
    """Float64 Lloyd trajectory -> list of (assign, centroids after the update, objective, smallest margin, d64 [n])."""
    c = np.asarray(c0, np.float64)
    out = []
    for _ in range(niter):
        a, d, margin = assign64(x, c)
        c, _ = means64(x, a, c.shape[0], c)
        out.append((a, c, d.sum(), margin.min(), d))
    return out


def centroid_bound(x, assign, k, c64):
    """Per component: ALPHA u mean_i |x_i| + 2 u |c64| (0 + 0 for an empty cluster: it must come back unchanged)."""
    ax, counts = means64(np.abs(np.asarray(x, np.float64)), assign, k, np.zeros_like(c64))
    b = ALPHA * U * ax + 2 * U * np.abs(c64)
    b[counts == 0] = 0.0
    return b


def obj_bound(d64):
    d64 = np.asarray(d64, np.float64)
    return eps_dist(d64).sum() + ALPHA * U * d64.sum()


def blobs(n, d, k, sigma, seed=7):
    """The trajectory recipe: k unit-norm Gaussian centres, label = arange(n) % k, x = centre[label] + sigma N(0,1)/sqrt(d),
    rows normalised, fp32 -> (x, label); init_centroids = x[:k] holds one point of every blob."""
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal((k, d))
    centre /= np.linalg.norm(centre, axis=1, keepdims=True)
    label = np.arange(n) % k
    x = centre[label] + sigma * rng.standard_normal((n, d)) / np.sqrt(d)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), label


def groups_of(d):
    """Row groups of a wave in km_sum_kernel: 64 / (the power of two >= min(d / 4, 64), at least 4)."""
    cw = 4
    while cw < d // 4 and cw < 64:
        cw *= 2
    return 64 // cw


def emulate_mean(rows, drop_row=None, twice_row=None, count_off=0):
    """fp32 emulation of km_sum_kernel + km_update_kernel for one list ``rows`` [m, d] (the list's order).  Faults:
    ``drop_row`` / ``twice_row`` (an index of the list) and ``count_off`` (added to the divisor)."""
    rows = np.asarray(rows, np.float32)
    m, d = rows.shape
    G = groups_of(d)
    weight = np.ones(m, np.float32)
    if drop_row is not None:
        weight[drop_row] = 0
    if twice_row is not None:
        weight[twice_row] = 2
    total = None
    for r0 in range(0, m, CHUNK):
        ch = rows[r0:r0 + CHUNK]
        wt = weight[r0:r0 + CHUNK]
        s = []
        for g in range(G):
            sub, sw = ch[g::G], wt[g::G]
            acc = np.zeros((UNR, d), np.float32)
            for j in range(len(sub)):
                for _ in range(int(sw[j])):
                    acc[j % UNR] = acc[j % UNR] + sub[j]
            s.append(((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7])))
        o = 1
        while o < G:
            s = [s[g] + s[g ^ o] for g in range(G)]
            o *= 2
        total = s[0] if total is None else total + s[0]
    inv = np.float32(1.0) / np.float32(m + count_off)
    return (total * inv).astype(np.float32)


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, iteration, ci):
    """The counter-based draw of the split: a 64-bit hash of (seed, iteration, ci)."""
    return _mix(_mix((seed + 0x9E3779B97F4A7C15) & M64) ^ (((iteration & 0xFFFFFFFF) << 32) | (ci & 0xFFFFFFFF)))


def split_ref(c, counts, seed, iteration):
    """faiss's split_clusters restated with the draw above, on float32 centroids -> (centroids, running counts,
    [(ci, cj), ...]).  Empty clusters in ascending order; donor cj with probability proportional to max(count - 1, 0)
    over the running counts; c[ci] = c[cj]; even components of c[ci] times 1 + 1/1024 and of c[cj] times 1 - 1/1024, odd
    ones swapped; the donor's running count halved between the two."""
    c = np.asarray(c, np.float32).copy()
    run = np.asarray(counts, np.int64).copy()
    pairs = []
    even = np.arange(c.shape[1]) % 2 == 0
    up, dn = np.float32(1 + SPLIT_EPS), np.float32(1 - SPLIT_EPS)
    for ci in np.nonzero(run == 0)[0]:
        w = np.maximum(run - 1, 0)
        total = int(w.sum())
        if total <= 0:
            break
        r = draw(seed, iteration, int(ci)) % total
        cj = int(np.searchsorted(np.cumsum(w), r, side="right"))
        v = c[cj].copy()
        c[ci] = np.where(even, v * up, v * dn)
        c[cj] = np.where(even, v * dn, v * up)
        run[ci] = run[cj] // 2
        run[cj] -= run[ci]
        pairs.append((int(ci), cj))
    return c, run, pairs
