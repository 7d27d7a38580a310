"""Float64 reference of the flat squared-L2 top-k (nano_vs_slam_amd.vpr.FlatL2Index) and the error bound its tests use.

Error bound
-----------
u = 2^-24.  For a query q and a database row d (both the fp32 values the device was given), M = sum_i |q_i d_i|.

* Ranking key.  The kernel ranks rows by key = |d|^2 - 2 q.d, and d64 = |q|^2 + key64, so a key error moves a row's
  rank exactly as a distance error would.  fp32 accumulation of q.d (split: exact fp16 x fp16 products summed in fp32;
  fp32 mode: a k-ordered fma chain) and of |d|^2 is bounded as tests/layer_ref.py does, by ALPHA u M and ALPHA u |d|^2
  with ALPHA = 32 (a worst-case K u bound would be too loose to see a lost split term at K = 4096).  The split adds the
  representation error of q = 2^-s (qh + ql + dq): |dq_i| <= max(2^-22 |q_i|, 2^-25 2^-s) with 2^-s <= 2^-14 max|q|,
  against q.d the kernel misses dq.d + q.dd + ql.dl: 3 * 2^-22 M + 2^-39 (max|q| sum|d| + max|d| sum|q|).  The key
  doubles the q.d term:  eps_key = 2 (ALPHA u M [+ split]) + ALPHA u |d|^2.
* Returned distance: the direct fp32 re-score sum (q - d)^2: eps_dist = (ALPHA + 2) u d64 (the subtraction and the
  square round once each).
* Set contract, with t the float64 k-th distance and eps = max over rows of eps_key: every returned row has
  d64 <= t + 2 eps and every row with d64 < t - 2 eps is returned.
tests/test_vpr_cpu.py pins the bound from both sides: a faithful numpy emulation of the split stays well inside it,
and a dropped cross term, flushed lo halves or a missing rescale each exceed it many times over.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
ALPHA = 32.0


def distances64(db, q):
    db = np.asarray(db, np.float64)
    q = np.asarray(q, np.float64)
    d = (q * q).sum(1)[:, None] + (db * db).sum(1)[None, :] - 2.0 * q @ db.T
    # the expansion cancels for near-duplicates: exact differences where it matters
    close = d < 1e-3 * ((q * q).sum(1)[:, None] + (db * db).sum(1)[None, :])
    for i, j in zip(*np.nonzero(close)):
        d[i, j] = ((q[i] - db[j]) ** 2).sum()
    return np.maximum(d, 0.0)


def topk64(d64, k, limit=None):
    """float64 top-k: ascending distance, ties by lower row; padding (inf, -1) past the rows available."""
    nq, n = d64.shape
    D = np.full((nq, k), np.inf)
    I = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        m = n if limit is None else int(min(max(limit[i], 0), n))
        o = np.lexsort((np.arange(m), d64[i, :m]))[:k]
        D[i, :len(o)] = d64[i, o]
        I[i, :len(o)] = o
    return D, I


def eps_key(db, q, split):
    db = np.asarray(db, np.float64)
    q = np.asarray(q, np.float64)
    M = np.abs(q) @ np.abs(db).T
    dot = ALPHA * U * M
    if split:
        dot = dot + 3 * 2.0 ** -22 * M + 2.0 ** -39 * (np.abs(q).max(1)[:, None] * np.abs(db).sum(1)[None, :]
                                                       + np.abs(db).max(1)[None, :] * np.abs(q).sum(1)[:, None])
    return 2 * dot + ALPHA * U * (db * db).sum(1)[None, :]


def eps_dist(d64):
    return (ALPHA + 2) * U * d64


def split_rows(x):
    """The kernel's pack: per-row power of two s with max|x| 2^s in [2^14, 2^15), hi = rn16(x 2^s), lo = rn16(x 2^s - hi)
    -> (hi, lo as float32 arrays, 2^-s per row)."""
    x = np.asarray(x, np.float32)
    mx = np.abs(x).max(1)
    e = np.where(mx > 0, np.floor(np.log2(np.where(mx > 0, mx, 1))), 0).astype(np.int64)
    sh = np.clip(14 - e, -125, 125)
    v = (x * np.ldexp(np.float32(1), sh)[:, None].astype(np.float32)).astype(np.float32)
    hi = v.astype(np.float16).astype(np.float32)
    lo = (v - hi).astype(np.float16).astype(np.float32)
    return hi, lo, np.ldexp(1.0, -sh).astype(np.float32)


def emulate_keys(db, q, drop_cross=False, flush_lo=False, skip_rescale=False):
    """numpy emulation of the split-fp16 key |d|^2 - 2 q.d: exact products of fp16 halves summed in fp32 16 at a time
    (one MFMA k-step), the three terms in the kernel's order, then the two exact rescales.  The flags model faults."""
    qh, ql, uq = split_rows(q)
    dh, dl, ud = split_rows(db)
    if flush_lo:                                         # lo planes lost (flushed to zero)
        ql = np.zeros_like(ql)
        dl = np.zeros_like(dl)
    nq, dim = q.shape
    acc = np.zeros((nq, db.shape[0]), np.float32)
    terms = [(ql, dh), (qh, dl), (qh, dh)]
    if drop_cross:
        terms = [(qh, dl), (qh, dh)]
    for s in range(0, dim, 16):
        for a, b in terms:
            acc = (acc + (a[:, s:s + 16] @ b[:, s:s + 16].T).astype(np.float32)).astype(np.float32)
    dot = acc if skip_rescale else (acc * ud[None, :]).astype(np.float32) * uq[:, None]
    n2 = (np.asarray(db, np.float32) ** 2).sum(1, dtype=np.float32)
    return (n2[None, :].astype(np.float64) - 2.0 * dot.astype(np.float64)).astype(np.float32)


def check_contract(D, I, d64, k, eps, label, limit=None):
    """Set contract of kp2d_vpr_search against float64 -> number of rows that needed the 2 eps band (the exemption)."""
    D = np.asarray(D)
    I = np.asarray(I)
    nq, n = d64.shape
    D64, I64 = topk64(d64, k, limit)
    used = 0
    for i in range(nq):
        m = n if limit is None else int(min(max(limit[i], 0), n))
        kk = min(k, m)
        got = I[i, :kk]
        assert np.all(I[i, kk:] == -1) and np.all(D[i, kk:] == np.float32(np.finfo(np.float32).max)), (label, i, "padding")
        assert np.all(got >= 0) and np.all(got < m), (label, i, "row out of range")
        assert len(set(got.tolist())) == kk, (label, i, "duplicate rows")
        if kk == 0:
            continue
        t = D64[i, kk - 1]
        e = float(eps[i])
        dg = d64[i, got]
        assert np.all(dg <= t + 2 * e), (label, i, "returned row too far", float(dg.max() - t), e)
        must = set(np.nonzero(d64[i, :m] < t - 2 * e)[0].tolist())
        assert must <= set(got.tolist()), (label, i, "missed a row clearly inside the k nearest")
        used += len(set(got.tolist()) ^ set(I64[i, :kk].tolist())) // 2
        assert np.all(np.abs(D[i, :kk].astype(np.float64) - dg) <= eps_dist(dg) + 1e-45), (label, i, "distance")
        assert np.all(np.diff(D[i, :kk]) >= 0), (label, i, "not ascending")
        tie = np.diff(D[i, :kk]) == 0
        assert np.all(np.diff(got)[tie] > 0), (label, i, "equal distances not by ascending row")
    return used


def eps_set(db, q, d64, k, split, limit=None):
    """eps of the set contract per query: the largest eps_key among the rows that could compete for the k nearest (d64
    within 4x the k-th distance; a row beyond that is farther out than its own key error by orders of magnitude)."""
    e = eps_key(db, q, split)
    D64, _ = topk64(d64, k, limit)
    t = np.where(np.isfinite(D64), D64, 0).max(1)
    near = d64 <= 4 * t[:, None] + 1e-30
    return np.where(near, e, 0).max(1)
