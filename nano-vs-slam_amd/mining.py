"""Triplet mining on the device — the step between "descriptors cached" and "next training batch".

* ``radius_neighbors`` / ``get_positives`` — the ground truth the reference takes from
  ``sklearn.neighbors.NearestNeighbors.radius_neighbors`` over UTM positions (src/data/pittsburgh.py:189-200, :258-289), as
  per-query row masks (``RowMask``) and, on request, index lists.  float64, sklearn's closed ball.
* ``FlatL2Index.search(..., mask=...)`` (vpr.py) — the flat index restricted to a query's rows.
* ``TripletMiner`` — the hard-triplet mining of ``QueryDatasetFromStruct.__getitem__`` (:295-333) for all queries in one
  call (kp2d_vpr_mine, include/kp2d.h): nearest non-trivial positive, sampled + cached negatives, the margin rule.  The
  draws follow the reference's algorithm (with replacement, then unique), not numpy's random stream.

Mask format (include/kp2d.h): 32-bit words, [nq, W] with W = ceil(ndb / 32); row r of query i is bit r & 31 of word
i W + (r >> 5).  The tensors are int32 (torch's plain 32-bit type); the bits are what counts.

There is no CPU path: CPU tensors raise, like the rest of the product.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _dev, _lib
from ._dev import ptr as _ptr, stream as _stream
from .vpr import PRECISIONS, FlatL2Index

GEO_INVERT = 1
MAX_CANDIDATES = 1024


def mask_words(ndb: int) -> int:
    return (int(ndb) + 31) // 32


def pack_mask(member) -> np.ndarray:
    """bool [nq, ndb] -> mask words [nq, W] uint32 (numpy; for masks that do not come from a radius)."""
    member = np.asarray(member, bool)
    nq, ndb = member.shape
    padded = np.zeros((nq, mask_words(ndb) * 32), np.uint8)
    padded[:, :ndb] = member
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").reshape(nq, mask_words(ndb))


def unpack_mask(words, ndb: int) -> np.ndarray:
    """mask words [nq, W] (uint32 / int32) -> bool [nq, ndb]; bits at or past ndb are dropped."""
    words = np.ascontiguousarray(words).view(np.uint32).astype("<u4")
    return np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")[:, :ndb].astype(bool)


def _positions(x, what, device):
    """numpy / device tensor [n, 2] -> (contiguous float64 device tensor, input was numpy)."""
    if isinstance(x, np.ndarray):
        t, is_np = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)), True
    elif isinstance(x, torch.Tensor):
        _dev.require_device(what, x, "pass numpy or a device tensor")
        t, is_np = x, False
    else:
        raise TypeError(f"{what} must be a numpy array or a torch tensor")
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError(f"{what} must be [n, 2] positions, got {tuple(t.shape)}")
    return t.to(device if is_np else t.device, torch.float64).contiguous(), is_np


class RowMask:
    """A per-query subset of database rows on the device: ``mask`` [nq, W] int32 words, ``count`` [nq] int32 set bits,
    ``ndb``.  ``lists()`` -> (lims [nq + 1] int64, idx [lims[-1]] int64): query i's rows, ascending, at
    idx[lims[i]:lims[i + 1]] (numpy when the mask was made from numpy positions)."""

    def __init__(self, mask, count, ndb, as_numpy=False):
        self.mask, self.count, self.ndb, self.as_numpy = mask, count, int(ndb), as_numpy
        self._lists = None

    @property
    def nq(self) -> int:
        return self.mask.shape[0]

    def lists(self):
        if self._lists is None:
            dev = self.mask.device
            lims = torch.zeros(self.nq + 1, dtype=torch.int64, device=dev)
            lims[1:] = torch.cumsum(self.count, 0)
            total = int(lims[-1]) if self.nq else 0
            idx = torch.empty(total, dtype=torch.int64, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            if self.nq:
                _lib.check(_lib.load().kp2d_mask_lists(_ptr(self.mask), self.nq, self.ndb, _ptr(lims), _ptr(idx) if total else None,
                                                       total, _ptr(status), _stream(dev)))
            self._lists = (lims.cpu().numpy(), idx.cpu().numpy()) if self.as_numpy else (lims, idx)
        return self._lists

    def index_arrays(self):
        """-> object array of nq int64 index arrays (what sklearn's radius_neighbors returns, each sorted)."""
        lims, idx = self.lists()
        if not self.as_numpy:
            lims, idx = lims.cpu().numpy(), idx.cpu().numpy()
        out = np.empty(self.nq, dtype=object)
        for i in range(self.nq):
            out[i] = idx[lims[i]:lims[i + 1]]
        return out


def radius_neighbors(db_xy, q_xy, radius, invert=False, device="cuda:0") -> RowMask:
    """The database rows within ``radius`` of every query position (closed ball, float64, no fused multiply-add: sklearn's
    ``radius_neighbors``) as a RowMask; ``invert``: the rows outside it.  numpy in -> numpy out of ``lists()``; device
    tensors in -> device tensors out."""
    db, np_db = _positions(db_xy, "db_xy", device)
    q, np_q = _positions(q_xy, "q_xy", db.device)
    if q.device != db.device:
        raise ValueError("db_xy and q_xy must live on one device")
    ndb, nq = db.shape[0], q.shape[0]
    mask = torch.zeros(nq, mask_words(ndb), dtype=torch.int32, device=db.device)
    count = torch.zeros(nq, dtype=torch.int32, device=db.device)
    if nq:
        _lib.check(_lib.load().kp2d_geo_radius_mask(_ptr(db) if ndb else None, ndb, _ptr(q), nq, float(radius),
                                                    GEO_INVERT if invert else 0, _ptr(mask) if ndb else None, _ptr(count),
                                                    _stream(db.device)))
    return RowMask(mask, count, ndb, as_numpy=np_db and np_q)


def get_positives(utmDb, utmQ, posDistThr, device="cuda:0"):
    """What ``WholeDatasetFromStruct.getPositives()`` returns (pittsburgh.py:189-200): an array of index arrays, the
    database rows within ``posDistThr`` of each query — directly the ``gt`` of ``vpr.recall_at_n`` and what
    ``evaluate_global_descriptor`` asks its ``eval_set`` for.  Each array is sorted (sklearn's are not; only membership
    is used)."""
    return radius_neighbors(np.asarray(utmDb, np.float64), np.asarray(utmQ, np.float64), posDistThr, device=device).index_arrays()


def mine_round(index: FlatL2Index, q, pos_mask, neg_mask, neg_cache=None, qid=None, n_sample=1000, n_neg=10, n_neg_factor=10,
               margin=0.1, seed=1234, round=0, want_cand=False, scratch=None):
    """kp2d_vpr_mine on device tensors -> (pos_idx [nq] int64, neg_idx [nq, n_neg] int32, neg_cnt [nq] int32, d_pos [nq]
    float32, cand_mask [nq, W] int32 or None); nothing is synchronised.  ``index``: a FlatL2Index holding the database."""
    q = _dev.require_device("mine", q).to(index.device, torch.float32).contiguous()
    nq, ndb, dev = q.shape[0], index.ntotal, index.device
    W = mask_words(ndb)
    for name, m in (("pos_mask", pos_mask), ("neg_mask", neg_mask)):
        _dev.require_device(name, m)
        if m.dtype not in (torch.int32, torch.uint32) or tuple(m.shape) != (nq, W) or not m.is_contiguous():
            raise ValueError(f"{name} must be a contiguous [{nq}, {W}] int32 / uint32 device tensor")
    if q.dim() != 2 or q.shape[1] != index.d:
        raise ValueError(f"queries must be [n, {index.d}], got {tuple(q.shape)}")
    if neg_cache is not None:
        _dev.require_device("neg_cache", neg_cache)
        if neg_cache.dtype != torch.int32 or tuple(neg_cache.shape) != (nq, n_neg) or not neg_cache.is_contiguous():
            raise ValueError(f"neg_cache must be a contiguous [{nq}, {n_neg}] int32 device tensor")
    if qid is not None:
        qid = _dev.require_device("qid", qid).to(dev, torch.int32).contiguous()
        if qid.numel() != nq:
            raise ValueError(f"qid must have one entry per query ({nq})")
    lib = _lib.load()
    pos_idx = torch.empty(nq, dtype=torch.int64, device=dev)
    neg_idx = torch.empty(nq, n_neg, dtype=torch.int32, device=dev)
    neg_cnt = torch.empty(nq, dtype=torch.int32, device=dev)
    d_pos = torch.empty(nq, dtype=torch.float32, device=dev)
    cand = torch.empty(nq, W, dtype=torch.int32, device=dev) if want_cand else None
    if nq:
        nbytes = int(lib.kp2d_vpr_mine_scratch_bytes(nq, ndb, index.d, n_neg, n_neg_factor))
        if scratch is None or scratch.numel() < nbytes:
            scratch = _dev.scratch(nbytes, dev)
        _lib.check(lib.kp2d_vpr_mine(_ptr(index._p) if ndb else None, _ptr(index._x) if ndb else None, ndb, index.d, _ptr(q), nq,
                                     _ptr(qid), _ptr(pos_mask) if ndb else None, _ptr(neg_mask) if ndb else None, _ptr(neg_cache),
                                     n_sample, n_neg, n_neg_factor, margin, seed, round, PRECISIONS[index.precision],
                                     _ptr(pos_idx), _ptr(neg_idx), _ptr(neg_cnt), _ptr(d_pos), _ptr(cand) if ndb else None,
                                     _ptr(scratch), scratch.numel(), _stream(dev)))
    return pos_idx, neg_idx, neg_cnt, d_pos, cand


class TripletMiner:
    """The mining half of the reference's ``QueryDatasetFromStruct`` (pittsburgh.py:234-333) on the device.  Built from
    the positions alone, it carries the reference's attributes: ``queries`` (the queries with at least one non-trivial
    positive), ``nontrivial_positives`` and ``potential_negatives`` (lists of sorted index arrays, materialised from the
    masks on first access) and ``negCache`` (here one device tensor [numQ, nNeg] int32 padded with -1).

    ``mine(dbFeat, qFeat)`` runs one round for every query (or for ``queries``) and returns device tensors
    ``pos_idx [n] int64`` (-1: no non-trivial positive), ``neg_idx [n, nNeg] int32`` padded with -1, ``neg_cnt [n] int32``
    (0: the reference's ``return None``) and ``d_pos [n]`` (Euclidean; NaN without a positive).  ``negCache`` rows are
    replaced only where ``neg_cnt > 0``; the round counter advances per call.  Draws: the reference's algorithm, a
    counter-based hash of (seed, round, query, draw) in place of numpy's stream."""

    def __init__(self, utmDb, utmQ, posDistThr, nonTrivPosDistSqThr, nNegSample=1000, nNeg=10, margin=0.1, nNegFactor=10,
                 seed=1234, precision="f16x3", device="cuda:0"):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        if nNeg < 1 or nNegFactor < 1 or nNeg * nNegFactor > MAX_CANDIDATES:
            raise ValueError(f"nNeg * nNegFactor = {nNeg * nNegFactor} outside [1, {MAX_CANDIDATES}]")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TripletMiner runs on the HIP device only (no CPU fallback)")
        utmDb, utmQ = np.asarray(utmDb, np.float64), np.asarray(utmQ, np.float64)
        self.numDb, self.numQ = utmDb.shape[0], utmQ.shape[0]
        self.nNegSample, self.nNeg, self.margin, self.nNegFactor = int(nNegSample), int(nNeg), float(margin), int(nNegFactor)
        self.seed, self.precision, self.round = int(seed), precision, 0
        self.pos_mask = radius_neighbors(utmDb, utmQ, float(nonTrivPosDistSqThr) ** 0.5, device=self.device)
        self.neg_mask = radius_neighbors(utmDb, utmQ, posDistThr, invert=True, device=self.device)
        self.queries = np.where(self.pos_mask.count.cpu().numpy() > 0)[0]
        self.negCache = torch.full((self.numQ, self.nNeg), -1, dtype=torch.int32, device=self.device)
        self.last = None            # (query numbers, pos_idx, neg_idx, neg_cnt, d_pos) of the latest round
        self.last_cand = None       # its candidate masks, when asked for
        self._index = self._scratch = self._pos_lists = self._neg_lists = None

    @property
    def nontrivial_positives(self):
        if self._pos_lists is None:
            self._pos_lists = list(self.pos_mask.index_arrays())
        return self._pos_lists

    @property
    def potential_negatives(self):
        if self._neg_lists is None:
            self._neg_lists = list(self.neg_mask.index_arrays())
        return self._neg_lists

    def mine(self, dbFeat, qFeat=None, queries=None, want_cand=False):
        """``dbFeat`` [numDb, d] and ``qFeat`` [numQ, d] device tensors, or one [numDb + numQ, d] tensor in the reference's
        cache layout (queries after the database).  ``queries``: the query numbers to mine (default: all numQ)."""
        _dev.require_device("mine", dbFeat)
        if qFeat is None:
            if dbFeat.shape[0] != self.numDb + self.numQ:
                raise ValueError(f"a single feature tensor must have numDb + numQ = {self.numDb + self.numQ} rows")
            dbFeat, qFeat = dbFeat[:self.numDb], dbFeat[self.numDb:]
        _dev.require_device("mine", qFeat)
        if dbFeat.shape[0] != self.numDb or qFeat.shape[0] != self.numQ:
            raise ValueError(f"dbFeat must be [{self.numDb}, d] and qFeat [{self.numQ}, d]")
        if self._index is None or self._index.d != dbFeat.shape[1]:
            self._index = FlatL2Index(dbFeat.shape[1], device=self.device, precision=self.precision)
        self._index.reset()
        self._index.add(dbFeat)
        pos, neg, cache, qid = self.pos_mask.mask, self.neg_mask.mask, self.negCache, None
        if queries is not None:
            qid = torch.as_tensor(np.asarray(queries), dtype=torch.int64).to(self.device)
            qFeat, pos, neg, cache = qFeat[qid], pos[qid].contiguous(), neg[qid].contiguous(), cache[qid].contiguous()
        out = mine_round(self._index, qFeat, pos, neg, cache, qid, self.nNegSample, self.nNeg, self.nNegFactor, self.margin,
                         self.seed, self.round, want_cand)
        pos_idx, neg_idx, neg_cnt, d_pos, self.last_cand = out
        keep = torch.where((neg_cnt > 0)[:, None], neg_idx, cache)     # the reference leaves the cache alone on `return None`
        if qid is None:
            self.negCache = keep
        else:
            self.negCache[qid] = keep
        self.last = (np.arange(self.numQ) if queries is None else np.asarray(queries), pos_idx, neg_idx, neg_cnt, d_pos)
        self.round += 1
        return pos_idx, neg_idx, neg_cnt, d_pos

    def triplets(self):
        """Yields ``[index, posIndex] + negIndices`` for every query of the latest round that has a triplet — what the
        reference's ``__getitem__`` returns besides the images (pittsburgh.py:351)."""
        if self.last is None:
            raise RuntimeError("mine() first")
        ids, pos_idx, neg_idx, neg_cnt, _ = self.last
        pos_idx, neg_idx, neg_cnt = pos_idx.cpu().numpy(), neg_idx.cpu().numpy(), neg_cnt.cpu().numpy()
        for i, q in enumerate(ids):
            if neg_cnt[i] > 0:
                yield [int(q), int(pos_idx[i])] + neg_idx[i, :neg_cnt[i]].tolist()
