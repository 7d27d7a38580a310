"""Place recognition on the device — the retrieval step behind the global descriptor (`vlad`).

* ``FlatL2Index`` — faiss.IndexFlatL2's surface (``d``, ``ntotal``, ``add``, ``search``, ``reset``) on the HIP kernels of
  csrc/vpr.hip (kp2d_vpr_pack / kp2d_vpr_search / kp2d_vpr_search_masked, include/kp2d.h): exact brute-force squared L2, the database resident in
  HBM, a fused top-k that never writes the Q x N distance matrix.
* ``recall_at_n`` — Recall@N / AUC / MatchRatio exactly as the reference computes them
  (src/evaluation/global_descriptor.py:58-106), quirks included.
* ``evaluate_global_descriptor`` — drop-in for the reference function (global_descriptor.py:8-106) with this index in
  place of faiss.

There is no CPU path: CPU tensors raise, like the rest of the product.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _dev, _lib
from ._dev import ptr as _ptr, stream as _stream

VPR_FP32 = 1
PRECISIONS = {"f16x3": 0, "fp32": VPR_FP32}
MAX_K = 1024


def check_dim(d: int) -> int:
    d = int(d)
    if d < 16 or d > 16384 or d % 16:
        raise ValueError(f"descriptor dim {d} unsupported: needs d % 16 == 0 and 16 <= d <= 16384")
    return d


def row_bytes(d: int) -> int:
    """Bytes of one packed database row (|x|^2, scale and guard bit, then the split-fp16 hi and lo planes)."""
    return 4 * d + 16


class FlatL2Index:
    """faiss.IndexFlatL2 on the MI355X.  ``precision``: "f16x3" (split-fp16 keys, the default) or "fp32" (exact fp32
    products); both return the k finalists' distances re-scored in fp32 and sorted ascending, equal distances by lower
    row, padding (FLT_MAX, -1) where fewer than k rows exist (include/kp2d.h, kp2d_vpr_search)."""

    def __init__(self, d: int, device="cuda:0", precision: str = "f16x3"):
        self.d = check_dim(d)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("FlatL2Index runs on the HIP device only (no CPU fallback)")
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        self.precision = precision
        self.reset()

    def reset(self) -> None:
        self.ntotal = 0
        self._x = None          # [capacity, d] float32
        self._p = None          # [capacity * row_bytes(d)] uint8
        self._scratch = None

    def _rows(self, x, what):
        """numpy / device tensor [n, d] -> (contiguous float32 device tensor, input was numpy)."""
        if isinstance(x, np.ndarray):
            t, is_np = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), True
            if t.dim() != 2 or t.shape[1] != self.d:
                raise ValueError(f"{what} must be [n, {self.d}], got {tuple(t.shape)}")
            t = t.to(self.device)
        elif isinstance(x, torch.Tensor):
            _dev.require_device(what, x, "pass numpy or a device tensor")
            if x.dim() != 2 or x.shape[1] != self.d:
                raise ValueError(f"{what} must be [n, {self.d}], got {tuple(x.shape)}")
            t, is_np = x.to(self.device, torch.float32).contiguous(), False
        else:
            raise TypeError(f"{what} must be a numpy array or a torch tensor")
        return t, is_np

    def add(self, x) -> None:
        x, _ = self._rows(x, "add")
        n = x.shape[0]
        if n == 0:
            return
        lib = _lib.load()
        need = self.ntotal + n
        cap = 0 if self._x is None else self._x.shape[0]
        if need > cap:                                   # amortised growth: the rows already there are copied, not repacked
            cap = max(need, 2 * cap, 1024)
            nx = torch.empty(cap, self.d, dtype=torch.float32, device=self.device)
            npk = torch.empty(cap * row_bytes(self.d), dtype=torch.uint8, device=self.device)
            if self.ntotal:
                nx[:self.ntotal] = self._x[:self.ntotal]
                npk[:self.ntotal * row_bytes(self.d)] = self._p[:self.ntotal * row_bytes(self.d)]
            self._x, self._p = nx, npk
        self._x[self.ntotal:need] = x
        dst = self._p[self.ntotal * row_bytes(self.d):]
        _lib.check(lib.kp2d_vpr_pack(_ptr(self._x[self.ntotal:need]), n, self.d, _ptr(dst), _stream(self.device)))
        self.ntotal = need

    def search(self, x, k: int, limit=None, mask=None):
        """-> (D [nq, k] squared L2 distances, I [nq, k] row indices); numpy in -> numpy out (float32 / int64), device
        tensors in -> device tensors out.  ``limit`` [nq] (optional): query i only sees rows [0, limit[i]).  ``mask``
        (optional, not with ``limit``): a mining.RowMask or a [nq, ceil(ntotal / 32)] int32 / uint32 device tensor of row
        bits (include/kp2d.h, kp2d_vpr_search_masked): query i only sees the rows whose bit is set."""
        if limit is not None and mask is not None:
            raise ValueError("search takes limit or mask, not both")
        k = int(k)
        if k < 1 or k > MAX_K:
            raise ValueError(f"k = {k} outside [1, {MAX_K}]")
        q, is_np = self._rows(x, "search")
        nq = q.shape[0]
        lim = None
        if limit is not None:
            lim = torch.as_tensor(np.asarray(limit) if not isinstance(limit, torch.Tensor) else limit)
            if isinstance(limit, torch.Tensor):
                _dev.require_device("search", lim, None)
            lim = lim.to(self.device, torch.int64).contiguous().reshape(-1)
            if lim.numel() != nq:
                raise ValueError(f"limit must have one entry per query ({nq}), got {lim.numel()}")
        if mask is not None:
            words = getattr(mask, "mask", mask)
            if not isinstance(words, torch.Tensor):
                raise TypeError("mask must be a RowMask or a device tensor")
            _dev.require_device("search", words, None)
            if words.dtype not in (torch.int32, torch.uint32) or tuple(words.shape) != (nq, (self.ntotal + 31) // 32):
                raise ValueError(f"mask must be [{nq}, {(self.ntotal + 31) // 32}] int32 / uint32, got {words.dtype} {tuple(words.shape)}")
            words = words.to(self.device).contiguous()
        D = torch.empty(nq, k, dtype=torch.float32, device=self.device)
        I = torch.empty(nq, k, dtype=torch.int64, device=self.device)
        if nq:
            lib = _lib.load()
            nbytes = int(lib.kp2d_vpr_scratch_bytes(nq, self.ntotal, self.d, k))
            if self._scratch is None or self._scratch.numel() < nbytes:
                self._scratch = _dev.scratch(nbytes, self.device)
            call, sel = (lib.kp2d_vpr_search, lim) if mask is None else (lib.kp2d_vpr_search_masked, words if self.ntotal else None)
            _lib.check(call(_ptr(self._p) if self.ntotal else None, _ptr(self._x) if self.ntotal else None,
                            self.ntotal, self.d, _ptr(q), nq, _ptr(sel), k, PRECISIONS[self.precision],
                            _ptr(D), _ptr(I), _ptr(self._scratch), self._scratch.numel(), _stream(self.device)))
        if is_np:
            return D.cpu().numpy(), I.cpu().numpy()
        return D, I


def recall_at_n(predictions, gt, num_q, n_values=(1, 5, 10, 20)):
    """Recall@N, AUC and MatchRatio of ranked predictions [numQ, >= max(n_values)] against positives gt[q] — the
    reference's loop (global_descriptor.py:58-106) restated line by line: a query's first hit at rank r counts for every
    N > r (``correct_hist[first_hit:] += 1``), the histogram is divided by ``num_q``, and MatchRatio is averaged over the
    queries that have positives only, each divided by ``min(len(gt[q]), n)``."""
    n_values = list(n_values)
    n_max = max(n_values)
    match_ratio_at_n = np.zeros(len(n_values))
    count_n = np.zeros(len(n_values))
    correct_hist = np.zeros(n_max)
    for q_ix, pred in enumerate(predictions):
        correct_matches = np.isin(np.asarray(pred)[:n_max], gt[q_ix])
        total_matches = len(gt[q_ix])
        match_idxs = np.where(correct_matches)
        if np.any(correct_matches):
            first_hit = match_idxs[0].min()
            correct_hist[first_hit:] += 1
        for i, n in enumerate(n_values):
            if total_matches > 0:
                match_ratio_at_n[i] += sum(correct_matches[:n]) / min(total_matches, n)
                count_n[i] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        match_ratio_at_n = match_ratio_at_n / count_n
    recall_hist = correct_hist / num_q
    recalls, auc, match_ratio = {}, {}, {}
    for i, n in enumerate(n_values):
        recalls[n] = recall_hist[n - 1]
        auc[n] = np.sum(recall_hist[:n]) / n
        match_ratio[n] = match_ratio_at_n[i]
    return {"Recall": recalls, "AUC": auc, "MatchRatio": match_ratio}


def evaluate_global_descriptor(model, eval_set, batch_size=4, device="cuda", num_workers=8, precision="f16x3"):
    """Drop-in for the reference's evaluate_global_descriptor (src/evaluation/global_descriptor.py:8-106).
    eval_set: items (img, index), ``dbStruct.numDb`` / ``dbStruct.numQ``, ``getPositives()``; the first numDb items are
    the database, the rest the queries.  The descriptors stay on the device: ``vlad`` of every batch goes straight into a
    FlatL2Index (post_processing passes ``vlad`` through unchanged, so it is not run).  Prints the reference's lines and
    returns its dict {"Recall", "AUC", "MatchRatio"} keyed by N in (1, 5, 10, 20)."""
    from torch.utils.data import DataLoader
    loader = DataLoader(dataset=eval_set, shuffle=False, batch_size=batch_size, pin_memory=True, num_workers=num_workers)
    model.eval()
    pool_size = model.get_global_desc_dim()
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    feats = torch.empty(len(eval_set), pool_size, dtype=torch.float32, device=dev)
    with torch.no_grad():
        for img, indices in loader:
            out = model(img.to(dev))
            vlad = out["vlad"]
            feats[indices.to(dev, torch.int64)] = vlad.reshape(vlad.shape[0], -1).float()
    num_db = eval_set.dbStruct.numDb
    index = FlatL2Index(pool_size, device=dev, precision=precision)
    index.add(feats[:num_db])
    n_values = [1, 5, 10, 20]
    _, predictions = index.search(feats[num_db:], max(n_values))
    res = recall_at_n(predictions.cpu().numpy(), eval_set.getPositives(), eval_set.dbStruct.numQ, n_values)
    for n in n_values:
        print("====> Recall@{}: {:.4f} AUC: {:.4f} MR: {:.4f}".format(n, res["Recall"][n], res["AUC"][n], res["MatchRatio"][n]))
    return res
