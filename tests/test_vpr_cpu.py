"""Place recognition without a device: the reference's Recall@N / AUC / MatchRatio, the float64 top-k and the error
bound the GPU tests (tests/test_gpu_vpr.py) use, shown to be tight, and the argument checks of FlatL2Index."""
import numpy as np
import pytest
import torch

import vpr_ref as vr
from nano_vs_slam_amd.vpr import FlatL2Index, recall_at_n


def literal(predictions, gt, num_q, n_values):
    """global_descriptor.py:73-106 once more, as written there (np.in1d included where numpy still has it)."""
    in1d = np.isin          # (np.in1d: deprecated alias of the same function for 1-D input)
    n_max = max(n_values)
    match_ratio_at_n = np.zeros(len(n_values))
    count_n = np.zeros(len(n_values))
    correct_hist = np.zeros(n_max)
    for qIx, pred in enumerate(predictions):
        correct_matches = in1d(pred[:n_max], gt[qIx])
        total_matches = len(gt[qIx])
        match_idxs = np.where(correct_matches)
        if np.any(correct_matches):
            first_hit = match_idxs[0].min()
            correct_hist[first_hit:] += 1
        for i, n in enumerate(n_values):
            if total_matches > 0:
                match_ratio_at_n[i] += sum(correct_matches[:n]) / min(total_matches, n)
                count_n[i] += 1
    match_ratio_at_n = match_ratio_at_n / count_n
    recall_hist = correct_hist / num_q
    return ({n: recall_hist[n - 1] for n in n_values}, {n: np.sum(recall_hist[:n]) / n for n in n_values},
            {n: match_ratio_at_n[i] for i, n in enumerate(n_values)})


def test_recall_hand_cases():
    # q0: hit at rank 1; q1: first hit at rank 3 (index 2); q2: no positives at all; q3: positives, never retrieved
    pred = np.array([[5, 1, 2, 3], [9, 8, 4, 4], [0, 1, 2, 3], [7, 7, 7, 7]])
    gt = [np.array([5, 2]), np.array([4]), np.array([], np.int64), np.array([1, 2, 3, 6, 9])]
    r = recall_at_n(pred, gt, 4, n_values=(1, 2, 3, 4))
    assert r["Recall"] == {1: 0.25, 2: 0.25, 3: 0.5, 4: 0.5}
    assert r["AUC"][4] == pytest.approx((0.25 + 0.25 + 0.5 + 0.5) / 4)
    # MatchRatio over the three queries with positives; n larger than a query's positives divides by len(gt)
    assert r["MatchRatio"][1] == pytest.approx((1 / 1 + 0 + 0) / 3)
    assert r["MatchRatio"][3] == pytest.approx((2 / 2 + 1 / 1 + 0) / 3)
    assert r["MatchRatio"][4] == pytest.approx((2 / 2 + 2 / 1 + 0) / 3)      # a repeated hit counts twice, as there


def test_recall_matches_literal_restatement():
    rng = np.random.default_rng(3)
    for trial in range(20):
        nq, ndb = int(rng.integers(1, 40)), int(rng.integers(20, 60))
        pred = np.stack([rng.permutation(ndb)[:20] for _ in range(nq)])
        if trial % 3 == 0:
            pred[:, -3:] = -1                                   # faiss's padding
        gt = [rng.choice(ndb, size=int(rng.integers(0, 8)), replace=False) for _ in range(nq)]
        num_q = nq + int(rng.integers(0, 3))
        r = recall_at_n(pred, gt, num_q)
        with np.errstate(invalid="ignore", divide="ignore"):
            rec, auc, mr = literal(pred, gt, num_q, [1, 5, 10, 20])
        assert r["Recall"] == rec and r["AUC"] == auc
        for n in mr:
            assert (np.isnan(mr[n]) and np.isnan(r["MatchRatio"][n])) or mr[n] == r["MatchRatio"][n]


def test_topk64_order_and_padding():
    db = np.array([[0.0] * 16, [1.0] * 16, [0.0] * 16, [2.0] * 16], np.float32)
    q = np.zeros((2, 16), np.float32)
    d = vr.distances64(db, q)
    D, I = vr.topk64(d, 6, limit=[4, 1])
    assert I[0].tolist() == [0, 2, 1, 3, -1, -1] and D[0, :4].tolist() == [0, 0, 16, 64]
    assert I[1].tolist() == [0, -1, -1, -1, -1, -1] and np.isinf(D[1, 1:]).all()


def same_sign_residuals(rng, n, dim):
    """Positive rows (GeM-like) whose every element lies just above an fp16 number at the row's scale: every lo half
    is positive, so a lost split term adds up instead of cancelling — the case a bound must be able to see."""
    x = rng.uniform(0.5, 1.0, (n, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    hi, lo, u = vr.split_rows(x)
    return ((hi + np.abs(lo) + np.float32(2.0 ** -13) * np.abs(hi)) * u[:, None]).astype(np.float32)


@pytest.mark.parametrize("dim", [768, 4096])
def test_bound_is_tight(dim):
    rng = np.random.default_rng(dim)
    for kind in ("gauss", "residual"):
        if kind == "gauss":
            db = rng.standard_normal((96, dim)).astype(np.float32)
            db /= np.linalg.norm(db, axis=1, keepdims=True)
            q = rng.standard_normal((6, dim)).astype(np.float32)
            q /= np.linalg.norm(q, axis=1, keepdims=True)
            q[0] = db[3] + np.float32(1e-3) * q[0]              # a near-duplicate
        else:
            db = same_sign_residuals(rng, 96, dim)
            q = same_sign_residuals(rng, 6, dim)
        d64 = vr.distances64(db, q)
        key64 = d64 - (np.asarray(q, np.float64) ** 2).sum(1)[:, None]
        eps = vr.eps_key(db, q, split=True)
        ok = np.abs(vr.emulate_keys(db, q) - key64) / eps
        assert ok.max() < 0.5, (kind, ok.max())
        if kind == "residual":
            for fault in ("drop_cross", "flush_lo"):
                r = np.abs(vr.emulate_keys(db, q, **{fault: True}) - key64) / eps
                assert r.max() > 8, (fault, r.max())
        r = np.abs(vr.emulate_keys(db, q, skip_rescale=True) - key64) / eps
        assert r.max() > 1e3


@pytest.mark.parametrize("scale", [1e5, 1e-6])
def test_bound_holds_across_magnitude(scale):
    rng = np.random.default_rng(7)
    db = (rng.standard_normal((64, 1536)) * scale).astype(np.float32)
    q = (rng.standard_normal((4, 1536)) * scale).astype(np.float32)
    key64 = vr.distances64(db, q) - (np.asarray(q, np.float64) ** 2).sum(1)[:, None]
    assert (np.abs(vr.emulate_keys(db, q) - key64) / vr.eps_key(db, q, split=True)).max() < 0.25


def test_argument_checks_need_no_device():
    for d in (0, 8, 100, 770, 16400):
        with pytest.raises(ValueError):
            FlatL2Index(d)
    with pytest.raises(RuntimeError):
        FlatL2Index(768, device="cpu")
    with pytest.raises(ValueError):
        FlatL2Index(768, precision="bf16")
    ix = FlatL2Index(768)
    for k in (0, -1, 1025):
        with pytest.raises(ValueError):
            ix.search(np.zeros((1, 768), np.float32), k)
    with pytest.raises(RuntimeError):
        ix.add(torch.zeros(2, 768))
    with pytest.raises(RuntimeError):
        ix.search(torch.zeros(2, 768), 5)
    with pytest.raises(ValueError):
        ix.add(np.zeros((2, 512), np.float32))
    assert ix.ntotal == 0 and ix.d == 768


def test_reference_import_line_resolves_without_faiss():
    import importlib
    import os
    import sys
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "src")
    sys.path.insert(0, src)
    try:
        mod = importlib.import_module("evaluation.global_descriptor")
    finally:
        sys.path.remove(src)
    from nano_vs_slam_amd import vpr
    assert mod.evaluate_global_descriptor is vpr.evaluate_global_descriptor
    assert "faiss" not in sys.modules
