"""numpy restatement of the reference's LightGlue forward WITH point pruning (width_confidence > 0, eval mode), built from
oracle/lightglue_oracle.py's own blocks.  Test infrastructure, shared by test_lightglue_prune_cpu.py and
test_gpu_lightglue_prune.py.

Everything cites the reference's lightglue/lightglue.py:
  :535         do_point_pruning = width_confidence > 0 and not training
  :539-544     ind = arange, prune = ones_like(ind) (int64)
  :553-556     no pruning after the last layer
  :564-579     per set: scores = log_assignment[i].get_matchability(desc) (:395-396: sigmoid(matchability(desc))),
               keep = where(mask), index_select of ind / desc / encoding, prune[:, ind] += 1
  :618-625     get_pruning_mask: keep = scores > 1 - width_confidence; the token-confidence term is absent (confidences
               is None without early stopping)
  :581-583     log_assignment[n_layers - 1] and filter_matches on the survivors
  :585-594     matches mapped back through ind0 / ind1, dropped points -1 / 0
The reference asserts b == 1 (:565); a batch is run pair by pair here.  The results come back in the PADDED layout of the
device entry point (include/kp2d_lightglue.h kp2d_lg_forward_pruned): survivors in the leading rows / columns.
"""
import numpy as np

from oracle import lightglue_oracle as lg


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def forward_one(data, p, conf, wc):
    """One pair (b == 1) in the reference's data-dependent shapes.  Raises ValueError when a set becomes empty, as the
    reference does (max over an empty dimension in filter_matches)."""
    k0, k1 = data["keypoints0"], data["keypoints1"]
    assert k0.shape[0] == 1                                                       # :565
    s0 = data.get("view0", {}).get("image_size")
    s1 = data.get("view1", {}).get("image_size")
    k0, k1 = lg.normalize_keypoints(k0, s0), lg.normalize_keypoints(k1, s1)
    d0, d1 = data["descriptors0"], data["descriptors1"]
    if conf["input_dim"] != conf["descriptor_dim"]:
        d0, d1 = lg.linear(d0, p, "input_proj"), lg.linear(d1, p, "input_proj")
    e0, e1 = lg.posenc(k0, p), lg.posenc(k1, p)
    m, n, h, nl = k0.shape[1], k1.shape[1], conf["num_heads"], conf["n_layers"]
    ind0, ind1 = np.arange(m), np.arange(n)                                       # :540-541
    prune0, prune1 = np.ones(m, np.int64), np.ones(n, np.int64)                   # :543-544
    thr = 1 - wc                                                                  # :622
    margin = np.inf
    scores_seen = []
    for i in range(nl):
        d0 = lg.self_block(d0, e0, p, f"transformers.{i}.self_attn", h)
        d1 = lg.self_block(d1, e1, p, f"transformers.{i}.self_attn", h)
        d0, d1 = lg.cross_block(d0, d1, p, f"transformers.{i}.cross_attn", h)
        if i == nl - 1:                                                           # :553-556
            break
        sc0 = sigmoid(lg.linear(d0, p, f"log_assignment.{i}.matchability"))[0, :, 0]      # :566, :395-396
        keep0 = np.nonzero(sc0 > thr)[0]                                          # :567-568 (ascending, torch.where)
        scores_seen.append((i, 0, ind0.copy(), sc0))
        ind0, d0, e0 = ind0[keep0], d0[:, keep0], e0[..., keep0, :]               # :569-571
        prune0[ind0] += 1                                                         # :572
        sc1 = sigmoid(lg.linear(d1, p, f"log_assignment.{i}.matchability"))[0, :, 0]      # :573
        keep1 = np.nonzero(sc1 > thr)[0]
        scores_seen.append((i, 1, ind1.copy(), sc1))
        ind1, d1, e1 = ind1[keep1], d1[:, keep1], e1[..., keep1, :]               # :576-578
        prune1[ind1] += 1                                                         # :579
        for sc in (sc0, sc1):
            if sc.size:
                margin = min(margin, float(np.abs(sc - thr).min()))
    if ind0.size == 0 or ind1.size == 0:
        raise ValueError("a set is empty after pruning: filter_matches takes max over an empty dimension")
    scores, _ = lg.match_assignment(d0, d1, p, f"log_assignment.{nl - 1}")        # :582
    m0, m1, ms0, ms1 = lg.filter_matches(scores, conf["filter_threshold"])        # :583
    m0_, m1_ = np.full((1, m), -1, np.int64), np.full((1, n), -1, np.int64)       # :586-587
    m0_[:, ind0] = np.where(m0 == -1, -1, ind1[np.clip(m0, 0, None)])             # :588
    m1_[:, ind1] = np.where(m1 == -1, -1, ind0[np.clip(m1, 0, None)])             # :589
    ms0_, ms1_ = np.zeros((1, m), scores.dtype), np.zeros((1, n), scores.dtype)   # :590-591
    ms0_[:, ind0], ms1_[:, ind1] = ms0, ms1                                       # :592-593
    return {"matches0": m0_, "matches1": m1_, "matching_scores0": ms0_, "matching_scores1": ms1_,
            "ref_descriptors0": d0[:, None], "ref_descriptors1": d1[:, None], "log_assignment": scores,
            "prune0": prune0[None], "prune1": prune1[None], "ind0": ind0, "ind1": ind1,
            "survivor_matches0": m0, "margin": margin, "scores_seen": scores_seen}


def pair_of(data, b):
    """Pair b of a batch as a b == 1 input."""
    def view(v):
        s = v["image_size"]
        return {"image_size": s if s is None or np.ndim(s) == 1 else np.asarray(s)[b:b + 1]}
    return {k: view(v) if isinstance(v, dict) else v[b:b + 1] for k, v in data.items()}


def forward_pruned(data, p, conf, wc):
    """A batch, pair by pair, in the padded layout: matches / scores / prune by original index; log_assignment
    [B, M+1, N+1] with the survivors' block in the leading rows / columns, their dustbin entries in column N / row M and
    -inf in the rest of the inner block; ref_descriptors [B, 1, M, D] with the survivors' rows first (zeros after);
    keep0/1 [B, M/N] = original index of survivor j (-1 past the count), num_kept0/1 [B]; margin = the smallest
    |score - (1 - wc)| over every prune decision made."""
    B, M, N = data["keypoints0"].shape[0], data["keypoints0"].shape[1], data["keypoints1"].shape[1]
    D, dt = conf["descriptor_dim"], data["descriptors0"].dtype
    out = {"matches0": np.full((B, M), -1, np.int64), "matches1": np.full((B, N), -1, np.int64),
           "matching_scores0": np.zeros((B, M), dt), "matching_scores1": np.zeros((B, N), dt),
           "ref_descriptors0": np.zeros((B, 1, M, D), dt), "ref_descriptors1": np.zeros((B, 1, N, D), dt),
           "log_assignment": np.zeros((B, M + 1, N + 1), dt),
           "prune0": np.zeros((B, M), np.int64), "prune1": np.zeros((B, N), np.int64),
           "keep0": np.full((B, M), -1, np.int32), "keep1": np.full((B, N), -1, np.int32),
           "num_kept0": np.zeros(B, np.int32), "num_kept1": np.zeros(B, np.int32), "margin": np.inf, "pairs": []}
    out["log_assignment"][:, :M, :N] = -np.inf
    for b in range(B):
        r = forward_one(pair_of(data, b), p, conf, wc)
        m, n = len(r["ind0"]), len(r["ind1"])
        for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "prune0", "prune1"):
            out[k][b] = r[k][0]
        out["ref_descriptors0"][b, 0, :m], out["ref_descriptors1"][b, 0, :n] = r["ref_descriptors0"][0, 0], r["ref_descriptors1"][0, 0]
        la = out["log_assignment"][b]
        la[:m, :n], la[:m, N], la[M, :n] = r["log_assignment"][0, :m, :n], r["log_assignment"][0, :m, n], r["log_assignment"][0, m, :n]
        out["keep0"][b, :m], out["keep1"][b, :n] = r["ind0"], r["ind1"]
        out["num_kept0"][b], out["num_kept1"][b] = m, n
        out["margin"] = min(out["margin"], r["margin"])
        out["pairs"].append(r)
    return out
