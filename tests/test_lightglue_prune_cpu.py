"""Point pruning (width_confidence > 0) of the LightGlue restatement, on the CPU: tests/lightglue_prune_ref.py against the
unpruned oracle where nothing is pruned, against a second formulation that masks instead of selecting, and the host
helper unpad_pruned.  (Parity unpinned, as every LightGlue test: the reference's lightglue.py cannot be imported here.)"""
import numpy as np
import pytest
import torch

import lightglue_prune_ref as ref
from oracle import lightglue_oracle as lg
from test_lightglue_oracle import make_data

# (M, N, seed, width_confidence) for config S, seeded weights: oracle margin >= 1e-3 (tests/test_gpu_lightglue_prune.py)
CASES = [(70, 45, 11, 0.6), (70, 45, 3, 0.6), (128, 128, 3, 0.6), (33, 64, 5, 0.55)]


def f64(data, sd):
    p = {k: v.astype(np.float64) for k, v in sd.items()}
    d = {k: ({"image_size": v["image_size"].astype(np.float64)} if isinstance(v, dict) else v.astype(np.float64))
         for k, v in data.items()}
    return d, p


def setup(name, M, N, seed, th=0.0):
    conf = lg.get_config(dict(lg.LIGHT_GLUE_CONFIGS[name], filter_threshold=th))
    sd = lg.seeded_state_dict(conf)
    return conf, sd, make_data(1, M, N, conf["input_dim"], seed=seed)


@pytest.mark.parametrize("M,N,seed,wc", CASES)
def test_nothing_pruned_equals_the_unpruned_oracle(M, N, seed, wc):
    """width_confidence = 0.95: every score of the seeded S weights is above 0.05 on these inputs, so every index_select is
    the identity and the pruned forward IS the unpruned one, bit for bit; prune == n_layers."""
    conf, sd, data = setup("S", M, N, seed, th=0.1)
    got, want = ref.forward_pruned(data, sd, conf, 0.95), lg.forward(data, sd, conf)
    for _, _, _, s in got["pairs"][0]["scores_seen"]:
        assert s.min() > 0.05
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "log_assignment", "ref_descriptors0",
              "ref_descriptors1"):
        assert np.array_equal(got[k], want[k]), k
    assert np.all(got["prune0"] == conf["n_layers"]) and np.all(got["prune1"] == conf["n_layers"])
    assert got["prune0"].dtype == np.int64
    assert np.array_equal(got["keep0"][0], np.arange(M)) and np.array_equal(got["keep1"][0], np.arange(N))


def masked_forward(data, p, conf, wc):
    """Second formulation: no row is ever removed.  Arrays keep their full size; a pruned point is masked with -inf as a
    KEY of every later attention and as a row / column of the assignment.  Returns the alive masks after every layer."""
    k0 = lg.normalize_keypoints(data["keypoints0"], data["view0"]["image_size"])
    k1 = lg.normalize_keypoints(data["keypoints1"], data["view1"]["image_size"])
    x = [data["descriptors0"], data["descriptors1"]]
    enc = [lg.posenc(k0, p), lg.posenc(k1, p)]
    h, d, nl = conf["num_heads"], conf["descriptor_dim"], conf["n_layers"]
    hd = d // h
    alive = [np.ones(x[0].shape[1], bool), np.ones(x[1].shape[1], bool)]
    history = []

    def attend(q, k, v, key_alive):
        s = np.einsum("bhid,bhjd->bhij", q, k) * hd ** -0.5
        s = np.where(key_alive[None, None, None, :], s, -np.inf)
        return lg.softmax(s, -1) @ v

    heads = lambda t: t.reshape(t.shape[0], t.shape[1], h, hd).transpose(0, 2, 1, 3)
    merge = lambda t: t.transpose(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], d)
    for i in range(nl):
        for s in range(2):
            pre = f"transformers.{i}.self_attn"
            qkv = lg.linear(x[s], p, f"{pre}.Wqkv").reshape(1, -1, h, hd, 3).transpose(0, 2, 1, 3, 4)
            q, k, v = lg.apply_rotary(enc[s], qkv[..., 0]), lg.apply_rotary(enc[s], qkv[..., 1]), qkv[..., 2]
            msg = lg.linear(merge(attend(q, k, v, alive[s])), p, f"{pre}.out_proj")
            x[s] = x[s] + lg.ffn(np.concatenate([x[s], msg], -1), p, f"{pre}.ffn")
        pre = f"transformers.{i}.cross_attn"
        qk = [heads(lg.linear(t, p, f"{pre}.to_qk")) for t in x]
        vv = [heads(lg.linear(t, p, f"{pre}.to_v")) for t in x]
        msg = [lg.linear(merge(attend(qk[s], qk[1 - s], vv[1 - s], alive[1 - s])), p, f"{pre}.to_out") for s in range(2)]
        x = [x[s] + lg.ffn(np.concatenate([x[s], msg[s]], -1), p, f"{pre}.ffn") for s in range(2)]
        if i < nl - 1:
            for s in range(2):
                sc = ref.sigmoid(lg.linear(x[s], p, f"log_assignment.{i}.matchability"))[0, :, 0]
                alive[s] = alive[s] & (sc > 1 - wc)
            history.append([a.copy() for a in alive])
    pre = f"log_assignment.{nl - 1}"
    f = [lg.linear(t, p, f"{pre}.final_proj") / d ** 0.25 for t in x]
    z = [lg.linear(t, p, f"{pre}.matchability")[0, :, 0] for t in x]
    sim = f[0][0] @ f[1][0].T
    sim = np.where(alive[0][:, None] & alive[1][None, :], sim, -np.inf)
    with np.errstate(invalid="ignore"):
        inner = lg.log_softmax(sim, 1) + lg.log_softmax(sim, 0) + lg.log_sigmoid(z[0])[:, None] + lg.log_sigmoid(z[1])[None, :]
    return x, alive, history, inner, z


@pytest.mark.parametrize("M,N,seed,wc", CASES)
def test_selecting_rows_equals_masking_keys_in_float64(M, N, seed, wc):
    conf, sd, data = setup("S", M, N, seed)
    d64, p64 = f64(data, sd)
    got = ref.forward_pruned(d64, p64, conf, wc)
    x, alive, history, inner, z = masked_forward(d64, p64, conf, wc)
    i0, i1 = np.nonzero(alive[0])[0], np.nonzero(alive[1])[0]
    m, n = len(i0), len(i1)
    assert 0 < m < M and 0 < n < N                                # the case must prune something and leave something
    assert np.array_equal(got["keep0"][0, :m], i0) and np.all(got["keep0"][0, m:] == -1)
    assert np.array_equal(got["keep1"][0, :n], i1) and np.all(got["keep1"][0, n:] == -1)
    assert got["num_kept0"][0] == m and got["num_kept1"][0] == n
    assert np.all(np.diff(got["keep0"][0, :m]) > 0) and np.all(np.diff(got["keep1"][0, :n]) > 0)
    assert np.max(np.abs(got["ref_descriptors0"][0, 0, :m] - x[0][0, i0])) < 1e-9
    assert np.max(np.abs(got["ref_descriptors1"][0, 0, :n] - x[1][0, i1])) < 1e-9
    block = inner[np.ix_(i0, i1)]
    la = got["log_assignment"][0]
    assert np.max(np.abs(la[:m, :n] - block)) < 1e-9
    assert np.all(np.isneginf(la[:M, :N][m:])) and np.all(np.isneginf(la[:M, :N][:, n:]))
    assert np.max(np.abs(la[:m, N] - lg.log_sigmoid(-z[0][i0]))) < 1e-9
    assert np.max(np.abs(la[M, :n] - lg.log_sigmoid(-z[1][i1]))) < 1e-9
    # matches: filter_matches on the survivors' block, named by original indices
    scores = np.zeros((1, m + 1, n + 1))
    scores[0, :m, :n] = block
    m0, m1, ms0, ms1 = lg.filter_matches(scores, conf["filter_threshold"])
    want0 = np.full(M, -1)
    want0[i0] = np.where(m0[0] < 0, -1, i1[np.clip(m0[0], 0, None)])
    want1 = np.full(N, -1)
    want1[i1] = np.where(m1[0] < 0, -1, i0[np.clip(m1[0], 0, None)])
    assert np.array_equal(got["matches0"][0], want0) and np.array_equal(got["matches1"][0], want1)
    s0 = np.zeros(M)
    s0[i0] = ms0[0]
    assert np.max(np.abs(got["matching_scores0"][0] - s0)) < 1e-9
    assert np.all(got["matches0"][0][~alive[0]] == -1) and np.all(got["matching_scores0"][0][~alive[0]] == 0)
    # prune: a point dropped after layer i holds i + 1, a survivor n_layers
    for s, key in ((0, "prune0"), (1, "prune1")):
        want = np.ones(len(alive[s]), np.int64)
        for layer_alive in history:
            want += layer_alive[s]
        assert np.array_equal(got[key][0], want)
        assert np.all(got[key][0][alive[s]] == conf["n_layers"]) and np.all(got[key][0][~alive[s]] < conf["n_layers"])
    assert got["margin"] >= 1e-3


def test_empty_set_fails_in_the_reference_formulation():
    """(1, 40, seed 5, wc 0.6): the single point of set 0 is pruned; the reference's forward cannot go on from there."""
    conf, sd, data = setup("S", 1, 40, 5)
    with pytest.raises(ValueError):
        ref.forward_pruned(data, sd, conf, 0.6)


def test_unpad_pruned_shapes_and_entries():
    from lightglue.lightglue import unpad_pruned
    B, M, N, D = 2, 5, 4, 3
    g = torch.Generator().manual_seed(0)
    pred = {"log_assignment": torch.randn(B, M + 1, N + 1, generator=g),
            "ref_descriptors0": torch.randn(B, 1, M, D, generator=g), "ref_descriptors1": torch.randn(B, 1, N, D, generator=g),
            "matches0": torch.tensor([[-1, 2, -1, -1, 0], [3, -1, -1, -1, -1]]), "matches1": torch.tensor([[4, -1, 1, -1], [-1, -1, -1, 0]]),
            "matching_scores0": torch.rand(B, M, generator=g), "matching_scores1": torch.rand(B, N, generator=g),
            "prune0": torch.tensor([[1, 4, 2, 4, 4], [4, 1, 1, 4, 2]]), "prune1": torch.tensor([[4, 3, 4, 1], [1, 2, 4, 4]]),
            "keep0": torch.tensor([[1, 3, 4, -1, -1], [0, 3, -1, -1, -1]], dtype=torch.int32),
            "keep1": torch.tensor([[0, 2, -1, -1], [2, 3, -1, -1]], dtype=torch.int32),
            "num_kept0": torch.tensor([3, 2], dtype=torch.int32), "num_kept1": torch.tensor([2, 2], dtype=torch.int32)}
    for b, (m, n) in enumerate([(3, 2), (2, 2)]):
        one = unpad_pruned(pred, b)
        la = one["log_assignment"]
        assert la.shape == (1, m + 1, n + 1)
        assert torch.equal(la[0, :m, :n], pred["log_assignment"][b, :m, :n])
        assert torch.equal(la[0, :m, n], pred["log_assignment"][b, :m, N])          # the dustbin column
        assert torch.equal(la[0, m, :n], pred["log_assignment"][b, M, :n])          # the dustbin row
        assert la[0, m, n] == pred["log_assignment"][b, M, N]
        assert one["ref_descriptors0"].shape == (1, 1, m, D) and one["ref_descriptors1"].shape == (1, 1, n, D)
        assert torch.equal(one["ref_descriptors0"][0, 0], pred["ref_descriptors0"][b, 0, :m])
        assert torch.equal(one["ind0"][0], pred["keep0"][b, :m].long()) and one["ind1"].shape == (1, n)
        assert torch.equal(one["matches0"], pred["matches0"][b:b + 1]) and one["prune1"].shape == (1, N)
