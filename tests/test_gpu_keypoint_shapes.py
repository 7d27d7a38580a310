"""The keypoint loss on the device (nano_vs_slam_amd.keypoint_training.keypoint_loss, csrc/keypoint_train.hip) at the cases of
keypoint_shapes_ref: more than 64 channels (every chunk count and last-chunk width of kd_search, the u >= 1 passes of the
wave-per-anchor kernels), more than one tile of every scan (kl_nearest, kl_target_grad, kd_search, kd_tar_grad, kd_feat_grad,
with full and ragged last tiles), exact ties of a_i and of the descriptor distances, and one column as the negative of most
anchors.

Every call gets its own scratch of exactly the stated size in front of 4096 guard bytes, all 0xFF, and every stage is read back
from it (the layout: keypoint_shapes_ref.pieces, which test_keypoint_shapes_cpu.py holds to the library's own size), so a wrong
neg, a or hit cannot hide diluted in a sum.  keypoint_shapes_ref.evaluate, the function the CPU module shows to refuse ten
wrong walks, judges the run: counts, fcnt, neg[], hit[] and a[] on the valid cells exact; the outputs and d[], hinge[], the
normalised rows and the pairs' sums within max(8 x the oracle's own float32 error of that case, 16 x 2^-24), the placed cases
within 16 x 2^-24 alone (but dfeat of the tied cases, where one column sums some 225 anchors: 8 x the error of a float32
restatement of the device's own order, keypoint_shapes_ref.device_order32, which gives the device's error to three digits);
dfeat exactly 0 at every pixel no tap touches, dscore exactly 0 on the border ring.  Every call is
made twice: outputs and scratch are bit-identical, guard and padding still hold 0xFF.  Every test prints the share of each
bound it used.
"""
import numpy as np
import pytest
import torch

import keypoint_shapes_ref as ks

kr = ks.kr
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096
KEYS = (("score", "score"), ("coord", "shift"), ("feat", "feat"))


def _dev(a):
    return torch.from_numpy(np.array(a, np.float32)).to(DEV)          # (a copy: the shared inputs are read-only)


def _pieces_of(raw, pieces):
    """The pieces as numpy arrays by name; asserts that the guard and the padding between the pieces still hold 0xFF."""
    at, need = ks.carve_offsets(pieces)
    out, end = {}, 0
    for name, (n, size), lo in zip(ks.PIECE_NAMES, pieces, at):
        assert (raw[end:lo] == 0xFF).all(), f"padding in front of {name} written"
        out[name] = raw[lo:lo + n * size].view(ks.PIECE_DTYPES[name]).copy()
        end = lo + n * size
    assert raw.size == need + GUARD and (raw[end:] == 0xFF).all(), "bytes behind the scratch written"
    return out


def _once(inp, pairs=slice(None)):
    """One call on a fresh scratch -> (the tensors to compare bit for bit, the run as evaluate takes it)."""
    from nano_vs_slam_amd import keypoint_training as kt
    out, aug = ({k: _dev(inp[view][o][pairs]) for k, o in KEYS} for view in ("tgt", "src"))
    B, C, Hf, Wf = out["feat"].shape
    Hc, Wc = out["score"].shape[2:]
    N, n = Hc * Wc, (Hc - 2) * (Wc - 2)
    pieces = ks.pieces(B, Hc, Wc, C)
    need = ks.carve(pieces)
    buf = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    lw, dw, sw, kw = inp["weights"]
    loss, grads, stats = kt.keypoint_loss(out, aug, _dev(inp["hom"][pairs]), (inp["H"], inp["W"]), inp["cell"], loc_weight=lw, descriptor_weight=dw,
                                          score_weight=sw, keypoint_weight=kw, scratch=buf[:need], return_parts=True)
    torch.cuda.synchronize()
    p = _pieces_of(buf.cpu().numpy(), pieces)
    bits = [buf, loss, stats["parts"], stats["valid"], stats["anchors"], stats["hits"]] + [grads[v][k] for v in ("out", "out_aug") for k, _ in KEYS]
    got = {"counts": (int(stats["valid"]), int(stats["anchors"]), int(stats["hits"])), "fcnt": p["fcnt"].reshape(B, 2), "a": p["a"].reshape(B, N),
           "d": p["d"].reshape(B, N), "fsum": p["fsum"].reshape(B, 6)[:, :5], "loss": float(loss), "parts": stats["parts"].cpu().numpy().astype(np.float64)}
    for k in ("neg", "hit", "hinge"):
        got[k] = p[k].reshape(B, n)
    for k in ("r", "t"):
        got[k] = p[k].reshape(B, n, C)
    for view, tag in (("out", "t"), ("out_aug", "s")):
        for k, o in KEYS:
            assert torch.isfinite(grads[view][k]).all()
            got[f"d{o}_{tag}"] = grads[view][k].cpu().numpy().astype(np.float64)
    assert abs(float(stats["recall"]) - got["counts"][2] / (B * n)) <= 1e-6
    return bits, got


def _twice(case):
    inp = ks.inputs(case)
    bits, got = _once(inp)
    again, _ = _once(inp)
    for i, (a, b) in enumerate(zip(bits, again)):
        assert torch.equal(a, b), f"{case}: {'scratch' if i == 0 else 'output ' + str(i)} differs between two calls"
    return got


def _report(case, got):
    fails, ratios = ks.evaluate(case, got)
    print(f"{case}: share of the bounds used " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    worst = max(ratios, key=ratios.get)
    print(f"{case}: largest share of a bound {ratios[worst]:.3f} ({worst})")
    assert not fails, fails


@pytest.mark.parametrize("case", ks.DRAWN)
def test_drawn_cases_stage_by_stage(case):
    _report(case, _twice(case))


@pytest.mark.parametrize("case", ks.PLACED)
def test_placed_ties_stage_by_stage(case):
    o = ks.oracle(case)
    assert ks.check_placed(case, o) is None
    assert all(v == ks.FLOOR for k, v in ks.bounds(case).items() if case == "Ta" or k not in ks.WIDENED)
    got = _twice(case)
    ref = ks.as_got(o)
    assert np.array_equal(got["a"], ref["a"]) and np.array_equal(got["neg"], ref["neg"]) and np.array_equal(got["hit"], ref["hit"].astype(np.int32))
    if case == "Ta":
        assert got["a"][0, 255] == 255
    else:
        k1, k2 = ks.tie_of(case)
        assert got["neg"][0, k2] == k1 and got["neg"][0, k1] == k2 and got["hit"][0, k1] == 1 and got["hit"][0, k2] == 0
        assert np.array_equal(got["t"][0, k1].view(np.uint32), got["t"][0, k2].view(np.uint32))
    _report(case, got)


def test_k1_pair_alone_and_in_its_batch():
    inp = ks.inputs("K1")
    _, both = _once(inp)
    _, alone = _once(inp, slice(0, 1))
    assert alone["neg"].shape == (1, 256) and both["neg"].shape == (2, 256)
    for k in ("neg", "hit", "a"):
        assert np.array_equal(alone[k][0], both[k][0]), k
    assert np.array_equal(alone["r"].view(np.uint32)[0], both["r"].view(np.uint32)[0]) and np.array_equal(alone["d"].view(np.uint32)[0], both["d"].view(np.uint32)[0])
