"""Host-side checks of the dense-head scores: the oracle (tests/dense_ref.py) and the Python reductions on the issue's
worked example, the zero-division cases, the header's depth bound pinned from both sides, and the argument checks of
kp2d_seg_stats / kp2d_depth_sums, which return before anything touches a device.  No GPU involved."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dense_ref as dr
from nano_vs_slam_amd import _lib
from nano_vs_slam_amd import dense_metrics as dm

TARGET = np.array([[0, 0, 1, 1, 255, 2]])
PRED = np.array([[0, 1, 1, 1, 2, 0]])
SCORES = {"iou": dm.iou_score, "accuracy": dm.accuracy, "f1": dm.f1_score}


def columns(stats):
    return [torch.from_numpy(np.ascontiguousarray(stats[..., i])) for i in range(4)]


def test_worked_example():
    stats, conf, ignored, stray = dr.seg_stats(PRED, TARGET, 3, ignore=255)
    assert stats[0].tolist() == [[1, 1, 1, 2], [2, 1, 0, 2], [0, 0, 1, 4]]
    assert conf[0].tolist() == [[1, 1, 0], [0, 2, 0], [1, 0, 0]]
    assert ignored.tolist() == [1] and stray.tolist() == [0]
    want = {("iou", "micro"): 3 / 7, ("accuracy", "micro"): 11 / 15, ("f1", "micro"): 0.6, ("iou", "macro"): 1 / 3}
    for (kind, red), v in want.items():
        assert abs(dr.score(kind, stats, red) - v) <= 1e-15
        assert abs(float(SCORES[kind](*columns(stats), reduction=red)) - v) <= 1e-15
    # one image: the imagewise reductions are the plain ones
    assert dr.score("iou", stats, "micro-imagewise") == dr.score("iou", stats, "micro")
    assert dr.score("iou", stats, "macro-imagewise") == dr.score("iou", stats, "macro")


def test_stray_pixels_count_nowhere_else():
    target = np.array([[0, 1, 5, -1, 255, 1]])
    pred = np.array([[0, 7, 1, 1, 9, 1]])
    stats, conf, ignored, stray = dr.seg_stats(pred, target, 3, ignore=255)
    assert ignored.tolist() == [1] and stray.tolist() == [3]
    assert stats[0].tolist() == [[1, 0, 0, 1], [1, 0, 0, 1], [0, 0, 0, 2]] and conf.sum() == 2
    # without an ignore index the 255 is one more stray value
    _, _, ignored, stray = dr.seg_stats(pred, target, 3, None)
    assert ignored.tolist() == [0] and stray.tolist() == [4]


@pytest.mark.parametrize("reduction", dr.REDUCTIONS)
@pytest.mark.parametrize("kind", sorted(SCORES))
def test_reductions_agree_with_the_oracle(kind, reduction):
    rng = np.random.default_rng(7)
    pred, target = dr.seg_case(3, 9, 11, 5, np.uint8, 7, ("mixed", "ignored", "single"))
    stats = dr.seg_stats(pred.reshape(3, -1), target.reshape(3, -1), 5, 255)[0]
    stats[:, 4] = 0                                  # a class absent from both maps ...
    stats[:, 4, 3] = stats[:, 0].sum(1)              # ... is all true negatives
    assert stats[1].sum() == 0                       # the wholly ignored image has no counted pixel
    for zd in (1.0, 0.0, float(rng.random())):
        got = SCORES[kind](*columns(stats), reduction=reduction, zero_division=zd)
        want = dr.score(kind, stats, reduction, zd)
        assert got.dtype == torch.float64
        assert np.abs(got.numpy() - want).max() <= 1e-15
    if reduction is None:
        got = SCORES[kind](*columns(stats), zero_division=0.25).numpy()
        assert np.all(got[1] == 0.25)                                     # 0/0 everywhere in the ignored image
        assert np.all(got[[0, 2], 4] == (1.0 if kind == "accuracy" else 0.25))  # absent class: only accuracy has a denominator


def test_unbuilt_options_raise():
    st = columns(dr.seg_stats(PRED, TARGET, 3, 255)[0])
    for red in ("weighted", "weighted-imagewise", "none"):
        with pytest.raises(ValueError, match="not built"):
            dm.iou_score(*st, reduction=red)
    with pytest.raises(ValueError, match="not built"):
        dm.f1_score(*st, reduction="micro", zero_division="warn")
    with pytest.raises(ValueError, match="not built"):
        dm.get_stats(torch.zeros(1, 2, 2, dtype=torch.int64), torch.zeros(1, 2, 2, dtype=torch.int64), mode="multilabel",
                     num_classes=3)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        dm.get_stats(torch.zeros(1, 2, 2, dtype=torch.int64), torch.zeros(1, 2, 2, dtype=torch.int64), num_classes=3)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        dm.depth_sums(torch.ones(1, 2, 2), torch.ones(1, 2, 2))
    with pytest.raises(ValueError, match="num_classes"):
        dm.get_stats(torch.zeros(1, 2, 2, dtype=torch.int64), torch.zeros(1, 2, 2, dtype=torch.int64), num_classes=1025)


def test_metrics_from_sums_on_cpu_numbers():
    gt, pred, valid = dr.depth_case(*dr.DEPTH_SHAPES[0])
    rows = dr.depth_sums(gt, pred, valid, *dr.DEPTH_LIMITS)
    assert np.all(rows[:, 0] + rows[:, 10] == gt[0].size) and np.all(rows[:, 10] > 8)
    tot = np.array([math.fsum(rows[:, s]) for s in range(dr.NSUMS)])
    got = dict(zip(dm.DEPTH_KEYS, dm.metrics_from_sums(torch.from_numpy(tot)).tolist()))
    want = dr.depth_metrics(tot)
    assert dm.DEPTH_KEYS == dr.DEPTH_KEYS
    for k in dr.DEPTH_KEYS:
        assert abs(got[k] - want[k]) <= 1e-14 * abs(want[k]), k
    # the straight float64 formulas of the reference on the valid pixels give the same nine numbers
    ok = dr.depth_valid(gt, pred, valid, *dr.DEPTH_LIMITS)
    g, p = gt[ok].astype(np.float64), pred[ok].astype(np.float64)
    err = np.log(p) - np.log(g)
    direct = {"a1": (np.maximum(g / p, p / g) < 1.25).mean(), "abs_rel": np.mean(np.abs(g - p) / g),
              "rmse": np.sqrt(((g - p) ** 2).mean()), "silog": np.sqrt(np.mean(err ** 2) - np.mean(err) ** 2) * 100,
              "log_10": np.abs(np.log10(g) - np.log10(p)).mean()}
    for k, v in direct.items():
        assert abs(want[k] - v) <= 1e-12 * abs(v), k
    # with sigma = 0.3 the difference inside silog cancels less than two digits
    m2, m1 = tot[7] / tot[0], tot[8] / tot[0]
    assert m2 / (m2 - m1 * m1) < 100
    # no valid pixel: count 0, every metric NaN
    empty = dm.metrics_from_sums(torch.zeros(dr.NSUMS, dtype=torch.float64))
    assert bool(torch.isnan(empty).all()) and all(math.isnan(v) for v in dr.depth_metrics(np.zeros(dr.NSUMS)).values())


@pytest.mark.parametrize("shape", dr.DEPTH_SHAPES)
def test_depth_bound_is_pinned_from_both_sides(shape):
    gt, pred, valid = dr.depth_case(*shape)
    n = gt[0].size
    D = dr.depth_depth(n)
    assert D == 33 + math.ceil(math.ceil(n / 4096) / 256) == 34
    for b in range(shape[0]):
        ok = dr.depth_valid(gt[b], pred[b], valid[b], *dr.DEPTH_LIMITS)
        g, p = gt[b][ok], pred[b][ok]
        terms, bound = dr.depth_terms(g, p), dr.depth_bounds(g, p, n)
        for s in dr.FLOAT_SLOTS:
            t = terms[s]
            exact, mass = math.fsum(t), math.fsum(np.abs(t))
            chain = 0.0                                       # one chain of n additions: NOT the bound's premise, which
            for v in t[::-1].tolist():                        # is D(n) additions per term; it keeps its own (n - 1) u
                chain += v
            assert abs(chain - exact) <= (len(t) - 1) * dr.U * mass
            rev = float(np.sum(t[::-1]))                      # reversed, numpy's pairwise float64 sum
            shaped = [dr.emulate_sum(t), dr.emulate_sum(t[::-1])]     # the device's own shape, both ways round
            chunked = 0.0
            for i in range(0, len(t), 1000):
                chunked += float(np.sum(t[i:i + 1000]))
            f32 = math.fsum(dr.depth_terms_f32(g, p, s))
            worst = int(np.argmax(np.abs(t)))                 # ONE pixel's term in float32, the rest in float64
            one = exact - t[worst] + dr.depth_terms_f32(g[worst:worst + 1], p[worst:worst + 1], s)[0]
            print(f"{shape} image {b} slot {s}: bound {bound[s]:.3e} = 2^{math.log2(bound[s] / mass):.1f} sum|t|; reversed "
                  f"{abs(rev - exact):.2e} (as one chain {abs(chain - exact):.2e}), device order "
                  f"{abs(shaped[0] - exact):.2e} / {abs(shaped[1] - exact):.2e}, chunks of 1000 {abs(chunked - exact):.2e}, float32 terms {abs(f32 - exact):.2e}, "
                  f"one float32 term {abs(one - exact):.2e}")
            assert abs(rev - exact) <= bound[s] and abs(chunked - exact) <= bound[s]
            assert max(abs(v - exact) for v in shaped) <= D * dr.U * mass <= bound[s]
            assert abs(f32 - exact) > bound[s]
            assert abs(one - exact) > bound[s]
            assert bound[s] < 2.0 ** -40 * mass


def _fake(addr=4096):
    return C.c_void_p(addr)          # never dereferenced: every case below is refused by the argument checks


def test_entry_points_check_arguments_without_a_device():
    lib = _lib.load()
    ok = dict(pred=_fake(), target=_fake(), dtype=2, B=2, n=100, C=19, ignore=255, stats=_fake(), conf=None, ignored=_fake(),
              stray=_fake())

    def seg(**kw):
        a = dict(ok, **kw)
        return lib.kp2d_seg_stats(a["pred"], a["target"], a["dtype"], a["B"], a["n"], a["C"], a["ignore"], a["stats"], a["conf"],
                                  a["ignored"], a["stray"], None)

    def refused(rc, code, text):
        assert rc == code, (rc, lib.kp2d_last_error())
        assert text.encode() in lib.kp2d_last_error(), lib.kp2d_last_error()
        with pytest.raises(_lib.Kp2dError):
            _lib.check(rc)

    ARG, UNSUPPORTED = -1, -2
    refused(seg(C=0), ARG, "num_classes")
    refused(seg(C=1025), ARG, "num_classes")
    refused(seg(C=257, conf=_fake()), UNSUPPORTED, "confusion")
    refused(seg(n=0), ARG, "n = 0")
    refused(seg(n=-5), ARG, "n = -5")
    refused(seg(B=0), ARG, "B = 0")
    refused(seg(dtype=3), ARG, "target_dtype")
    refused(seg(dtype=-1), ARG, "target_dtype")
    for name in ("pred", "target", "stats", "ignored", "stray"):
        refused(seg(**{name: None}), ARG, "null")
    refused(seg(stats=_fake(4100)), ARG, "misaligned")
    assert lib.kp2d_seg_conf_lds_max() == dm.seg_conf_lds_max() and 1 <= dm.seg_conf_lds_max() < dm.SEG_CONF_MAX_CLASSES

    need = lib.kp2d_depth_scratch_bytes(2, 10000)
    assert need == 2 * 3 * dr.NSUMS * 8 and dm.DEPTH_NSUMS == dr.NSUMS == len(dm.DEPTH_SUMS)
    assert lib.kp2d_depth_scratch_bytes(0, 100) == 0 and lib.kp2d_depth_scratch_bytes(2, 0) == 0
    dok = dict(gt=_fake(), pred=_fake(), valid=None, B=2, n=10000, sums=_fake(), scratch=_fake(), nbytes=need)

    def depth(**kw):
        a = dict(dok, **kw)
        return lib.kp2d_depth_sums(a["gt"], a["pred"], a["valid"], a["B"], a["n"], float("nan"), float("nan"), a["sums"],
                                   a["scratch"], a["nbytes"], None)

    refused(depth(n=0), ARG, "n = 0")
    refused(depth(B=-1), ARG, "B = -1")
    for name in ("gt", "pred", "sums", "scratch"):
        refused(depth(**{name: None}), ARG, "null")
    refused(depth(nbytes=need - 1), ARG, "scratch")
    refused(depth(nbytes=0), ARG, "scratch")
