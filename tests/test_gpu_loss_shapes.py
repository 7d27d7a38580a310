"""The two dense losses on the device (nano_vs_slam_amd.seg_training.segmentation_loss, csrc/seg_train.hip;
nano_vs_slam_amd.depth_training.depth_loss, csrc/depth_train.hip) at the shapes of loss_shapes_ref: two and three 1024-pixel
chunks per group with a short, ragged last group and frame boundaries inside a chunk (P2: 1 051 250 pixels, P3: 2 101 707), and
on the small P1 the class counts 86, 100 and 128 at which sl_merge_kernel and sl_grad_kernel take their second pass.

Every call gets its own scratch, filled with 0xFF, and the groups' partial sums are read back from it, so each group is
checked on its own (loss_shapes_ref.evaluate_seg / evaluate_depth, the functions test_loss_shapes_cpu.py shows to refuse
every wrong walk but one):

1. Exact: on one-hot and uniform logits every class sum of every group is a float32 number in any order (check_exact asserts
   the condition again here), so the device's partials equal the float64 ones bit for bit; counts are exact everywhere.
2. Float-valued: loss, dlogits and each group's sums within max(8 x the error of the float32 restatement of the device's own
   order, 16 x 2^-24), formed from the restatement alone; dlogits exactly 0 at every pixel without a valid label or ground
   truth.  Every test prints the share of its bounds it used.
3. Every call is made twice: outputs and scratch are bit-identical, and neither the bytes behind the scratch's stated size
   nor the padding between its pieces are written.
"""
import numpy as np
import pytest
import torch

import loss_shapes_ref as ls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096
UNSUPPORTED = -2
SEG_DTYPES = (np.int64, np.float32, np.float32)
DEPTH_DTYPES = (np.int64, np.float64, np.float64)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared inputs are read-only)


def _fresh(pieces):
    """A scratch of exactly the stated size in front of GUARD more bytes, all 0xFF -> (the whole buffer, the scratch)."""
    need = ls.carve(pieces)
    buf = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    return buf, buf[:need]


def _pieces_of(buf, pieces, dtypes):
    """The pieces as numpy arrays; asserts that the guard and the padding between the pieces still hold 0xFF."""
    raw = buf.cpu().numpy()
    at, need = ls.carve_offsets(pieces)
    out, end = [], 0
    for (n, size), lo, dt in zip(pieces, at, dtypes):
        assert np.dtype(dt).itemsize == size and (raw[end:lo] == 0xFF).all(), "padding written"
        out.append(raw[lo:lo + n * size].view(dt).copy())
        end = lo + n * size
    assert raw.size == need + GUARD and (raw[end:] == 0xFF).all(), "bytes behind the scratch written"
    return out


def _seg_once(z, labels, nc):
    from nano_vs_slam_amd import seg_training as st
    N, _, H, W = z.shape
    pieces = ls.seg_pieces(N, H * W, nc)
    buf, scratch = _fresh(pieces)
    loss, dz, valid, stray = st.segmentation_loss(z, labels, *ls.SEG_WEIGHTS, ignore_index=ls.IGNORE, scratch=scratch)
    torch.cuda.synchronize()
    cnt, part, coef = _pieces_of(buf, pieces, SEG_DTYPES)
    return dict(loss=loss, dz=dz, valid=valid, stray=stray, cnt=cnt.reshape(-1, 2), part=part.reshape(-1, 1 + 3 * nc), coef=coef)


def _depth_once(z, gt):
    from nano_vs_slam_amd import depth_training as dt
    N, H, W = z.shape
    pieces = ls.depth_pieces(N, H * W)
    buf, scratch = _fresh(pieces)
    loss, dz, valid, stray, parts = dt.depth_loss(z, gt, *ls.DEPTH_WEIGHTS, scratch=scratch, return_parts=True)
    torch.cuda.synchronize()
    cnt, part, coef = _pieces_of(buf, pieces, DEPTH_DTYPES)
    return dict(loss=loss, dz=dz, valid=valid, stray=stray, silog=parts[0], huber=parts[1], cnt=cnt.reshape(-1, 2), part=part.reshape(-1, 3), coef=coef)


def _same_bits(what, a, b, but=()):
    for k in a:
        if k in but:
            continue
        same = torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))
        assert same, f"{what}: {k} differs"


def _host(r):
    """What evaluate_* takes: scalars as Python numbers, dlogits as a float64 array."""
    out = {k: v for k, v in r.items() if k in ("cnt", "part")}
    out.update({k: float(r[k]) for k in ("loss", "silog", "huber") if k in r})
    out.update(valid=int(r["valid"]), stray=int(r["stray"]), dz=r["dz"].cpu().numpy().astype(np.float64))
    return out


def _twice(what, once, *args):
    r = once(*args)
    _same_bits(f"{what} twice", r, once(*args))
    return r


def _report(case, fails, ratios):
    print(f"{ls.case_id(case)}: share of the bounds used " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert not fails, fails


# ---- segmentation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ls.SEG_EXACT, ids=ls.case_id)
def test_seg_groups_are_exact(case):
    used = ls.check_exact(case)
    print(f"{ls.case_id(case)}: share of 2^24 used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    z, labels = ls.seg_inputs(case)
    r = _twice("segmentation_loss", _seg_once, _dev(z), _dev(labels), case[2])
    ref = ls.seg_reference(case)
    cols = ls.exact_columns(case)
    assert torch.equal(torch.from_numpy(r["part"][:, cols]), torch.from_numpy(ref["part"].astype(np.float32)[:, cols]))
    assert np.array_equal(r["cnt"], ref["cnt"]) and int(r["valid"]) == ref["valid"] and int(r["stray"]) == ref["stray"]
    _report(case, *ls.evaluate_seg(case, _host(r)))


@pytest.mark.parametrize("case", ls.SEG_FLOAT, ids=ls.case_id)
def test_seg_groups_within_the_float32_bound(case):
    nc = case[2]
    z, labels = ls.seg_inputs(case)
    r = _twice("segmentation_loss", _seg_once, _dev(z), _dev(labels), nc)
    _report(case, *ls.evaluate_seg(case, _host(r)))
    if nc == ls.MAX_CLASSES:          # the coefficient table's 257th entry, which sl_grad_kernel's second pass alone loads
        want = np.float32(ls.SEG_WEIGHTS[0]) / np.float32(int(r["valid"]))
        assert r["coef"].size == 2 * nc + 1 == 257 and abs(float(r["coef"][2 * nc]) - float(want)) <= 2 * float(np.spacing(want))
        assert bool(r["dz"].any())


def test_seg_label_types_give_the_same_bits():
    case = ("float", "P2", 19)
    assert case in ls.SEG_FLOAT
    z, labels = ls.seg_inputs(case)
    zd = _dev(z)
    base = _seg_once(zd, _dev(labels), case[2])
    for dt in (np.int32, np.int64):
        _same_bits(f"labels as {np.dtype(dt).name}", base, _seg_once(zd, _dev(labels.astype(dt)), case[2]))
    # negative labels, which only int64 and int32 can hold, over ignored pixels: strays, and nothing else moves
    neg, extra = ls.negative_labels(case)
    r = _seg_once(zd, _dev(neg), case[2])
    _same_bits("negative labels", base, r, but=("cnt", "stray"))
    assert np.array_equal(r["cnt"][:, 0], base["cnt"][:, 0]) and np.array_equal(r["cnt"][:, 1], base["cnt"][:, 1] + extra)
    assert int(r["stray"]) == ls.seg_reference(case)["stray"] + len(ls.NEGATIVES)


def test_more_than_128_classes_are_refused():
    from nano_vs_slam_amd import _lib, seg_training as st
    from nano_vs_slam_amd._dev import ptr, stream
    lib = _lib.load()
    N, H, W = ls.SHAPES["P1"]
    nc = ls.MAX_CLASSES + 1
    assert int(lib.kp2d_seg_loss_scratch_bytes(N, H * W, nc)) == 0
    z = torch.zeros((N, nc, H, W), dtype=torch.float32, device=DEV)
    labels = torch.zeros((N, H, W), dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), 7.0, dtype=torch.float32, device=DEV)
    dz = torch.full_like(z, 7.0)
    counts = torch.full((2,), 7, dtype=torch.int64, device=DEV)
    scratch = torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device=DEV)
    rc = lib.kp2d_seg_loss(ptr(z), ptr(labels), 0, N, H * W, nc, ls.IGNORE, 0.5, 1.5, ptr(loss), ptr(dz), ptr(counts[0:1]), ptr(counts[1:2]),
                           ptr(scratch), scratch.numel(), stream(z.device))
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED and b"C above 128" in lib.kp2d_last_error(), (rc, lib.kp2d_last_error())
    assert float(loss) == 7.0 and bool((dz == 7.0).all()) and bool((counts == 7).all()) and bool((scratch == 0xFF).all())
    with pytest.raises(ValueError):
        st.segmentation_loss(z, labels)


# ---- depth -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ls.DEPTH_CASES, ids=ls.case_id)
def test_depth_runs_within_the_float32_bound(case):
    z, gt = ls.depth_inputs(case)
    r = _twice("depth_loss", _depth_once, _dev(z), _dev(gt))
    assert r["part"].dtype == np.float64 and r["coef"].size == 4
    _report(case, *ls.evaluate_depth(case, _host(r)))
