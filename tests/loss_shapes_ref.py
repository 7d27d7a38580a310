"""Cases and float64 references of the two dense losses (nano_vs_slam_amd.seg_training.segmentation_loss, csrc/seg_train.hip;
nano_vs_slam_amd.depth_training.depth_loss, csrc/depth_train.hip) past one 1024-pixel chunk per workgroup, and at the class
counts where the merge and gradient kernels of the segmentation loss take a second pass.  test_loss_shapes_cpu.py holds
everything here to itself without a device, test_gpu_loss_shapes.py holds the kernels to it.

* The geometry: geo_of restates loss_geo / depth_geo (chunks of LP = 1024 pixels, at most 1024 groups of cpg = ceil(chunks /
  1024) consecutive chunks; depth_train.hip calls a group a run), GEOMETRY the figures the three shapes were chosen for:

      shape  N, H, W       pixels     chunks  cpg  groups  last group          what it is for
      P1     1, 33, 37     1 221      2       1    2       1 chunk of 197 px   small: the class counts 86, 100 and 128
      P2     2, 725, 725   1 051 250  1027    2    514     1 chunk of 626 px   the frame boundary (pixel 525 625) lies in chunk
                                                                               513, the second chunk of group 256
      P3     3, 837, 837   2 101 707  2053    3    685     1 chunk of 459 px   both frame boundaries lie inside a chunk

  seg_pieces / depth_pieces restate the scratch walks of loss_plan and depth_plan, carve the rule they are cut by; the tests
  pass their own scratch and read every group's partial sums back, so a wrong cut between chunks cannot cancel in a total.
* placed(shape) puts, on P2 and P3, into the labels or the ground truth: group 0 wholly ignored; one group wholly ignored
  (the merge's nb == 0 branch); one group whose chunk 1 is wholly ignored (on P3 its middle chunk: cn = 0 inside a run that
  has a state); one group whose first chunk is wholly ignored; the ragged last group with exactly one valid pixel.
* Segmentation, exact cases (SEG_EXACT): "onehot" logits are 0 at a drawn class and -200 elsewhere, so in float32 s = 1 and
  p is 0 or 1 and the CE term is 0 or 200; "uniform" logits are all 0 with C = 4, so p = 1/4.  Every class sum of every group
  and of the batch is then a float32 number in any order (check_exact asserts the condition), and the device must give the
  float64 per-group partials bit for bit.  The uniform case's CE column (logf(4) per pixel) is float-valued.
* Segmentation, float cases (SEG_FLOAT): labels drawn as seg_training_ref.make_inputs draws them (the last class absent,
  one label in ten ignored, a dozen stray), logits normal with a spread of 2 (make_inputs draws no logits: its come out of the
  head).  Depth (DEPTH_CASES): drawn as depth_training_ref.make_loss_inputs draws them, a dozen stray pixels (NaN, +-inf in
  either array); "offset" is the recipe of its case L4 (logits near -20, gt near 0.9: mean^2 / variance about 2e9).
* References: loss, gradient, valid and stray are seg_training_ref.seg_loss / depth_training_ref.depth_loss, imported.  The
  per-group partials are formed straight from each group's pixels (depth: the two-pass mean and M2, not Chan's recurrence).
* Bounds: seg_eval32 restates the device's float32 summation order (a thread's four pixels per chunk in order, the 64-lane
  butterfly, the waves as (0 + 1) + (2 + 3), chunk after chunk, the groups in order); depth_eval32 forms the per-pixel terms in
  float32 and sums in float64 as the device does.  A bound is max(8 x that evaluation's error against float64, 16 x 2^-24):
  seg_bounds() takes the maximum over SEG_FLOAT and the uniform case, depth_bounds(case) is per case because "offset" is
  ill-conditioned on purpose.  Error measures: loss and parts |v - v64| / |v64|; dlogits max|G - G64| / max|G64|; a group's
  partial sum |v - v64| / (the sum of its terms' magnitudes), and exactly 0 where the group has no term; a run's mean against
  the mean magnitude of its g, its M2 against M2 (exactly 0 below two pixels).
* emulate_groups(case, mut) walks the geometry group by group and chunk by chunk in float64, as the kernels index their
  arrays; with mut=None it equals the direct references; MUTANTS are the ways the walk could be wrong.  int32_pixel (the pixel
  index wrapped at 2^31) changes nothing below 2^31 pixels and is NOT detected by these cases: a case that large is no test
  of a few seconds.  frame_of_chunk does not apply to depth (one channel: a pixel's address is its index).  raw_moments forms
  the run's M2 as sum g^2 - (sum g)^2 / n from float32 sums, the precision of the terms themselves: with float64 moments the
  shortcut costs 1.9e-5 of a run's M2 at offset's mean^2 / variance, which hides below the 2.2e-4 the float32 terms cost
  themselves, so only the float32 form of the shortcut is one these tests can promise to catch (it misses by a factor 690).

Out of scope: dl_grad_kernel's grid-stride form begins above 2^28 pixels (1 GiB per array on the device, a multi-GB float64
reference on the host: no test of a few seconds); the whole training steps at these sizes (the layer ops have their own
shape tests, train_ops_shapes_ref).

Measured.  Bounds (test_loss_shapes_cpu.py prints them; every quantity not listed sits on the floor 16 x 2^-24 = 9.54e-07):
segmentation loss 1.61e-06 (8 x 2.0e-07, float-P3-4), dlogits 8.32e-06 (8 x 1.04e-06, float-P2-19), a group's CE sum 1.13e-06,
I 5.01e-06 (8 x 6.3e-07, float-P1-86), sum p 1.51e-06; depth dlogits 1.69e-06 (depth-P2), 1.29e-06 (depth-P3), 2.61e-06
(offset-P2), and offset-P2's M2 of a run 1.76e-03 (8 x 2.2e-04: deviations of 4e-4 in float32 terms near -19.9).  The
device's error as a share of its bound, first run on the MI355X (no share is above 0.5; the exact cases' partials are equal):

    case           loss   dlogits  part_ce  part_I  part_P     case       loss   silog  huber  dlogits  run_mean  run_M2  run_huber
    onehot-P2-19   0.011  0.004    =        =       =          depth-P2   0.004  0.005  0.035  0.109    0.021     0.027   0.056
    onehot-P3-4    0.002  0.006    =        =       =          depth-P3   0.003  0.002  0.033  0.131    0.042     0.027   0.051
    uniform-P3-4   0.013  0.007    0.067    =       =          offset-P2  0.010  0.038  0.017  0.125    0.015     0.127   0.006
    float-P2-19    0.101  0.125    0.125    0.035   0.122
    float-P3-4     0.125  0.073    0.101    0.025   0.072
    float-P1-86    0.017  0.030    0.011    0.107   0.083
    float-P1-100   0.035  0.048    0.032    0.077   0.098
    float-P1-128   0.009  0.037    0.065    0.124   0.126
"""
import functools

import numpy as np

import depth_training_ref as dr
import seg_training_ref as sr

rel_err, FLOOR, IGNORE = sr.rel_err, sr.FLOOR, sr.IGNORE
assert dr.FLOOR == sr.FLOOR and dr.rel_err is sr.rel_err

# ---- geometry (csrc/seg_train.hip, csrc/depth_train.hip, csrc/api_common.h) ------------------------------------------------
LP = 1024                 # pixels of a chunk: four per thread of 256
MAX_GROUPS = 1024
MAX_CLASSES = 128
ALIGN = 256               # a scratch piece starts, and the total ends, on a multiple of this

SHAPES = {"P1": (1, 33, 37), "P2": (2, 725, 725), "P3": (3, 837, 837)}      # N, H, W
# what each shape was chosen for; last: chunks of the last group, ragged: pixels of the last chunk
GEOMETRY = {"P1": dict(total=1221, chunks=2, cpg=1, groups=2, last=1, ragged=197),
            "P2": dict(total=1051250, chunks=1027, cpg=2, groups=514, last=1, ragged=626),
            "P3": dict(total=2101707, chunks=2053, cpg=3, groups=685, last=1, ragged=459)}


def geo_of(N, HW):
    total = N * HW
    chunks = -(-total // LP)
    cpg = -(-chunks // MAX_GROUPS)
    groups = -(-chunks // cpg)
    return dict(total=total, chunks=chunks, cpg=cpg, groups=groups, last=chunks - (groups - 1) * cpg, ragged=total - (chunks - 1) * LP)


def shape_geo(shape):
    N, H, W = SHAPES[shape]
    return geo_of(N, H * W)


def boundary_chunks(shape):
    """[(group, chunk of the group, pixel of the chunk)] of every frame boundary that lies inside a chunk."""
    N, H, W = SHAPES[shape]
    g = shape_geo(shape)
    return [(n * H * W // LP // g["cpg"], n * H * W // LP % g["cpg"], n * H * W % LP) for n in range(1, N) if n * H * W % LP]


def carve_offsets(pieces):
    """Carve's walk over (count, itemsize) pieces -> (each piece's byte offset, the total): a piece starts at the next multiple
    of ALIGN, and so does the end."""
    end, at = 0, []
    for n, itemsize in pieces:
        at.append(-(-end // ALIGN) * ALIGN)
        end = at[-1] + n * itemsize
    return at, -(-end // ALIGN) * ALIGN


def carve(pieces):
    return carve_offsets(pieces)[1]


def seg_pieces(N, HW, C):
    """loss_plan's: cnt int64 [groups][2], part float32 [groups][1 + 3 C], coef float32 [2 C + 1]."""
    G = geo_of(N, HW)["groups"]
    return [(G * 2, 8), (G * (1 + 3 * C), 4), (2 * C + 1, 4)]


def depth_pieces(N, HW):
    """depth_plan's: cnt int64 [runs][2], part float64 [runs][3], coef float64 [4]."""
    G = geo_of(N, HW)["groups"]
    return [(G * 2, 8), (G * 3, 8), (4, 8)]


def placed(shape):
    """The placed patterns of a shape with more than one chunk per group -> dict: the groups (whole, second, first, last),
    off: the pixel ranges that hold no valid pixel, keep: the last group's only valid pixel.  None of the groups holds a
    frame boundary."""
    g = shape_geo(shape)
    G, cpg = g["groups"], g["cpg"]
    if cpg == 1:
        return None
    span = cpg * LP
    whole, second, first, last = G // 4, G // 2 + 1, 3 * G // 4, G - 1
    off = [(0, span), (whole * span, (whole + 1) * span), (second * span + LP, second * span + 2 * LP), (first * span, first * span + LP),
           (last * span, g["total"])]
    return dict(whole=whole, second=second, first=first, last=last, off=off, keep=last * span + g["ragged"] // 2)


def off_mask(shape):
    """bool [pixels]: the pixels placed() leaves without a valid label or ground truth."""
    m = np.zeros(shape_geo(shape)["total"], bool)
    pl = placed(shape)
    if pl:
        for lo, hi in pl["off"]:
            m[lo:hi] = True
        m[pl["keep"]] = False
    return m


# ---- the cases ---------------------------------------------------------------------------------------------------------------
SEG_EXACT = (("onehot", "P2", 19), ("onehot", "P3", 4), ("uniform", "P3", 4))
SEG_FLOAT = (("float", "P2", 19), ("float", "P3", 4), ("float", "P1", 86), ("float", "P1", 100), ("float", "P1", 128))
SEG_CASES = SEG_EXACT + SEG_FLOAT
SEG_BOUND_CASES = SEG_FLOAT + (("uniform", "P3", 4),)
DEPTH_CASES = (("depth", "P2"), ("depth", "P3"), ("offset", "P2"))
SEG_WEIGHTS, DEPTH_WEIGHTS = (0.5, 1.5), dr.WEIGHTS
STRAYS = 12
NEGATIVES = (-1, -2, -128, -255, -256, -2 ** 31, -2 ** 31 - 1, -2 ** 40, -2 ** 63)      # int64 labels only
MUTANTS = ("skip_last_chunk", "floor_groups", "frame_of_chunk", "no_reset", "int32_pixel", "raw_moments")
UNDETECTED = ("int32_pixel",)


def case_id(case):
    return "-".join(str(v) for v in case)


def _seed(case):
    return 9100 + (SEG_CASES + DEPTH_CASES).index(case)


def pixel_major(a, C):
    """[N, C, H, W] -> [N H W, C]"""
    a = np.asarray(a)
    N = a.shape[0]
    return a.reshape(N, C, -1).transpose(0, 2, 1).reshape(-1, C)


def frame_major(a, N, H, W):
    """[N H W, C] -> [N, C, H, W]"""
    C = a.shape[1]
    return np.ascontiguousarray(a.reshape(N, H * W, C).transpose(0, 2, 1)).reshape(N, C, H, W)


@functools.lru_cache(maxsize=None)
def seg_inputs(case):
    """-> (logits [N, C, H, W] float32, labels [N, H, W] uint8), computed once and shared: nobody writes to them."""
    kind, shape, C = case
    N, H, W = SHAPES[shape]
    total = N * H * W
    rng = np.random.default_rng(_seed(case))
    labels = rng.integers(0, C - 1, total).astype(np.uint8)           # class C - 1 is absent from every label
    if kind == "onehot":
        pred = np.where(rng.random(total) < 0.9, labels, rng.integers(0, C, total))
        z = np.full((total, C), -200.0, np.float32)
        z[np.arange(total), pred] = 0.0
    elif kind == "uniform":
        z = np.zeros((total, C), np.float32)
    else:
        z = 2.0 * rng.standard_normal((total, C), dtype=np.float32)
    labels[rng.random(total) < 0.1] = IGNORE
    labels[rng.choice(total, STRAYS, replace=False)] = rng.integers(C, IGNORE, STRAYS)
    labels[off_mask(shape)] = IGNORE
    pl = placed(shape)
    if pl:
        labels[pl["keep"]] = pl["keep"] % (C - 1)
    z, labels = frame_major(z, N, H, W), labels.reshape(N, H, W)
    z.setflags(write=False)
    labels.setflags(write=False)
    return z, labels


def negative_labels(case):
    """int64 labels with NEGATIVES written over ignored pixels (one of them in group 0), so the valid pixels and every sum
    stay what they were -> (labels, the extra strays per group)."""
    _, labels = seg_inputs(case)
    g = shape_geo(case[1])
    lab = labels.astype(np.int64).reshape(-1)
    at = np.flatnonzero(lab == IGNORE)
    at = at[np.linspace(0, at.size - 1, len(NEGATIVES)).astype(np.int64)]
    assert np.unique(at).size == len(NEGATIVES)
    lab[at] = NEGATIVES
    return lab.reshape(labels.shape), np.bincount(at // (g["cpg"] * LP), minlength=g["groups"])


@functools.lru_cache(maxsize=None)
def depth_inputs(case):
    """-> (logits [N, H, W], gt [N, H, W]) float32, computed once and shared."""
    kind, shape = case
    N, H, W = SHAPES[shape]
    total = N * H * W
    rng = np.random.default_rng(_seed(case))
    if kind == "offset":
        z = (-20.0 + 1e-3 * (rng.random(total) - 0.5)).astype(np.float32)
        gt = (0.9 * (1.0 + 1e-3 * (rng.random(total) - 0.5))).astype(np.float32)
        gt[rng.random(total) < 0.2] = 0.0
    else:
        z = np.clip(2.5 * rng.standard_normal(total), -7.5, 7.5).astype(np.float32)
        gt = dr._draw_gt(rng, (total,))
    off = off_mask(shape)
    gt[off] = np.where(rng.random(int(off.sum())) < 0.5, 0.0, -2.0)
    pl = placed(shape)
    if gt[pl["keep"]] <= 0:
        gt[pl["keep"]] = 1.75
    if kind != "offset":
        at = rng.choice(total, STRAYS, replace=False)
        at = at[at != pl["keep"]]
        bad = np.array([np.nan, np.inf, -np.inf], np.float32)
        gt[at[:6]] = bad[np.arange(6) % 3]
        z[at[6:]] = bad[np.arange(at.size - 6) % 3]
    z, gt = z.reshape(N, H, W), gt.reshape(N, H, W)
    z.setflags(write=False)
    gt.setflags(write=False)
    return z, gt


# ---- float64 references --------------------------------------------------------------------------------------------------
def _classes(labels, C):
    """class_of: a label as a class of [0, C), -1 ignored, -2 stray."""
    v = np.asarray(labels).astype(np.int64).reshape(-1)
    return np.where(v == IGNORE, -1, np.where((v < 0) | (v >= C), -2, v))


def _group_of_pixel(g):
    return np.arange(g["total"]) // (g["cpg"] * LP)


def _part_layout(ce, I, P, T):
    """[groups][1 + 3 C]: the CE sum, then per class I, sum p, sum t."""
    G, C = I.shape
    part = np.empty((G, 1 + 3 * C), ce.dtype)
    part[:, 0] = ce
    part[:, 1::3], part[:, 2::3], part[:, 3::3] = I, P, T
    return part


@functools.lru_cache(maxsize=None)
def seg_reference(case):
    """-> dict: loss, dz [N, C, H, W], valid, stray (seg_training_ref.seg_loss), and per group cnt [G, 2] and part
    [G, 1 + 3 C] in float64, each group's sums formed from its own pixels."""
    _, shape, C = case
    z, labels = seg_inputs(case)
    g = shape_geo(shape)
    G = g["groups"]
    ls = sr.seg_loss(z, labels, SEG_WEIGHTS)
    lab = _classes(labels, C)
    ok = lab >= 0
    zp = pixel_major(z, C).astype(np.float64)
    m = zp.max(axis=1)
    e = np.exp(zp - m[:, None])
    s = e.sum(axis=1)
    p = e / s[:, None] * ok[:, None]
    at = np.where(ok, lab, 0)
    rows = np.arange(g["total"])
    gid = _group_of_pixel(g)
    ce = np.bincount(gid, weights=np.where(ok, (m - zp[rows, at]) + np.log(s), 0.0), minlength=G)
    cell = (gid * C + at)[ok]
    I = np.bincount(cell, weights=p[rows, at][ok], minlength=G * C).reshape(G, C)
    T = np.bincount(cell, minlength=G * C).reshape(G, C).astype(np.float64)
    P = np.add.reduceat(p, np.arange(G) * g["cpg"] * LP, axis=0)
    cnt = np.stack([np.bincount(gid, weights=ok, minlength=G), np.bincount(gid, weights=lab == -2, minlength=G)], axis=1).astype(np.int64)
    assert int(cnt[:, 0].sum()) == ls["valid"] and int(cnt[:, 1].sum()) == ls["stray"]
    return dict(loss=ls["loss"], dz=ls["dz"], valid=ls["valid"], stray=ls["stray"], present=ls["present"], cnt=cnt,
                part=_part_layout(ce, I, P, T))


def _huber(d):
    ad = np.abs(d)
    return np.where(ad < dr.HUBER_DELTA, 0.5 * d * d, dr.HUBER_DELTA * (ad - 0.5 * dr.HUBER_DELTA))


def _run_stats(g, hub, ok, stray, geo):
    """Per run from its own pixels, two passes in float64 -> cnt [G, 2], part [G, 3] (mean, M2, the Huber sum), and the mean
    magnitude of g per run."""
    G = geo["groups"]
    rid = _group_of_pixel(geo)
    n = np.bincount(rid, weights=ok, minlength=G)
    nz = np.maximum(n, 1)
    g = np.where(ok, np.asarray(g, np.float64), 0.0)
    mean = np.bincount(rid, weights=g, minlength=G) / nz
    m2 = np.bincount(rid, weights=np.where(ok, (g - mean[rid]) ** 2, 0.0), minlength=G)
    H = np.bincount(rid, weights=np.where(ok, np.asarray(hub, np.float64), 0.0), minlength=G)
    cnt = np.stack([n, np.bincount(rid, weights=stray, minlength=G)], axis=1).astype(np.int64)
    return cnt, np.stack([mean, m2, H], axis=1), np.bincount(rid, weights=np.abs(g), minlength=G) / nz


@functools.lru_cache(maxsize=None)
def depth_reference(case):
    """-> dict: loss, silog, huber, dz [N, H, W], valid, stray (depth_training_ref.depth_loss), and per run cnt [G, 2], part
    [G, 3] and gmag [G] (the mean |g|) in float64."""
    z, gt = depth_inputs(case)
    ls = dr.depth_loss(z, gt, DEPTH_WEIGHTS)
    ok = ls["ok"].reshape(-1)
    stray = ~(np.isfinite(z) & np.isfinite(gt)).reshape(-1)
    cnt, part, gmag = _run_stats(ls["g"].reshape(-1), _huber(ls["d"].reshape(-1)), ok, stray, shape_geo(case[1]))
    assert int(cnt[:, 0].sum()) == ls["valid"] and int(cnt[:, 1].sum()) == ls["stray"]
    return dict(loss=ls["loss"], silog=ls["silog"], huber=ls["huber"], dz=ls["dz"], valid=ls["valid"], stray=ls["stray"], ok=ls["ok"],
                cnt=cnt, part=part, gmag=gmag)


# ---- the exact cases -----------------------------------------------------------------------------------------------------
def exact_columns(case):
    """The columns of part that are exact in the case: all of them on one-hot logits, the class sums on uniform ones."""
    C = case[2]
    return {"onehot": np.arange(1 + 3 * C), "uniform": np.arange(1, 1 + 3 * C)}.get(case[0], np.arange(3, 1 + 3 * C, 3))


def exact_heads(case):
    """Per quantity (A, step): the terms lie on the grid ``step`` and the magnitudes of the terms of any sum the device forms,
    up to the merged one over all groups, add up to at most A."""
    ref = seg_reference(case)
    part = ref["part"]
    heads = {"I": (part[:, 1::3].sum(axis=0).max(), 1.0), "P": (part[:, 2::3].sum(axis=0).max(), 1.0), "T": (part[:, 3::3].sum(axis=0).max(), 1.0)}
    if case[0] == "onehot":
        heads["ce"] = (part[:, 0].sum(), 8.0)             # 200 = 8 x 25 per mismatch
    else:
        heads["I"], heads["P"] = (heads["I"][0], 0.25), (heads["P"][0], 0.25)
    return {k: (float(a), q) for k, (a, q) in heads.items()}


def check_exact(case):
    """What makes "exact" a checked fact -> {name: A / step / 2^24}: with A / step < 2^24 every partial sum, in any order, is an
    integer below 2^24 times the step, a float32 number; every reference entry lies on the grid and passes through float32
    unchanged, but for the exp(-200) = 1.4e-87 per term that float64 keeps of a one-hot pixel's other classes where the sum
    has no other term (float32 has 0 there)."""
    ref, used = seg_reference(case), {}
    tiny = LP * shape_geo(case[1])["cpg"] * np.exp(-200.0)
    cols = {"ce": slice(0, 1), "I": slice(1, None, 3), "P": slice(2, None, 3), "T": slice(3, None, 3)}
    for k, (a, step) in exact_heads(case).items():
        used[k] = a / step / 2.0 ** 24
        v = ref["part"][:, cols[k]]
        assert used[k] < 1.0, f"{k}: the terms' magnitudes sum to {a:.6g} on the grid {step}: {a / step:.6g} >= 2^24"
        v32 = v.astype(np.float32).astype(np.float64)
        assert np.array_equal(np.round(v32 / step) * step, v32), f"{k}: off the grid {step}"
        assert np.abs(v32 - v).max() <= tiny, f"{k}: does not pass through float32 unchanged"
    return used


# ---- the device's order in float32 ---------------------------------------------------------------------------------------
_LANES = np.arange(64)


def _butterfly(v):
    """for (o = 32; o > 0; o >>= 1) v += shfl_xor(v, o) along the last axis of 64 lanes -> any lane's value."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANES ^ o]
    return v[..., 0]


def _seq(terms, axis):
    """A sequential float sum from 0 along ``axis``."""
    terms = np.moveaxis(terms, axis, 0)
    acc = np.zeros(terms.shape[1:], terms.dtype)
    for t in terms:
        acc = acc + t
    return acc


def _padded(a, g):
    """[pixels, ...] -> [groups, cpg, LP, ...], zeros behind the last pixel."""
    full = g["groups"] * g["cpg"] * LP
    out = np.zeros((full,) + a.shape[1:], a.dtype)
    out[:a.shape[0]] = a
    return out.reshape((g["groups"], g["cpg"], LP) + a.shape[1:])


def _softmax32(zp):
    """The kernels' per-pixel softmax pieces in float32: the maximum, exp(z - m) and their sum in class order."""
    m = zp.max(axis=1)
    e = np.exp(zp - m[:, None])
    return m, e, _seq(e, 1)


@functools.lru_cache(maxsize=None)
def seg_eval32(case):
    """sl_sums_kernel, sl_merge_kernel and sl_grad_kernel restated in float32 numpy in the device's summation order -> dict:
    part [G, 1 + 3 C], loss, dz [N, C, H, W] (float32)."""
    _, shape, C = case
    N, H, W = SHAPES[shape]
    z, labels = seg_inputs(case)
    g = shape_geo(shape)
    f = np.float32
    lab = _classes(labels, C)
    ok = lab >= 0
    at = np.where(ok, lab, 0)
    rows = np.arange(g["total"])
    zp = pixel_major(z, C)
    m, e, s = _softmax32(zp)
    p = (e / s[:, None]) * ok[:, None].astype(f)
    t = np.zeros((g["total"], C), f)
    t[rows[ok], at[ok]] = 1.0
    # the CE term: a thread's pixels tid + 256 i of every chunk in order, the butterfly, the waves
    ce = _padded(np.where(ok, (m - zp[rows, at]) + np.log(s), f(0)).astype(f), g).reshape(g["groups"], g["cpg"] * 4, 4, 64)
    w = _butterfly(_seq(ce, 1))
    ce = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])

    def class_sums(v):      # lane l: pixels l, l + 64, ... of the chunk in order, the butterfly, then chunk after chunk
        v = _padded(v, g).reshape(g["groups"], g["cpg"], 16, 64, C)
        return _seq(_butterfly(np.moveaxis(_seq(v, 2), 2, -1)), 1)

    part = _part_layout(ce, class_sums(p * t), class_sums(p), class_sums(t))
    tot = _seq(part, 0)                                   # ordered_sum: the groups in order
    # the merge
    wce, wd = f(SEG_WEIGHTS[0]), f(SEG_WEIGHTS[1])
    I, S, T = tot[1::3], tot[2::3] + tot[3::3], tot[3::3]
    present = T > 0
    D = np.maximum(S, f(1e-7))
    dice = _seq(np.where(present, f(1) - f(2) * I / D, f(0)).astype(f), 0) / f(C)
    a = np.where(present, wd * (f(-2) / (f(C) * D)), f(0)).astype(f)
    b = np.where(present & (S > f(1e-7)), wd * (f(2) * I / (f(C) * D * D)), f(0)).astype(f)
    valid = int(ok.sum())
    k = wce / f(valid) if valid else f(0)
    loss = wce * (tot[0] / f(valid) if valid else f(0)) + wd * dice
    # the gradient
    gc = b[None, :] + a[at][:, None] * t
    dot = np.zeros(g["total"], f)
    for c in range(C):
        dot = p[:, c] * gc[:, c] + dot
    dz = (k * (p - t) + p * (gc - dot[:, None])) * ok[:, None].astype(f)
    assert part.dtype == f and dz.dtype == f and np.asarray(loss).dtype == f
    return dict(part=part, loss=float(loss), dz=frame_major(dz, N, H, W))


@functools.lru_cache(maxsize=None)
def depth_eval32(case):
    """pixel_terms and the Huber term restated in float32, every sum in float64, the gradient as dl_grad_kernel forms it ->
    dict: part [G, 3], loss, silog, huber, dz [N, H, W]."""
    z, gt = depth_inputs(case)
    shape = z.shape
    z, gt = z.reshape(-1), gt.reshape(-1)
    f = np.float32
    finite = np.isfinite(z) & np.isfinite(gt)
    ok = finite & (np.where(finite, gt, f(0)) > 0)
    zs, gs = np.where(ok, z, f(0)), np.where(ok, gt, f(1))
    e = np.exp(-np.abs(zs))
    r = f(1) / (f(1) + e)
    p, q = np.where(zs >= 0, r, e * r), np.where(zs >= 0, e * r, r)
    g = -(np.maximum(-zs, f(0)) + np.log1p(e)) - np.log(gs)
    d = p - gs
    ad = np.abs(d)
    hub = np.where(ad < f(1), f(0.5) * d * d, f(1) * (ad - f(0.5) * f(1)))
    assert g.dtype == f and hub.dtype == f and p.dtype == f
    _, part, _ = _run_stats(g, hub, ok, ~finite, shape_geo(case[1]))
    M = int(ok.sum())
    g64 = g[ok].astype(np.float64)
    mean = g64.sum() / M
    Dg = ((g64 - mean) ** 2).sum() / (M - 1) + dr.SILOG_LAMBDA * mean * mean
    root = np.sqrt(Dg)
    silog, huber = dr.SILOG_SCALE * root, hub[ok].astype(np.float64).sum() / M
    ws, wh = DEPTH_WEIGHTS
    kk = ws * 0.5 * dr.SILOG_SCALE / root
    a, b, h = f(kk * 2.0 / (M - 1)), f(kk * 2.0 * dr.SILOG_LAMBDA * mean / M), f(wh / M)
    dev = (g.astype(np.float64) - mean).astype(f)
    clip = np.where(ad < f(1), d, np.copysign(f(1), d))
    dz = np.where(ok, (a * dev + b) * q + h * clip * (p * q), f(0))
    assert dz.dtype == f
    return dict(part=part, loss=float(f(ws * silog + wh * huber)), silog=float(f(silog)), huber=float(f(huber)), dz=dz.reshape(shape))


# ---- error measures and bounds -------------------------------------------------------------------------------------------
SEG_QUANTITIES = ("loss", "dlogits", "part_ce", "part_I", "part_P")
DEPTH_QUANTITIES = ("loss", "silog", "huber", "dlogits", "run_mean", "run_M2", "run_huber")
_SEG_COLS = {"part_ce": slice(0, 1), "part_I": slice(1, None, 3), "part_P": slice(2, None, 3)}


def _scalar_err(v, v64):
    return abs(float(v) - v64) / abs(v64)


def _own_err(got, ref, scale=None):
    """max |got - ref| / scale over the entries with a term (scale > 0; default: the reference itself, a sum of terms of one
    sign) -> (the error, the entries without a term that are not exactly 0)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref) if scale is None else np.broadcast_to(scale, ref.shape)
    has = scale > 0
    e = float((np.abs(got - ref)[has] / scale[has]).max()) if has.any() else 0.0
    return e, int(np.count_nonzero(got[~has]))


def seg_errors(case, got):
    """got: dict with any of loss, dz, part -> {quantity: (error, entries that must be 0 and are not)}."""
    ref, out = seg_reference(case), {}
    if "loss" in got:
        out["loss"] = (_scalar_err(got["loss"], ref["loss"]), 0)
    if "dz" in got:
        out["dlogits"] = (rel_err(got["dz"], ref["dz"]), 0)
    if "part" in got:
        for k, cols in _SEG_COLS.items():
            out[k] = _own_err(np.asarray(got["part"])[:, cols], ref["part"][:, cols])
    return out


def depth_errors(case, got):
    ref, out = depth_reference(case), {}
    for k in ("loss", "silog", "huber"):
        if k in got:
            out[k] = (_scalar_err(got[k], ref[k]), 0)
    if "dz" in got:
        out["dlogits"] = (rel_err(got["dz"], ref["dz"]), 0)
    if "part" in got:
        part, n = np.asarray(got["part"], np.float64), ref["cnt"][:, 0]
        out["run_mean"] = _own_err(part[:, 0], ref["part"][:, 0], ref["gmag"])
        out["run_M2"] = _own_err(part[:, 1], ref["part"][:, 1], np.where(n >= 2, ref["part"][:, 1], 0.0))
        out["run_huber"] = _own_err(part[:, 2], ref["part"][:, 2])
    return out


@functools.lru_cache(maxsize=None)
def seg_own_errors():
    """-> {case: {quantity: the float32 restatement's error against float64}}"""
    return {case: {k: e for k, (e, _) in seg_errors(case, seg_eval32(case)).items()} for case in SEG_BOUND_CASES}


@functools.lru_cache(maxsize=None)
def seg_bounds():
    """-> {quantity: max(8 x the float32 restatement's error, 16 x 2^-24)}, the maximum over SEG_BOUND_CASES."""
    errs = seg_own_errors()
    return {k: max(8.0 * max(e[k] for e in errs.values()), FLOOR) for k in SEG_QUANTITIES}


@functools.lru_cache(maxsize=None)
def depth_own_errors(case):
    return {k: e for k, (e, _) in depth_errors(case, depth_eval32(case)).items()}


@functools.lru_cache(maxsize=None)
def depth_bounds(case):
    """-> {quantity: max(8 x the error of the float32-term evaluation of this case, 16 x 2^-24)}"""
    return {k: max(8.0 * e, FLOOR) for k, e in depth_own_errors(case).items()}


def _judge(errors, bounds, fails, ratios):
    for k, (e, nonzero) in errors.items():
        ratios[k] = e / bounds[k]
        if not e <= bounds[k]:
            fails.append(f"{k}: error {e:.3e} above its bound {bounds[k]:.3e}")
        if nonzero:
            fails.append(f"{k}: {nonzero} entries without a term are not exactly 0")


def _first_bad(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def evaluate_seg(case, got):
    """What test_gpu_loss_shapes.py asks of a device run and test_loss_shapes_cpu.py of a mutant.  got: cnt [G, 2], part
    [G, 1 + 3 C], and, if there, loss, dz, valid, stray -> (failures, {quantity: error / bound})."""
    ref, fails, ratios = seg_reference(case), [], {}
    cnt, part = np.asarray(got["cnt"]), np.asarray(got["part"])
    if cnt.shape != ref["cnt"].shape or part.shape != ref["part"].shape:
        return [f"{cnt.shape[0]} groups, not {ref['cnt'].shape[0]}"], ratios
    if not np.array_equal(cnt, ref["cnt"]):
        fails.append(f"cnt differs first at (group, valid | stray) {_first_bad(cnt != ref['cnt'])}")
    for k in ("valid", "stray"):
        if k in got and int(got[k]) != ref[k]:
            fails.append(f"{k} {int(got[k])}, not {ref[k]}")
    cols = exact_columns(case)                                      # the label counts are exact in every case
    bad = part.astype(np.float32)[:, cols] != ref["part"].astype(np.float32)[:, cols]
    if bad.any():
        b = _first_bad(bad)
        fails.append(f"part: {int(bad.sum())} exact entries differ, first at group {b[0]}, column {int(cols[b[1]])}")
    errors = seg_errors(case, got)
    if case[0] == "onehot":
        errors = {k: v for k, v in errors.items() if not k.startswith("part_")}
    _judge(errors, seg_bounds(), fails, ratios)
    if "dz" in got:
        dead = pixel_major(got["dz"], case[2])[_classes(seg_inputs(case)[1], case[2]) < 0]
        if np.count_nonzero(dead):
            fails.append("dlogits is not exactly 0 at an ignored or stray pixel")
    return fails, ratios


def evaluate_depth(case, got):
    """The same for depth.  got: cnt [G, 2], part [G, 3], and, if there, loss, silog, huber, dz, valid, stray."""
    ref, fails, ratios = depth_reference(case), [], {}
    cnt, part = np.asarray(got["cnt"]), np.asarray(got["part"])
    if cnt.shape != ref["cnt"].shape or part.shape != ref["part"].shape:
        return [f"{cnt.shape[0]} runs, not {ref['cnt'].shape[0]}"], ratios
    if not np.array_equal(cnt, ref["cnt"]):
        fails.append(f"cnt differs first at (run, valid | stray) {_first_bad(cnt != ref['cnt'])}")
    for k in ("valid", "stray"):
        if k in got and int(got[k]) != ref[k]:
            fails.append(f"{k} {int(got[k])}, not {ref[k]}")
    _judge(depth_errors(case, got), depth_bounds(case), fails, ratios)
    if "dz" in got and np.count_nonzero(np.asarray(got["dz"]).reshape(-1)[~ref["ok"].reshape(-1)]):
        fails.append("dlogits is not exactly 0 at an invalid or stray pixel")
    return fails, ratios


# ---- the walk, and the ways it could be wrong ----------------------------------------------------------------------------
def _wrap32(gp):
    return (gp + 2 ** 31) % 2 ** 32 - 2 ** 31


def _emulate_seg(case, mut):
    _, shape, C = case
    N, H, W = SHAPES[shape]
    HW = H * W
    z, labels = seg_inputs(case)
    zf, lab = z.reshape(-1), _classes(labels, C)
    g = shape_geo(shape)
    total, chunks, cpg = g["total"], g["chunks"], g["cpg"]
    G = chunks // cpg if mut == "floor_groups" else g["groups"]
    cnt, part = np.zeros((G, 2), np.int64), np.zeros((G, 1 + 3 * C))
    cls = np.arange(C)
    for b in range(G):
        if b == 0 or mut != "no_reset":
            acc, ce, valid, stray = np.zeros((3, C)), 0.0, 0, 0
        q_end = min((b + 1) * cpg, chunks) - (mut == "skip_last_chunk")
        for q in range(b * cpg, q_end):
            gp = np.arange(q * LP, min((q + 1) * LP, total))
            if mut == "int32_pixel":
                gp = _wrap32(gp)
            l = lab[gp]
            stray += int((l == -2).sum())
            n = np.full(gp.shape, gp[0] // HW) if mut == "frame_of_chunk" else gp // HW
            gp, n, l = gp[l >= 0], n[l >= 0], l[l >= 0]
            if not gp.size:
                continue
            base = n * C * HW + (gp - n * HW)
            zc = zf[base[:, None] + cls[None, :] * HW].astype(np.float64)
            m = zc.max(axis=1)
            e = np.exp(zc - m[:, None])
            s = e.sum(axis=1)
            p = e / s[:, None]
            hit = np.arange(gp.size)
            ce += float(((m - zc[hit, l]) + np.log(s)).sum())
            valid += gp.size
            acc[0] += np.bincount(l, weights=p[hit, l], minlength=C)
            acc[1] += p.sum(axis=0)
            acc[2] += np.bincount(l, minlength=C)
        cnt[b] = valid, stray
        part[b, 0] = ce
        part[b, 1::3], part[b, 2::3], part[b, 3::3] = acc
    return dict(cnt=cnt, part=part)


def _emulate_depth(case, mut):
    z, gt = depth_inputs(case)
    ref = dr.depth_loss(z, gt, DEPTH_WEIGHTS)
    g64, hub, ok = ref["g"].reshape(-1), _huber(ref["d"].reshape(-1)), ref["ok"].reshape(-1)
    stray_px = ~(np.isfinite(z) & np.isfinite(gt)).reshape(-1)
    g = shape_geo(case[1])
    total, chunks, cpg = g["total"], g["chunks"], g["cpg"]
    G = chunks // cpg if mut == "floor_groups" else g["groups"]
    cnt, part = np.zeros((G, 2), np.int64), np.zeros((G, 3))
    for b in range(G):
        if b == 0 or mut != "no_reset":
            n, mean, m2, H, stray = 0, 0.0, 0.0, 0.0, 0
            s1, s2 = np.float32(0), np.float32(0)              # raw_moments: the run's sum g and sum g^2
        q_end = min((b + 1) * cpg, chunks) - (mut == "skip_last_chunk")
        for q in range(b * cpg, q_end):
            gp = np.arange(q * LP, min((q + 1) * LP, total))
            if mut == "int32_pixel":
                gp = _wrap32(gp)
            stray += int(stray_px[gp].sum())
            gc = g64[gp][ok[gp]]
            H += float(hub[gp][ok[gp]].sum())
            nb = gc.size
            if nb == 0:
                continue
            if mut == "raw_moments":
                g32 = gc.astype(np.float32)
                s1, s2 = s1 + g32.sum(dtype=np.float32), s2 + (g32 * g32).sum(dtype=np.float32)
                n += nb
                mean, m2 = float(s1) / n, float(s2) - float(s1) * float(s1) / n
                continue
            mb = gc.sum() / nb
            m2b = float(((gc - mb) ** 2).sum())
            if n == 0:
                n, mean, m2 = nb, mb, m2b
            else:                                               # Chan et al.
                nt, delta = n + nb, mb - mean
                m2 += m2b + delta * delta * (n * nb / nt)
                mean += delta * (nb / nt)
                n = nt
        cnt[b] = n, stray
        part[b] = mean, m2, H
    return dict(cnt=cnt, part=part)


def emulate_groups(case, mut=None):
    """The per-group partials in float64 by the kernels' own walk: group by group, chunk by chunk, a pixel's frame and
    address from its index -> dict(cnt, part).  mut: one of MUTANTS, or None for the walk as it should be."""
    assert mut is None or mut in MUTANTS
    if case in DEPTH_CASES:
        assert mut != "frame_of_chunk"
        return _emulate_depth(case, mut)
    assert mut != "raw_moments"
    return _emulate_seg(case, mut)


def evaluate(case, got):
    return (evaluate_depth if case in DEPTH_CASES else evaluate_seg)(case, got)

