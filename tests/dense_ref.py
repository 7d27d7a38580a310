"""numpy oracle of the dense-head scores (include/kp2d.h, kp2d_seg_stats / kp2d_depth_sums), written from the contract's
text: exact integer counts, float64 terms summed exactly (math.fsum), the header's depth error bounds restated, and the
seeded inputs the CPU and the GPU tests share.  Unpinned by the reference's libraries: smp and OpenCV are absent."""
import functools
import math

import numpy as np

U = 2.0 ** -53
LOG_ULP = 4                      # the header's assumption for the device's double log / log10
DEPTH_CHUNK, WG = 4096, 256
NSUMS = 11
FLOAT_SLOTS = (4, 5, 6, 7, 8, 9)
DEPTH_KEYS = ("a1", "a2", "a3", "abs_rel", "sq_rel", "rmse", "rmse_log", "silog", "log_10")
REDUCTIONS = (None, "micro", "macro", "micro-imagewise", "macro-imagewise")


# ---- segmentation -------------------------------------------------------------------------------------------------
def seg_stats(pred, target, C, ignore=None):
    """pred, target [B, n] integers -> stats [B, C, 4] (tp, fp, fn, tn), confusion [B, C, C], ignored [B], stray [B]."""
    pred, target = np.asarray(pred).astype(np.int64), np.asarray(target).astype(np.int64)
    B = pred.shape[0]
    stats = np.zeros((B, C, 4), np.int64)
    conf = np.zeros((B, C, C), np.int64)
    ignored, stray = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for b in range(B):
        g, p = target[b].ravel(), pred[b].ravel()
        ig = (g == ignore) if ignore is not None else np.zeros(g.shape, bool)
        out = ~ig & ((g < 0) | (g >= C) | (p < 0) | (p >= C))
        ok = ~ig & ~out
        ignored[b], stray[b] = ig.sum(), out.sum()
        conf[b] = np.bincount(g[ok] * C + p[ok], minlength=C * C).reshape(C, C)
        tp = np.diag(conf[b])
        stats[b, :, 0] = tp
        stats[b, :, 1] = conf[b].sum(0) - tp          # predicted c, target another class
        stats[b, :, 2] = conf[b].sum(1) - tp          # target c, predicted another class
        stats[b, :, 3] = ok.sum() - stats[b, :, :3].sum(1)
    return stats, conf, ignored, stray


def _ratio(num, den, zero_division):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.where(den == 0, float(zero_division), num / np.where(den == 0, 1.0, den))


def score(kind, stats, reduction=None, zero_division=1.0):
    """kind in ("iou", "accuracy", "f1") of stats [B, C, 4] under one of REDUCTIONS."""
    s = np.asarray(stats, np.int64)
    if reduction == "micro":
        s = s.sum((0, 1))
    elif reduction == "macro":
        s = s.sum(0)
    elif reduction == "micro-imagewise":
        s = s.sum(1)
    tp, fp, fn, tn = (s[..., i] for i in range(4))
    if kind == "iou":
        r = _ratio(tp, tp + fp + fn, zero_division)
    elif kind == "accuracy":
        r = _ratio(tp + tn, tp + fp + fn + tn, zero_division)
    else:
        r = _ratio(2 * tp, 2 * tp + fn + fp, zero_division)
    return r if reduction is None else float(np.mean(r))


def evaluate_segmentation(batches, C, ignore=255):
    """batches: (pred, target) per batch -> the four keys, each the mean over batches of the batch's score."""
    rows = []
    for pred, target in batches:
        st = seg_stats(pred, target, C, ignore)[0]
        rows.append([score("iou", st, "micro-imagewise"), score("accuracy", st, "micro-imagewise"),
                     score("f1", st, "micro-imagewise"), score("iou", st, "macro-imagewise")])
    return dict(zip(("IoU", "accuracy", "f1", "IoU_macro"), np.mean(np.asarray(rows, np.float64), 0).tolist()))


def seg_case(B, H, W, C, dtype, seed, kinds, ignore=255, strays=True):
    """Seeded class maps [B, H, W]: pred int64, target of ``dtype``.  kinds[b]: "mixed" (70 % of pixels right, ~10 %
    ignored, a few stray values in both maps), "ignored" (every target = ignore), "equal" (pred = target, no ignored pixel)
    or "single" (one target class).  Stray values are those the dtype and C leave free: with uint8 targets and C = 256
    there is none on the target side, and ``ignore`` itself is never planted as a stray."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    target = rng.integers(0, C, (B, H, W)).astype(np.int64)
    pred = np.where(rng.random((B, H, W)) < 0.7, target, rng.integers(0, C, (B, H, W)))
    free = [v for v in (C, C + 7, -3, info.max) if info.min <= v <= info.max and not 0 <= v < C and v != ignore]
    for b, kind in enumerate(kinds):
        if kind == "ignored":
            target[b] = ignore
        elif kind == "equal":
            pred[b] = target[b]
        elif kind == "single":
            target[b] = C // 2
        if kind in ("mixed", "single"):
            if ignore is not None and info.min <= ignore <= info.max:
                target[b][rng.random((H, W)) < 0.1] = ignore
            if strays:
                for v in free:
                    target[b].ravel()[rng.choice(H * W, 3, replace=False)] = v
                for v in (C, -1, 2 ** 40):
                    pred[b].ravel()[rng.choice(H * W, 3, replace=False)] = v
    return pred.astype(np.int64), target.astype(dtype)


# ---- depth --------------------------------------------------------------------------------------------------------
def depth_valid(g, p, valid=None, min_depth=None, max_depth=None):
    """The invalid-pixel rule on float32 maps of any shape -> boolean mask of the VALID pixels."""
    g64, p64 = g.astype(np.float64), p.astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(g64) & np.isfinite(p64) & (g64 > 0) & (p64 > 0)
        if min_depth is not None:
            ok &= ~(g64 < float(min_depth))
        if max_depth is not None:
            ok &= ~(g64 > float(max_depth))
    if valid is not None:
        ok &= np.asarray(valid) != 0
    return ok


def depth_terms(g, p):
    """float64 terms of the VALID pixels g, p (1-d): slot -> array, for the slots 1..9."""
    g, p = g.astype(np.float64), p.astype(np.float64)
    r = np.maximum(g / p, p / g)
    d, dl = g - p, np.log(g) - np.log(p)
    return {1: (r < 1.25).astype(np.float64), 2: (r < 1.25 ** 2).astype(np.float64), 3: (r < 1.25 ** 3).astype(np.float64),
            4: np.abs(d) / g, 5: d * d / g, 6: d * d, 7: dl * dl, 8: np.log(p) - np.log(g), 9: np.abs(np.log10(g) - np.log10(p))}


def depth_terms_f32(g, p, slot):
    """The terms of one floating slot with every operation in float32: what the bound has to tell from float64 work."""
    g, p = g.astype(np.float32), p.astype(np.float32)
    d = g - p
    t = {4: lambda: np.abs(d) / g, 5: lambda: d * d / g, 6: lambda: d * d, 7: lambda: (np.log(g) - np.log(p)) ** 2,
         8: lambda: np.log(p) - np.log(g), 9: lambda: np.abs(np.log10(g) - np.log10(p))}[slot]()
    assert t.dtype == np.float32
    return t.astype(np.float64)


def depth_depth(n):
    """D(n) of the header: the rounded additions a term can take part in."""
    return 33 + -(-(-(-n // DEPTH_CHUNK)) // WG)


def _workgroup_sum(rows):
    """rows [m, k]: thread t of 256 adds rows t, t + 256, ... in order; lanes by a butterfly, the four waves in order."""
    m, k = rows.shape
    steps = -(-m // WG)
    padded = np.zeros((steps * WG, k), np.float64)      # adding 0.0 is exact: the padding changes nothing
    padded[:m] = rows
    acc = np.zeros((WG, k), np.float64)
    for j in range(steps):
        acc = acc + padded[j * WG:(j + 1) * WG]
    lane = np.arange(WG)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ o]
    return ((acc[0] + acc[64]) + acc[128]) + acc[192]


def emulate_sum(t):
    """The device's order for one image's terms t [n] (csrc/dense_metrics.hip): chunks of 4096 pixels, each summed by a
    workgroup, then the chunk sums summed the same way.  Float64 throughout, like the device."""
    n = len(t)
    nchunk = -(-n // DEPTH_CHUNK)
    padded = np.zeros(nchunk * DEPTH_CHUNK, np.float64)
    padded[:n] = t
    # [chunk, step, thread] -> the chunks ride along as columns
    part = _workgroup_sum(padded.reshape(nchunk, DEPTH_CHUNK).T.copy())
    return float(_workgroup_sum(part[:, None])[0])


def depth_magnitudes(g, p):
    """Per-pixel magnitudes a_i of the header's bounds for the floating slots, and the constants c in units of U."""
    g, p = g.astype(np.float64), p.astype(np.float64)
    t = depth_terms(g, p)
    lg, lp, l10g, l10p = np.abs(np.log(g)), np.abs(np.log(p)), np.abs(np.log10(g)), np.abs(np.log10(p))
    d, d10 = np.abs(np.log(g) - np.log(p)), t[9]
    a = {4: t[4], 5: t[5], 6: t[6], 7: d * d + d * (lg + lp), 8: d + lg + lp, 9: d10 + l10g + l10p}
    c = {4: 2, 5: 4, 6: 3, 7: 3 + 4 * LOG_ULP, 8: 1 + 2 * LOG_ULP, 9: 1 + 2 * LOG_ULP}
    return a, c


def depth_bounds(g, p, n):
    """slot -> the header's bound on |device sum - float64 sum| for one image of n pixels whose valid pixels are g, p."""
    a, c = depth_magnitudes(g, p)
    D = depth_depth(n)
    return {s: 1.001 * (D + c[s]) * U * math.fsum(a[s]) for s in FLOAT_SLOTS}


def depth_sums(gt, pred, valid=None, min_depth=None, max_depth=None):
    """gt, pred [B, ...] float32 -> sums [B, NSUMS] float64, every sum exactly rounded (math.fsum)."""
    B = gt.shape[0]
    out = np.zeros((B, NSUMS), np.float64)
    for b in range(B):
        g, p = gt[b].ravel(), pred[b].ravel()
        ok = depth_valid(g, p, None if valid is None else np.asarray(valid[b]).ravel(), min_depth, max_depth)
        t = depth_terms(g[ok], p[ok])
        out[b, 0], out[b, 10] = ok.sum(), (~ok).sum()
        for s in range(1, 10):
            out[b, s] = math.fsum(t[s])
    return out


def depth_metrics(row):
    """One row of sums -> the nine metrics (float64; count 0: NaN)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.asarray(row[1:10], np.float64) / np.float64(row[0])
        silog = 100.0 * np.sqrt(np.maximum(m[6] - m[7] * m[7], 0.0)) if row[0] > 0 else np.nan
        vals = [m[0], m[1], m[2], m[3], m[4], np.sqrt(m[5]), np.sqrt(m[6]), silog, m[8]]
    return dict(zip(DEPTH_KEYS, (float(v) for v in vals)))


def compute_errors(gt, pred, valid=None, min_depth=None, max_depth=None):
    rows = depth_sums(gt, pred, valid, min_depth, max_depth)
    return depth_metrics([math.fsum(rows[:, s]) for s in range(NSUMS)])


DEPTH_SHAPES = ((3, 37, 53), (2, 240, 320))
DEPTH_LIMITS = (1.0, 70.0)


@functools.lru_cache(maxsize=None)
def depth_case(B, H, W, seed=0):
    """The issue's depth inputs: gt uniform in [0.5, 80], pred = gt exp(0.3 z); planted zeros and negatives in gt, a NaN and
    an inf in pred, and a ``valid`` mask with ~5 % zeros.  DEPTH_LIMITS cut both tails of gt.  Shared, read-only."""
    rng = np.random.default_rng(1000 + seed + H)
    gt = rng.uniform(0.5, 80.0, (B, H, W)).astype(np.float32)
    pred = (gt * np.exp(0.3 * rng.standard_normal((B, H, W)))).astype(np.float32)
    valid = (rng.random((B, H, W)) >= 0.05).astype(np.uint8)
    for b in range(B):
        at = rng.choice(H * W, 8, replace=False)
        gt[b].ravel()[at[:3]] = 0.0
        gt[b].ravel()[at[3:6]] = -2.5
        pred[b].ravel()[at[6]] = np.nan
        pred[b].ravel()[at[7]] = np.inf
    for a in (gt, pred, valid):
        a.setflags(write=False)
    return gt, pred, valid
