"""Case tables, float64 references, bounds and child-process source of the keypoint post-processing and selection tests.
Test infrastructure, shared by test_post_select_ref_cpu.py (CPU: the references against torch, the float32 emulation and
its mutants against the bounds, csrc/select_form.h against the tables) and test_gpu_post_select_fp64.py (GPU: every case;
the forms behind KP2D_TOPK_SMALL, KP2D_GATHER_LDS=0 and KP2D_MATCH_MFMA=0 in one child process per value).

The stage: csrc/post.hip (post_kernel<C>, the three class-id kernels, the top-k kernels, the gather kernels) through the
C ABI (kp2d_post, kp2d_select_topk, kp2d_gather_keypoints), and csrc/match.hip's VALU search from 256 train rows up.

Post-processing reference.  oracle.kp2d_oracle.post_processing in float64 on the same float32 inputs.  ``emulate`` restates
it with switches for the mutants; without a switch it IS the oracle, bit for bit, in float32 and float64 (asserted on the CPU).

Bounds.  u = 2^-24.  Every bound is computed per element from the float64 reference's own quantities; none from a device.
  score   equal to score * mask, bit for bit.
  coord   base = xc * cell + step is exact (small integers and halves).  t = sx * gain rounds once (|err| <= u |t|), the sum
          base + t rounds once (<= u |cx before the clamp|), the clamp is monotone and its ends are float32 numbers:
              |err| <= u (|sx gain| + |cx before the clamp|) (1 + 2^-20),
          the last factor for the reference's own rounding.  Regime ``grid``: equal.
  desc    v[c] = sum of four w f, d = v / |v|.  Against float64 sampling at the float64 coordinates:
          (1) arithmetic at a given sample coordinate: wx0 = (x0 + 1) - ix and wy0 round once each (wx1 = ix - x0 is exact),
              their product once, w f once, the three sums once each: 7 roundings on a term at most,
                  e1[c] = 7 u sum |w f|;
          (2) the sample coordinate ix = ((cx / ((W - 1) / 2) - 1) + 1) * 0.5 * (Wf - 1).  With s = (Wf - 1) / (W - 1): the
              coordinate's error arrives as ecx s; the division rounds (<= u (gx + 1), which times 0.5 (Wf - 1) is u ix), the
              -1 rounds (<= u |gx| <= u, times 0.5 (Wf - 1)), the +1 rounds (<= u (gx + 1): u ix again), * 0.5 is exact,
              * (Wf - 1) rounds (<= u ix):
                  dx = ecx s + u (3 |ix| + 0.5 (Wf - 1)),       likewise dy
              ("a few u of |ix| + Wf").  v is continuous and piecewise bilinear in (ix, iy), so it moves by at most
                  e2[c] = dx |dv/dix| + dy |dv/diy| + dx dy |f00 - f01 - f10 + f11|,
              the slopes taken in the reference's own patch and, where ix (iy) lies within dx (dy) of an integer, as the
              larger of the two patches meeting there (patches outside the map are never entered: 0 <= ix <= Wf - 1);
          (3) both through the division by the norm.  The norm itself: C / 4 fused multiply-adds per quarter and three
              sums (relative (C / 4 + 3) u on the sum of squares, half of it on the root), the root and the division round
              once each: c4 = (C / 4 + 3) / 2 + 2.  With ev = e1 + e2:
                  |err d[c]| <= (ev[c] / |v| + |d[c]| (||ev|| / |v| + c4 u)) (1 + 2^-10),
              the last factor for the terms of second order.
          A cell whose reference norm is 0 (regime ``z``) must be NaN in all C channels, and no other cell may be.
  dense class ids   equal to numpy.argmax of the same float32 logits (the first maximum; -0.0 == +0.0).
  sampled class ids equal to oracle grid_sample_nearest in float64 AT THE DEVICE'S OWN float32 coordinates, except where the
          float64 ix or iy lies within 8 u (|ix| + 1) of k + 0.5 (the five roundings of (2) without ecx, and room); at most
          2 % of a case's cells.  Regime ``grid``: every cell, the halves round to even.
  top-k   candidates s > thr (never NaN, never -inf under thr = -inf), ordered by value descending with -0.0 == +0.0, then
          index ascending; idx, val (the score's own bits, sign included) and count equal.
  gather  plain indexing, bit for bit; a row of zeros where idx is -1.
  guards  outputs sit inside larger buffers filled with a sentinel; no sentinel may change.
"""
import functools
import os
import zlib

import numpy as np

from oracle import kp2d_oracle as orc

U = 2.0 ** -24
REF_SLACK = 1.0 + 2.0 ** -20
SECOND_ORDER = 1.0 + 2.0 ** -10
C1 = 7.0
NEAR_HALF = 8.0
MAX_LEFT_OUT = 0.02
SEED = 20261
PAD = 64                        # guard elements on either side of an output
SENT_F, SENT_I = -777.25, -7777
INF = float("inf")

# name -> (tiny_factory / oracle configuration, cell, descriptor channels)
MODELS = {"S": ("S", 4, 32), "F": ("F", 8, 64), "D": ("D", 4, 128)}


def _rng(name, salt=0):
    return np.random.default_rng([SEED, zlib.crc32(name.encode()), salt])


# ---------------------------------------------------------------------------------------------------------------------
# post-processing: the case table
# ---------------------------------------------------------------------------------------------------------------------
def _pc(model, B, cells, fmap, regime="u", hw=None, seg=None, seg_regime="n", seg_off=0, argmax="fused,quad"):
    cell = MODELS[model][1]
    return dict(model=model, B=B, cells=cells, fmap=fmap, regime=regime, hw=hw or (cell * cells[0], cell * cells[1]),
                seg=seg or (28,) + tuple(fmap), seg_regime=seg_regime, seg_off=seg_off, argmax=argmax)


def _ac(seg, seg_regime="n", seg_off=0, argmax="fused,quad"):
    """a class-id case: the post part is S over 3 x 5 cells, the class map has a shape of its own"""
    return _pc("S", 2, (3, 5), (6, 10), seg=seg, seg_regime=seg_regime, seg_off=seg_off, argmax=argmax)


TWO = "two,scalar"
POST_CASES = {
    # ---- S: every shape.  cells over feature map; 64 cells per workgroup ----
    "S-1x1-u": _pc("S", 1, (1, 1), (2, 2)),
    "S-3x5-u": _pc("S", 2, (3, 5), (6, 10)),                                   # one partial workgroup
    "S-3x5-clamp-h": _pc("S", 2, (3, 5), (6, 10), "clamp", hw=(9, 20)),         # H = cell Hc - 3
    "S-3x5-f1": _pc("S", 1, (3, 5), (1, 1), argmax=TWO),                       # Hf = Wf = 1
    "S-8x8-u": _pc("S", 3, (8, 8), (16, 16)),                                  # exactly one workgroup
    "S-5x13-u": _pc("S", 2, (5, 13), (7, 11), argmax=TWO),                     # 65 cells, an odd feature map
    "S-5x13-clamp": _pc("S", 2, (5, 13), (7, 11), "clamp", argmax=TWO),
    "S-9x13-u": _pc("S", 1, (9, 13), (18, 26)),
    "S-9x13-clamp": _pc("S", 2, (9, 13), (18, 26), "clamp"),
    "S-9x13-z": _pc("S", 2, (9, 13), (18, 26), "z"),
    # W = H = 65 over a 33 x 33 map: every division exact; the class map of S-grid97 puts halves on EVEN k
    "S-grid": _pc("S", 2, (16, 16), (33, 33), "grid", hw=(65, 65), argmax=TWO),
    "S-grid97": _pc("S", 1, (16, 16), (33, 33), "grid", hw=(65, 65), seg=(19, 97, 97), argmax=TWO),
    # ---- F (cell 8, C = 64) and D (cell 4, C = 128): one full and one partial shape ----
    "F-8x8-u": _pc("F", 2, (8, 8), (16, 16)),
    "F-3x5-clamp": _pc("F", 1, (3, 5), (6, 10), "clamp"),
    "D-8x8-u": _pc("D", 1, (8, 8), (16, 16)),
    "D-5x13-u": _pc("D", 2, (5, 13), (7, 11), argmax=TWO),
    "D-9x13-z": _pc("D", 1, (9, 13), (18, 26), "z"),
    # ---- dense class ids: C in {1, 19, 28}; HW 35 (scalar), 36 (quad), 1028 (a second block with one live quad); a view one
    #      float into a larger buffer (HW % 4 == 0, misaligned: scalar); exact ties across classes ----
    "A-c1-35": _ac((1, 5, 7), argmax=TWO),
    "A-c19-35": _ac((19, 5, 7), argmax=TWO),
    "A-c28-35-ties": _ac((28, 5, 7), "ties", argmax=TWO),
    "A-c1-36": _ac((1, 6, 6)),
    "A-c19-36": _ac((19, 6, 6)),
    "A-c28-36-ties": _ac((28, 6, 6), "ties"),
    "A-c28-36-off1": _ac((28, 6, 6), seg_off=1, argmax=TWO),
    "A-c19-36-off1-ties": _ac((19, 6, 6), "ties", seg_off=1, argmax=TWO),
    "A-c19-1028": _ac((19, 4, 257)),
    "A-c28-1028-ties": _ac((28, 4, 257), "ties"),
    "A-c19-1028-off1": _ac((19, 4, 257), seg_off=1, argmax=TWO),
}


def post_dims(case):
    c = POST_CASES[case]
    _, cell, C = MODELS[c["model"]]
    return dict(B=c["B"], Hc=c["cells"][0], Wc=c["cells"][1], Hf=c["fmap"][0], Wf=c["fmap"][1], H=c["hw"][0], W=c["hw"][1],
                cell=cell, C=C, Cs=c["seg"][0], Hs=c["seg"][1], Ws=c["seg"][2])


@functools.lru_cache(maxsize=None)
def post_inputs(case):
    """score, shift, feat, seg: float32, seeded by the case's name"""
    c, d = POST_CASES[case], post_dims(case)
    g = _rng(case)
    B, Hc, Wc = d["B"], d["Hc"], d["Wc"]
    score = g.random((B, 1, Hc, Wc)).astype(np.float32)
    if c["regime"] == "grid":
        shift = g.choice(np.array([-0.5, 0.5], np.float32), (B, 2, Hc, Wc))
    else:
        amp = 6.0 if c["regime"] == "clamp" else 1.0
        shift = (g.random((B, 2, Hc, Wc)) * 2 * amp - amp).astype(np.float32)
    feat = g.standard_normal((B, d["C"], d["Hf"], d["Wf"])).astype(np.float32)
    if c["regime"] == "z":      # a block that is zero in every channel
        feat[:, :, d["Hf"] // 4:3 * d["Hf"] // 4, d["Wf"] // 4:3 * d["Wf"] // 4] = 0.0
    seg = g.standard_normal((B, d["Cs"], d["Hs"], d["Ws"])).astype(np.float32)
    if c["seg_regime"] == "ties" and d["Cs"] > 1:
        flat = seg.reshape(B, d["Cs"], -1)
        for b in range(B):
            for p in np.nonzero(g.random(flat.shape[2]) < 0.3)[0]:       # the exact maximum in two or three channels
                others = g.choice(d["Cs"], int(g.integers(2, 4)), replace=False)
                flat[b, others, p] = flat[b, :, p].max()
            for p in np.nonzero(g.random(flat.shape[2]) < 0.05)[0]:      # -0.0 before +0.0, everything else below
                lo, hi = np.sort(g.choice(d["Cs"], 2, replace=False))
                flat[b, :, p] = -1.0 - g.random(d["Cs"]).astype(np.float32)
                flat[b, lo, p], flat[b, hi, p] = -0.0, 0.0
    return {"score": score, "shift": shift, "feat": feat, "seg": seg}


# ---------------------------------------------------------------------------------------------------------------------
# post-processing: the oracle restated with switches (mut=None: the oracle itself)
# ---------------------------------------------------------------------------------------------------------------------
POST_MUTANTS = ("align_false", "feat_size", "swap_w", "swap_xy", "step_half", "ratio1", "clamp_W", "norm3", "eps", "border2",
                "last_max", "half_up", "trunc")


def _sample_coords(c, size, full, dt, mut):
    """normalize_coord with the IMAGE size, grid_sample's un-normalisation with the map's size"""
    norm = (size - 1) if mut == "feat_size" and size > 1 else (full - 1)
    g = c / dt.type(norm / 2.0) - dt.type(1)
    if mut == "align_false":
        return ((g + dt.type(1)) * dt.type(size) - dt.type(1)) / dt.type(2)
    return (g + dt.type(1)) / dt.type(2) * dt.type(size - 1)


def _bilinear(feat, ix, iy, mut):
    B, C, Hi, Wi = feat.shape
    dt = feat.dtype
    x0, y0 = np.floor(ix), np.floor(iy)
    out = np.zeros((B, C) + ix.shape[1:], dt)
    bi = np.arange(B)[:, None, None]
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            wx = (ix - x0) if (dx ^ (mut == "swap_w")) else (x0 + dt.type(1) - ix)
            wy = (iy - y0) if dy else (y0 + dt.type(1) - iy)
            ok = (xi >= 0) & (xi <= Wi - 1) & (yi >= 0) & (yi <= Hi - 1)
            val = feat[bi, :, np.clip(yi, 0, Hi - 1).astype(np.int64), np.clip(xi, 0, Wi - 1).astype(np.int64)]
            out += (val * (wx * wy * ok)[..., None]).transpose(0, 3, 1, 2)
    return out


def _round(v, mut):
    if mut == "half_up":
        return np.floor(v + v.dtype.type(0.5))
    if mut == "trunc":
        return np.trunc(v)
    return np.rint(v)


def nearest_ids(seg, ix, iy, mut=None):
    """argmax over the classes of the nearest pixel (zeros outside) -> int64 [B, Hc, Wc]"""
    B, C, Hi, Wi = seg.shape
    xi, yi = _round(ix, mut).astype(np.int64), _round(iy, mut).astype(np.int64)
    ok = (xi >= 0) & (xi < Wi) & (yi >= 0) & (yi < Hi)
    bi = np.arange(B)[:, None, None]
    val = seg[bi, :, np.clip(yi, 0, Hi - 1), np.clip(xi, 0, Wi - 1)] * ok[..., None]
    return val.argmax(axis=-1).astype(np.int64)


def argmax_ids(seg, mut=None):
    if mut == "last_max":
        return (seg.shape[1] - 1 - seg[:, ::-1].argmax(axis=1)).astype(np.int64)
    return seg.argmax(axis=1).astype(np.int64)


def emulate(case, dtype, mut=None):
    """post_processing of the case's inputs in ``dtype`` -> dict(score, coord, desc, ids_dense, ids_samp).  mut=None:
    oracle.kp2d_oracle.post_processing, operation by operation."""
    d, inp = post_dims(case), post_inputs(case)
    dt = np.dtype(dtype)
    score, shift, feat, seg = (inp[k].astype(dt) for k in ("score", "shift", "feat", "seg"))
    Hc, Wc, H, W, cell = d["Hc"], d["Wc"], d["H"], d["W"], d["cell"]
    ring = 2 if mut == "border2" else 1
    mask = np.zeros((Hc, Wc), dt)
    mask[ring:Hc - ring, ring:Wc - ring] = 1
    if mut == "swap_xy":
        shift = shift[:, ::-1]
    step = dt.type(cell / 2.0 if mut == "step_half" else (cell - 1) / 2.0)
    ratio = dt.type(1.0 if mut == "ratio1" else 2.0)
    xs = np.broadcast_to(np.arange(Wc, dtype=dt)[None, :], (Hc, Wc))
    ys = np.broadcast_to(np.arange(Hc, dtype=dt)[:, None], (Hc, Wc))
    coord = (np.stack([xs, ys])[None] * dt.type(cell) + step + shift * (ratio * step)).copy()
    top = 0 if mut == "clamp_W" else 1
    coord[:, 0] = np.clip(coord[:, 0], 0, W - top)
    coord[:, 1] = np.clip(coord[:, 1], 0, H - top)
    ix, iy = _sample_coords(coord[:, 0], d["Wf"], W, dt, mut), _sample_coords(coord[:, 1], d["Hf"], H, dt, mut)
    f = _bilinear(feat, ix, iy, mut)
    sq = f * f
    if mut == "norm3":
        sq = sq[:, :3 * d["C"] // 4]
    nrm = np.sqrt(sq.sum(axis=1, keepdims=True))
    if mut == "eps":
        nrm = np.maximum(nrm, dt.type(1e-12))
    with np.errstate(invalid="ignore", divide="ignore"):
        desc = f / nrm
    sx, sy = _sample_coords(coord[:, 0], d["Ws"], W, dt, mut), _sample_coords(coord[:, 1], d["Hs"], H, dt, mut)
    return {"score": score * mask, "coord": coord, "desc": desc, "ids_dense": argmax_ids(seg, mut)[:, None],
            "ids_samp": nearest_ids(seg, sx, sy, mut)[:, None]}


def oracle_post(case, dtype, sample):
    """oracle.kp2d_oracle.post_processing itself"""
    inp = post_inputs(case)
    d = post_dims(case)
    out = {"score": inp["score"].astype(dtype), "coord": inp["shift"].astype(dtype), "feat": inp["feat"].astype(dtype),
           "seg": inp["seg"].astype(dtype)}
    with np.errstate(invalid="ignore", divide="ignore"):
        return orc.post_processing(out, d["H"], d["W"], orc.get_config(MODELS[POST_CASES[case]["model"]][0]), training=False,
                                   sample_segmentation=sample)


# ---------------------------------------------------------------------------------------------------------------------
# post-processing: the bounds (module docstring), from float64 quantities only
# ---------------------------------------------------------------------------------------------------------------------
def _fetch(feat, yi, xi):
    """feat[b, :, yi, xi] with zeros outside -> [B, Hc, Wc, C]"""
    B, C, Hi, Wi = feat.shape
    ok = (xi >= 0) & (xi < Wi) & (yi >= 0) & (yi < Hi)
    bi = np.arange(B)[:, None, None]
    return feat[bi, :, np.clip(yi, 0, Hi - 1), np.clip(xi, 0, Wi - 1)] * ok[..., None]


@functools.lru_cache(maxsize=None)
def post_bounds(case):
    """-> dict(coord: bound [B, 2, Hc, Wc]; desc: bound [B, C, Hc, Wc] (NaN where the reference is NaN); ref: the float64
    reference (emulate(case, float64)))"""
    d, inp = post_dims(case), post_inputs(case)
    ref = emulate(case, np.float64)
    shift, feat = inp["shift"].astype(np.float64), inp["feat"].astype(np.float64)
    Hc, Wc, cell, C = d["Hc"], d["Wc"], d["cell"], d["C"]
    step = (cell - 1) / 2.0
    base = np.stack([np.broadcast_to(np.arange(Wc, dtype=np.float64)[None, :], (Hc, Wc)),
                     np.broadcast_to(np.arange(Hc, dtype=np.float64)[:, None], (Hc, Wc))])[None] * cell + step
    t = shift * (2.0 * step)
    ecoord = U * (np.abs(t) + np.abs(base + t)) * REF_SLACK
    delta, idx, slope = [], [], []
    for a, (size, full) in enumerate(((d["Wf"], d["W"]), (d["Hf"], d["H"]))):
        i = _sample_coords(ref["coord"][:, a], size, full, np.dtype(np.float64), None)
        delta.append(ecoord[:, a] * (size - 1) / (full - 1) + U * (3.0 * np.abs(i) + 0.5 * (size - 1)))
        idx.append(i)
    (ix, iy), (dx, dy) = idx, delta
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    wx1, wy1 = (ix - x0)[..., None], (iy - y0)[..., None]
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    f00, f01, f10, f11 = _fetch(feat, y0, x0), _fetch(feat, y0, x0 + 1), _fetch(feat, y0 + 1, x0), _fetch(feat, y0 + 1, x0 + 1)
    e1 = C1 * U * (np.abs(wx0 * wy0 * f00) + np.abs(wx1 * wy0 * f01) + np.abs(wx0 * wy1 * f10) + np.abs(wx1 * wy1 * f11))

    def slope_x(xp):
        return np.abs(wy0 * (_fetch(feat, y0, xp + 1) - _fetch(feat, y0, xp)) + wy1 * (_fetch(feat, y0 + 1, xp + 1) - _fetch(feat, y0 + 1, xp)))

    def slope_y(yp):
        return np.abs(wx0 * (_fetch(feat, yp + 1, x0) - _fetch(feat, yp, x0)) + wx1 * (_fetch(feat, yp + 1, x0 + 1) - _fetch(feat, yp, x0 + 1)))

    def widest(fn, i, i0, dl, size):
        """the slope in the reference's patch, and in a neighbour that the coordinate's error can reach; patches inside the map"""
        if size < 2:
            return np.zeros(f00.shape)
        last = size - 2
        s = fn(np.clip(i0, 0, last))
        below = ((i - i0) < dl) & (i0 - 1 >= 0)
        above = ((i0 + 1 - i) < dl) & (i0 + 1 <= last)
        s = np.where(below[..., None], np.maximum(s, fn(np.clip(i0 - 1, 0, last))), s)
        return np.where(above[..., None], np.maximum(s, fn(np.clip(i0 + 1, 0, last))), s)

    e2 = (dx[..., None] * widest(slope_x, ix, x0, dx, d["Wf"]) + dy[..., None] * widest(slope_y, iy, y0, dy, d["Hf"])
          + (dx * dy)[..., None] * np.abs(f00 - f01 - f10 + f11))
    ev = (e1 + e2).transpose(0, 3, 1, 2)
    v = (wx0 * wy0 * f00 + wx1 * wy0 * f01 + wx0 * wy1 * f10 + wx1 * wy1 * f11).transpose(0, 3, 1, 2)
    nv = np.sqrt((v * v).sum(1, keepdims=True))
    c4 = (C / 4 + 3) / 2.0 + 2.0
    with np.errstate(invalid="ignore", divide="ignore"):
        dref = v / nv
        bdesc = (ev / nv + np.abs(dref) * (np.sqrt((ev * ev).sum(1, keepdims=True)) / nv + c4 * U)) * SECOND_ORDER
    bdesc = np.where(nv > 0, bdesc, np.nan)
    return {"coord": ecoord, "desc": bdesc, "ref": ref, "ix": ix, "iy": iy}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _ratio(err, bound):
    """the largest err / bound; inf where the bound is 0 and the error is not"""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0


def evaluate_post(case, rec):
    """rec: dict(score, coord, desc, ids_dense, ids_samp [, guards, same]) of a device run or of emulate(case, float32[, mut])
    -> (one line of figures, the list of failures)"""
    c, d = POST_CASES[case], post_dims(case)
    inp, bd = post_inputs(case), post_bounds(case)
    ref = bd["ref"]
    bad = []
    if not np.array_equal(_bits(np.asarray(rec["score"], np.float32)), _bits(ref["score"].astype(np.float32))):
        bad.append("score differs from score * mask")
    coord = np.asarray(rec["coord"], np.float64)
    if c["regime"] == "grid":
        Ec = 0.0 if np.array_equal(coord, ref["coord"]) else INF
    else:
        Ec = _ratio(np.abs(coord - ref["coord"]), bd["coord"])
    if not Ec <= 1.0:
        bad.append(f"coord: {Ec:.3g} of the bound")
    desc = np.asarray(rec["desc"], np.float64)
    nan_ref = np.isnan(bd["desc"])
    if not np.array_equal(np.isnan(desc), nan_ref):
        bad.append(f"desc: NaN at {int(np.isnan(desc).sum())} elements, the reference at {int(nan_ref.sum())}")
    ok = ~nan_ref & ~np.isnan(desc)
    Ed = _ratio(np.abs(desc - ref["desc"])[ok], bd["desc"][ok])
    if not Ed <= 1.0:
        bad.append(f"desc: {Ed:.3g} of the bound")
    if not np.array_equal(np.asarray(rec["ids_dense"]), argmax_ids(inp["seg"])[:, None]):
        bad.append(f"dense class ids differ from numpy.argmax at {int((np.asarray(rec['ids_dense']) != argmax_ids(inp['seg'])[:, None]).sum())} pixels")
    # sampled ids: float64 nearest sampling at the record's own float32 coordinates
    c32 = np.asarray(rec["coord"], np.float32).astype(np.float64)
    f64 = np.dtype(np.float64)
    sx, sy = _sample_coords(c32[:, 0], d["Ws"], d["W"], f64, None), _sample_coords(c32[:, 1], d["Hs"], d["H"], f64, None)
    want = nearest_ids(inp["seg"].astype(np.float64), sx, sy)[:, None]
    if c["regime"] == "grid":
        out = np.zeros(want.shape, bool)
    else:
        near = lambda v: np.abs(v - np.floor(v) - 0.5) <= NEAR_HALF * U * (np.abs(v) + 1.0)
        out = (near(sx) | near(sy))[:, None]
    left = float(out.mean())
    wrong = int(((np.asarray(rec["ids_samp"]) != want) & ~out).sum())
    if left > MAX_LEFT_OUT:
        bad.append(f"sampled class ids: {left:.3f} of the cells left out (> {MAX_LEFT_OUT})")
    if wrong:
        bad.append(f"sampled class ids differ at {wrong} cells")
    if "guards" in rec and not bool(rec["guards"]):
        bad.append("a guard element changed")
    if "same" in rec and not bool(rec["same"]):
        bad.append("the launch with sampled ids and the launch with dense ids differ in score, coord or desc")
    line = (f"POST_SELECT post   {case:20s} argmax<{c['argmax']}> coord {Ec:.3f} desc {Ed:.3f} of the bound; NaN cells "
            f"{int(nan_ref[:, 0].sum())}; sampled ids left out {int(out.sum())} of {out.size}")
    return line, bad


# ---------------------------------------------------------------------------------------------------------------------
# top-k
# ---------------------------------------------------------------------------------------------------------------------
# (n, k, the form select_form.h must name at the default KP2D_TOPK_SMALL = 256)
TOPK_SHAPES = {
    "t256-300-100": (300, 100, "topk<256,kpow=128,cached,reg>"),
    "t256-2048-256": (2048, 256, "topk<256,kpow=256,cached,reg>"),
    "t256-2049-256": (2049, 256, "topk<256,kpow=256,uncached,reg>"),
    "t1024-300-257": (300, 257, "topk<1024,kpow=512,cached,reg>"),
    "t1024-8193-300": (8193, 300, "topk<1024,kpow=512,uncached,reg>"),
    "t1024-8192-3000": (8192, 3000, "topk<1024,kpow=4096,cached,loop>"),
    "t1024-8193-3000": (8193, 3000, "topk<1024,kpow=4096,uncached,loop>"),
    "t1024-8192-8192": (8192, 8192, "topk<1024,kpow=8192,cached,loop,optin>"),
    "t1024-17000-16384": (17000, 16384, "topk<1024,kpow=16384,uncached,loop,optin>"),      # the last k of the LDS path
    "tglobal-17000-16385": (17000, 16385, "topk<global>"),
}
# regime -> the thresholds it runs under
TOPK_REGIMES = {"ties": (0.7, -INF), "signed": (-INF, -0.5), "zeros": (-INF,), "equal": (-INF, 0.0), "special": (-INF, 0.0)}
# the forms behind KP2D_TOPK_SMALL: (n, k) -> the form per value
TOPK_KNOB_SHAPES = {
    "k-2000-1500": (2000, 1500, {4096: "topk<256,kpow=2048,cached,loop>", 64: "topk<1024,kpow=2048,cached,loop>"}),
    "k-4800-1000": (4800, 1000, {4096: "topk<256,kpow=1024,uncached,loop>", 64: "topk<1024,kpow=1024,cached,reg>"}),
    "k-19200-4096": (19200, 4096, {4096: "topk<256,kpow=4096,uncached,loop>", 64: "topk<1024,kpow=4096,uncached,loop>"}),
}
TOPK_KNOB_REGIMES = ("ties", "signed")
TOPK_MUTANTS = ("zero_order", "idx_desc", "nan_selected")


def topk_shape(shape):
    return (TOPK_SHAPES.get(shape) or TOPK_KNOB_SHAPES[shape])[:2]


def topk_cases(shapes=TOPK_SHAPES, regimes=TOPK_REGIMES):
    return [(s, r, t) for s in shapes for r in regimes for t in TOPK_REGIMES[r]]


def topk_id(shape, regime, thr):
    return f"{shape}-{regime}-thr{thr:g}"


def topk_scores(shape, regime, thr):
    """three frames [3, n] float32, the middle one without a candidate"""
    n, _ = topk_shape(shape)
    g = _rng(shape + regime)
    if regime == "ties":
        s = g.random((3, n)).astype(np.float32)
        s[:, ::7] = np.float32(0.75)            # many exact ties: the lowest index must win
    elif regime == "signed":
        s = g.standard_normal((3, n)).astype(np.float32)
    elif regime == "zeros":
        s = g.choice(np.array([0.0, -0.0], np.float32), (3, n))
        pos = g.random((3, n)) < 0.1
        s[pos] = g.random(int(pos.sum())).astype(np.float32)
    elif regime == "equal":
        s = np.full((3, n), 0.25, np.float32)
    else:
        s = g.standard_normal((3, n)).astype(np.float32)
        specials = np.array([INF, -INF, np.nan, 1e-40, -1e-40, 1.4e-45, -0.0], np.float32)
        hit = g.random((3, n)) < 0.15
        s[hit] = g.choice(specials, int(hit.sum()))
    s[1] = np.float32(thr)                       # s > thr is false: at the threshold itself, or -inf
    if regime == "special":
        s[1, ::2] = np.nan
    return s


def topk_reference(s, k, thr, mut=None):
    """one frame -> the selected indices in order.  Candidates s > thr; value descending with -0.0 == +0.0, index ascending."""
    with np.errstate(invalid="ignore"):
        cand = np.nonzero((s > np.float32(thr)) | (np.isnan(s) if mut == "nan_selected" else False))[0]
    v = s[cand].astype(np.float64) + 0.0                       # -0.0 + 0.0 = +0.0
    if mut == "zero_order":
        v = np.where((s[cand] == 0) & np.signbit(s[cand]), -1e-300, v)
    if mut == "nan_selected":
        v = np.where(np.isnan(v), INF, v)
    order = np.lexsort((-cand if mut == "idx_desc" else cand, -v))
    return cand[order][:min(k, len(s))]


def evaluate_topk(shape, regime, thr, rec):
    """rec: dict(idx [3, k], val [3, k], cnt [3] [, guards]) -> (line, failures)"""
    n, k = topk_shape(shape)
    s = topk_scores(shape, regime, thr)
    kk = min(k, n)
    bad, counts = [], []
    for b in range(3):
        order = topk_reference(s[b], k, thr)
        m = len(order)
        counts.append(m)
        if int(rec["cnt"][b]) != m:
            bad.append(f"frame {b}: count {int(rec['cnt'][b])}, the reference {m}")
            continue
        if not np.array_equal(rec["idx"][b, :m], order):
            first = int(np.nonzero(rec["idx"][b, :m] != order)[0][0])
            bad.append(f"frame {b}: idx differs from rank {first} on ({int(rec['idx'][b, first])} for {int(order[first])})")
        if not (np.all(rec["idx"][b, m:kk] == -1) and np.all(_bits(rec["val"][b, m:kk]) == 0)):
            bad.append(f"frame {b}: the rows past the count are not (-1, +0.0)")
        if not np.array_equal(_bits(rec["val"][b, :m]), _bits(s[b][order])):
            bad.append(f"frame {b}: val is not the score's own bits")
    if counts[1] != 0:
        bad.append("the middle frame is not empty")
    if "guards" in rec and not bool(rec["guards"]):
        bad.append("a guard element changed")
    return f"POST_SELECT top-k  {topk_id(shape, regime, thr):40s} counts {counts} equal: {not bad}", bad


# ---------------------------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------------------------
def _gc(B, C, n, k, form):
    return dict(B=B, C=C, n=n, k=k, form=form)


D_, L8, L8S = "gather<direct>", "gather<lds8,vcopy,vstore>", "gather<lds8,scopy,vstore>"
GATHER_CASES = {
    # ---- direct: few frames; k in {1, 2, 3, 7} ----
    "g-direct-k1": _gc(3, 32, 96, 1, D_), "g-direct-k2": _gc(3, 32, 96, 2, D_), "g-direct-k3": _gc(4, 64, 96, 3, D_),
    "g-direct-k7": _gc(3, 128, 35, 7, D_), "g-direct-300": _gc(2, 32, 1200, 300, D_),
    # ---- direct at many frames: C % 8 != 0 ----
    "g-direct-c36": _gc(32, 36, 117, 30, D_), "g-direct-c2": _gc(32, 2, 117, 117, D_),
    # ---- LDS, 8 planes: a scalar copy (n = 9 x 13), k = ceil(n / 8) and k = n, k = 7; C = 128 with 8 frames ----
    "g-lds8-117-k15": _gc(32, 32, 117, 15, L8S), "g-lds8-117-kn": _gc(32, 32, 117, 117, L8S), "g-lds8-48-k7": _gc(32, 32, 48, 7, L8),
    "g-lds8-c128": _gc(8, 128, 1200, 150, L8), "g-lds8-c128-b7": _gc(7, 128, 1200, 150, D_),
    "g-lds8-117-k14": _gc(32, 32, 117, 14, D_),                      # k * 8 < n: direct
    # ---- the byte limits: 8 planes to 2048 cells, 4 to 5120, 2 to 8192, then direct ----
    "g-lds8-2048": _gc(32, 32, 2048, 256, L8), "g-lds4-2049": _gc(32, 32, 2049, 2049, "gather<lds4,scopy,vstore,optin>"),
    "g-lds4-5120": _gc(32, 32, 5120, 640, "gather<lds4,vcopy,vstore,optin>"),
    "g-lds2-5121": _gc(32, 32, 5121, 641, "gather<lds2,scopy,sstore>"),
    "g-lds2-8192": _gc(32, 32, 8192, 1024, "gather<lds2,vcopy,sstore>"),
    "g-direct-8193": _gc(32, 32, 8193, 1025, D_),
}


def gather_lds_cases():
    return [c for c, g in GATHER_CASES.items() if g["form"] != D_]


@functools.lru_cache(maxsize=4)
def gather_inputs(case):
    """coord [B, 2, n], desc [B, C, n] float32, idx [B, k] int32: even frames from the top-k (padded with -1 past the count),
    odd frames hand-made: random cells with duplicates and -1 in the middle of the row"""
    c = GATHER_CASES[case]
    B, C, n, k = c["B"], c["C"], c["n"], c["k"]
    g = _rng(case)
    coord = (g.random((B, 2, n)) * 300).astype(np.float32)
    desc = g.standard_normal((B, C, n)).astype(np.float32)
    idx = np.full((B, k), -1, np.int32)
    for b in range(B):
        if b % 2 == 0:
            sel = topk_reference(g.random(n).astype(np.float32), k, 0.3 if b % 4 == 0 else -INF)
            idx[b, :len(sel)] = sel
        else:
            row = g.integers(0, n, k).astype(np.int32)
            row[g.random(k) < 0.2] = row[0]                    # duplicates
            row[g.random(k) < 0.1] = -1
            row[k // 2] = -1 if b % 4 == 1 else n - 1         # -1 in the middle of a row; the last cell
            idx[b] = row
    return {"coord": coord, "desc": desc, "idx": idx}


def evaluate_gather(case, rec, form=None):
    """rec: dict(pts [B, k, 2], dsel [B, k, C] [, guards]) -> (line, failures)"""
    inp = gather_inputs(case)
    idx = inp["idx"].astype(np.int64)
    live = (idx >= 0)[..., None]
    bi = np.arange(idx.shape[0])[:, None]
    safe = np.maximum(idx, 0)
    dsel = np.where(live, inp["desc"].transpose(0, 2, 1)[bi, safe], np.float32(0))
    pts = np.where(live, inp["coord"].transpose(0, 2, 1)[bi, safe], np.float32(0))
    bad = []
    if not np.array_equal(_bits(rec["dsel"]), _bits(dsel.astype(np.float32))):
        bad.append(f"descriptors differ at {int((_bits(rec['dsel']) != _bits(dsel.astype(np.float32))).sum())} elements")
    if not np.array_equal(_bits(rec["pts"]), _bits(pts.astype(np.float32))):
        bad.append(f"points differ at {int((_bits(rec['pts']) != _bits(pts.astype(np.float32))).sum())} elements")
    if "guards" in rec and not bool(rec["guards"]):
        bad.append("a guard element changed")
    return f"POST_SELECT gather {case:20s} {form or GATHER_CASES[case]['form']:34s} rows with -1: {int((~live).sum())} equal: {not bad}", bad


# ---------------------------------------------------------------------------------------------------------------------
# the VALU matcher from 256 train rows up (KP2D_MATCH_MFMA=0)
# ---------------------------------------------------------------------------------------------------------------------
MATCH_K0, MATCH_TILE, MATCH_RATIO, MATCH_NCLS = 400, 40, 0.7, 6
MATCH_CASES = {f"m-{k1}-c{C}-{mode}": dict(k1=k1, C=C, mode=mode) for k1 in (300, 1100) for C in (32, 128)
               for mode in ("ratio", "classes", "mutual")}
MATCH_KEYS = ("nn_idx", "nn_dist", "nn_dist2", "match_q", "match_d")


@functools.lru_cache(maxsize=2)
def match_inputs(case):
    """two pairs (test_gpu_parity.py's _match_problem): true correspondences with noise, exact duplicates among the queries"""
    c = MATCH_CASES[case]
    B, k0, k1, C, n_true = 2, MATCH_K0, c["k1"], c["C"], 150
    g = _rng(case)
    d0 = g.standard_normal((B, k0, C)).astype(np.float32)
    d1 = g.standard_normal((B, k1, C)).astype(np.float32)
    for b in range(B):
        src = g.permutation(k1)[:n_true]
        d0[b, :n_true] = d1[b, src] + 0.05 * g.standard_normal((n_true, C)).astype(np.float32)
        d0[b, n_true:n_true + 10] = d0[b, :10]
    d0 /= np.linalg.norm(d0, axis=-1, keepdims=True)
    d1 /= np.linalg.norm(d1, axis=-1, keepdims=True)
    c0 = g.integers(0, MATCH_NCLS, (B, k0)).astype(np.int32)
    c1 = g.integers(0, MATCH_NCLS, (B, k1)).astype(np.int32)
    for b in range(B):      # true correspondences share their class
        c0[b, :n_true] = c1[b, np.argmin(((d0[b, :n_true, None, :] - d1[b, None, :, :]) ** 2).sum(-1), axis=1)]
    return {"d0": d0, "d1": d1, "n0": np.array([k0, k0 - 83], np.int32), "n1": np.array([k1, k1 - 3], np.int32), "c0": c0, "c1": c1}


def _pairs_equal(got_q, ref, dd1=None, dd2=None):
    """test_gpu_parity.py's boundary rule: the pair sets may differ only where the ratio test sits on its fp32 boundary"""
    got = {int(t): int(q) for t, q in enumerate(got_q) if q >= 0}
    want = {t: q for t, (q, _) in ref.items()}
    bad = []
    for t in set(got) ^ set(want):
        q = got.get(t, want.get(t))
        if dd1 is None or not abs(dd1[q] - MATCH_RATIO * dd2[q]) < 1e-5:
            bad.append(f"train row {t}: query {got.get(t)} for {want.get(t)}")
    bad += [f"train row {t}: query {got[t]} for {want[t]}" for t in set(got) & set(want) if got[t] != want[t]]
    return len(got), bad


def evaluate_match(case, rec):
    """rec: the sliced run's MATCH_KEYS arrays and ``same`` (sliced == one slice, bit for bit) -> (line, failures)"""
    c, inp = MATCH_CASES[case], match_inputs(case)
    bad = [] if bool(rec["same"]) else ["the sliced and the one-slice search differ"]
    total = 0
    for b in range(2):
        n0, n1 = int(inp["n0"][b]), int(inp["n1"][b])
        d0, d1 = inp["d0"][b, :n0], inp["d1"][b, :n1]
        got_q = rec["match_q"][b]
        if c["mode"] == "mutual":
            n, bb = _pairs_equal(got_q, orc.bf_match_crosscheck(d0, d1))
        elif c["mode"] == "ratio":
            best, nn, dd1, dd2 = orc.bf_match_one_to_one(d0, d1, MATCH_RATIO)
            if not np.array_equal(rec["nn_idx"][b, :n0], nn):
                bad.append(f"pair {b}: nn_idx differs")
            if not np.max(np.abs(rec["nn_dist"][b, :n0] - dd1)) < 2e-5:
                bad.append(f"pair {b}: nn_dist differs")
            n, bb = _pairs_equal(got_q, best, dd1, dd2)
        else:
            c0, c1 = inp["c0"][b, :n0], inp["c1"][b, :n1]
            ref = orc.bf_match_semantic(d0, c0, d1, c1, MATCH_RATIO, n_classes=MATCH_NCLS)
            dd1, dd2 = np.full(n0, np.inf, np.float32), np.full(n0, np.inf, np.float32)
            for q in range(n0):
                same = np.where(c1 == c0[q])[0]
                dist = np.sort(np.sqrt(((d0[q] - d1[same]) ** 2).sum(-1, dtype=np.float32)))
                dd1[q], dd2[q] = dist[0], (dist[1] if len(dist) > 1 else np.inf)
            n, bb = _pairs_equal(got_q, ref, dd1, dd2)
            t = np.where(got_q >= 0)[0]
            if not np.all(inp["c1"][b][t] == inp["c0"][b][got_q[t]]):
                bad.append(f"pair {b}: a match across classes")
        if not np.all(got_q[n1:] == -1):
            bad.append(f"pair {b}: a match past the train count")
        bad += [f"pair {b}: {x}" for x in bb]
        total += n
    if total < 100:
        bad.append(f"only {total} matches: the problem does not exercise the matcher")
    return f"POST_SELECT match  {case:22s} VALU, sliced == one slice: {bool(rec['same'])}; {total} pairs as the oracle's: {not bad}", bad


# ---------------------------------------------------------------------------------------------------------------------
# the device side (this process, or a knob's child)
# ---------------------------------------------------------------------------------------------------------------------
class _Guarded:
    """an output inside a larger buffer filled with a sentinel"""

    def __init__(self, shape, dtype, dev):
        import torch
        self.n = int(np.prod(shape))
        self.sent = SENT_F if dtype.is_floating_point else SENT_I
        self.buf = torch.full((self.n + 2 * PAD,), self.sent, dtype=dtype, device=dev)
        self.view = self.buf[PAD:PAD + self.n].view(*shape)

    def intact(self):
        return bool((self.buf[:PAD] == self.sent).all()) and bool((self.buf[PAD + self.n:] == self.sent).all())


@functools.lru_cache(maxsize=None)
def _model(name, dev):
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import tiny_factory
    m = tiny_factory(MODELS[name][0], 28).to(dev).eval()      # no weights: kp2d_post reads the configuration only
    m.training = False
    return m


def device_post(case, dev="cuda:0"):
    import torch
    from nano_vs_slam_amd import _lib
    from nano_vs_slam_amd._dev import ptr, stream
    c, d, inp = POST_CASES[case], post_dims(case), post_inputs(case)
    model = _model(c["model"], dev)
    eng = model._get_engine(torch.device(dev), need_weights=False)
    score, shift, feat = (torch.from_numpy(inp[k]).to(dev) for k in ("score", "shift", "feat"))
    segbuf = torch.zeros(inp["seg"].size + 8, device=dev)
    seg = segbuf[c["seg_off"]:c["seg_off"] + inp["seg"].size].view(*inp["seg"].shape)      # seg_off = 1: 4 bytes past 16-byte alignment
    seg.copy_(torch.from_numpy(inp["seg"]))
    assert seg.data_ptr() % 16 == 4 * c["seg_off"]
    B, Hc, Wc = d["B"], d["Hc"], d["Wc"]
    runs = []
    for sample in (0, 1):
        o = {"score": _Guarded((B, 1, Hc, Wc), torch.float32, dev), "coord": _Guarded((B, 2, Hc, Wc), torch.float32, dev),
             "desc": _Guarded((B, d["C"], Hc, Wc), torch.float32, dev),
             "ids": _Guarded((B, 1, Hc, Wc) if sample else (B, 1, d["Hs"], d["Ws"]), torch.int64, dev)}
        _lib.check(eng.lib.kp2d_post(eng.handle, ptr(score), ptr(shift), ptr(feat), ptr(seg), B, d["H"], d["W"], Hc, Wc, d["C"],
                                     d["Hf"], d["Wf"], d["Cs"], d["Hs"], d["Ws"], ptr(o["score"].view), ptr(o["coord"].view),
                                     ptr(o["desc"].view), ptr(o["ids"].view), sample, stream(torch.device(dev))))
        torch.cuda.synchronize()
        runs.append(o)
    dense, samp = runs
    same = all(torch.equal(dense[k].view.view(torch.int32), samp[k].view.view(torch.int32)) for k in ("score", "coord", "desc"))
    rec = {k: dense[k].view.cpu().numpy() for k in ("score", "coord", "desc")}
    rec.update(ids_dense=dense["ids"].view.cpu().numpy(), ids_samp=samp["ids"].view.cpu().numpy(), same=np.array(same),
               guards=np.array(all(g.intact() for o in runs for g in o.values())))
    return rec


def device_topk(shape, regime, thr, dev="cuda:0"):
    import torch
    from nano_vs_slam_amd import _lib
    from nano_vs_slam_amd._dev import ptr, stream
    n, k = topk_shape(shape)
    kk = min(k, n)
    s = torch.from_numpy(topk_scores(shape, regime, thr)).to(dev)
    idx, val, cnt = _Guarded((3, kk), torch.int32, dev), _Guarded((3, kk), torch.float32, dev), _Guarded((3,), torch.int32, dev)
    _lib.check(_lib.load().kp2d_select_topk(ptr(s), 3, n, kk, float(thr), ptr(idx.view), ptr(val.view), ptr(cnt.view),
                                            stream(torch.device(dev))))
    torch.cuda.synchronize()
    return {"idx": idx.view.cpu().numpy(), "val": val.view.cpu().numpy(), "cnt": cnt.view.cpu().numpy(),
            "guards": np.array(idx.intact() and val.intact() and cnt.intact())}


def device_gather(case, dev="cuda:0"):
    import torch
    from nano_vs_slam_amd import _lib
    from nano_vs_slam_amd._dev import ptr, stream
    c, inp = GATHER_CASES[case], gather_inputs(case)
    coord, desc, idx = (torch.from_numpy(inp[k]).to(dev) for k in ("coord", "desc", "idx"))
    pts, dsel = _Guarded((c["B"], c["k"], 2), torch.float32, dev), _Guarded((c["B"], c["k"], c["C"]), torch.float32, dev)
    _lib.check(_lib.load().kp2d_gather_keypoints(ptr(coord), ptr(desc), ptr(idx), c["B"], c["C"], c["n"], c["k"], ptr(pts.view),
                                                 ptr(dsel.view), stream(torch.device(dev))))
    torch.cuda.synchronize()
    return {"pts": pts.view.cpu().numpy(), "dsel": dsel.view.cpu().numpy(), "guards": np.array(pts.intact() and dsel.intact())}


def device_match(case, dev="cuda:0"):
    """the case's two pairs as they are (few workgroups: the train range is sliced) and tiled MATCH_TILE times (one slice)"""
    import torch
    from nano_vs_slam_amd.matching import match_descriptors
    c, inp = MATCH_CASES[case], match_inputs(case)
    t = lambda a, rep=1: torch.from_numpy(np.tile(a, (rep,) + (1,) * (a.ndim - 1))).to(dev)
    kw = dict(mutual=True) if c["mode"] == "mutual" else {}
    cls = lambda rep: dict(cls0=t(inp["c0"], rep), cls1=t(inp["c1"], rep)) if c["mode"] == "classes" else {}
    run = lambda rep: match_descriptors(t(inp["d0"], rep), t(inp["n0"], rep), t(inp["d1"], rep), t(inp["n1"], rep), MATCH_RATIO, **cls(rep), **kw)
    r, rb = run(1), run(MATCH_TILE)
    torch.cuda.synchronize()
    same = True
    for k in MATCH_KEYS:
        for b in range(2):
            nq = int(inp["n0"][b]) if k.startswith("nn") else c["k1"]
            same &= torch.equal(r[k][b, :nq], rb[k][b, :nq]) and torch.equal(r[k][b, :nq], rb[k][2 * (MATCH_TILE - 1) + b, :nq])
    rec = {k: r[k].cpu().numpy() for k in MATCH_KEYS}
    rec["same"] = np.array(bool(same))
    return rec


# ---------------------------------------------------------------------------------------------------------------------
# a knob's child process: every case of the knob's forms -> one .npz
# ---------------------------------------------------------------------------------------------------------------------
FORMS = {"small4096": {"KP2D_TOPK_SMALL": "4096"}, "small64": {"KP2D_TOPK_SMALL": "64"}, "gather0": {"KP2D_GATHER_LDS": "0"},
         "valu": {"KP2D_MATCH_MFMA": "0"}}
KNOBS = ("KP2D_TOPK_SMALL", "KP2D_GATHER_LDS", "KP2D_MATCH_MFMA")


def form_cases(form):
    """the keys of a form's child: (kind, ...)"""
    if form.startswith("small"):
        return [("topk",) + c for c in topk_cases(TOPK_KNOB_SHAPES, TOPK_KNOB_REGIMES)]
    if form == "gather0":
        return [("gather", c) for c in gather_lds_cases()]
    return [("match", c) for c in MATCH_CASES]


def form_key(key):
    return "/".join(f"{v:g}" if isinstance(v, float) else str(v) for v in key)


def child_run(form, out_path):
    res = {}
    for key in form_cases(form):
        rec = {"topk": device_topk, "gather": device_gather, "match": device_match}[key[0]](*key[1:])
        for k, v in rec.items():
            res[f"{form_key(key)}/{k}"] = v
    np.savez(out_path, **res)


CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import post_select_ref as R
R.child_run(sys.argv[2], sys.argv[3])
"""


def child_env(form):
    """the parent's environment without any of the knobs, plus the form's setting"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(FORMS[form])
    return env


def unpack(z, key):
    pre = form_key(key) + "/"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
