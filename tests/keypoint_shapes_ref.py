"""Cases of the keypoint loss (nano_vs_slam_amd.keypoint_training.keypoint_loss, csrc/keypoint_train.hip) past one tile of its
scans, past 64 channels and at exact ties, with the functions that judge a run.  test_keypoint_shapes_cpu.py holds everything
here to itself without a device, test_gpu_keypoint_shapes.py holds the kernels to it.  The oracle is
keypoint_training_ref.keypoint_loss (float64 numpy, held to the reference's own forward by the five fixtures), imported; its
``stages`` are what the device keeps in its scratch.

* The geometry (geometry(case), restated from the kernels): kl_nearest and kl_target_grad tile the N cells by 256; kd_search
  walks 64 anchors per workgroup against 64 candidates at a time and the channels in chunks of 64 (kc: the width of the last
  chunk); the wave-per-anchor kernels take channel lane + 64 u in pass u; kd_feat_grad walks the anchors 256 at a time, a
  workgroup per 256 pixels of the descriptor map; kd_tar_grad collects a column's anchors by ballots over 64 anchors.
  pieces() restates make_plan's scratch walk.

      case   B, Hc x Wc, cell, C, Hf x Wf   N, n        what it reaches
      K1     2, 18 x 18, 4, 128, 36 x 36    324, 256    C = 128: two full chunks, u = 0 and 1; n = exactly four anchor tiles and
                                                        one kd_feat_grad pass; two pairs
      K2     1, 16 x 16, 4, 80, 16 x 16     256, 196    N = exactly one tile; kc = 16; Hf Wf = exactly one workgroup of kd_feat_grad
      K3     1, 20 x 30, 4, 256, 40 x 60    600, 504    three cell tiles (256, 256, 88); eight anchor tiles, the last of 56; two
                                                        kd_feat_grad passes; four chunks, every u
      K4     1, 32 x 33, 4, 32, 32 x 33     1056, 930   five cell tiles; fifteen anchor tiles; four kd_feat_grad passes; Hf = Hc
      K5     1, 16 x 32, 8, 16, 32 x 64     512, 420    N = exactly two tiles; cell 8
      K6     2, 12 x 14, 4, 80, 24 x 28     168, 120    pair 1 under the strong homography of case C: taps that leave both maps
                                                        with u = 1 lanes and a kc = 16 chunk
      S<C>   1, 10 x 10, 4, C, 20 x 20      100, 64     n = exactly one anchor tile; C in 48, 80, 112, 128, 144, 192, 208, 256 and
                                                        96: every chunk count 1..4 and every last-chunk width 16, 32 (96 alone),
                                                        48, 64

  Inputs are drawn as keypoint_training_ref.make_loss_inputs draws them; SEEDS holds, per case, the first seed of base,
  base + 1000, ... (at most 1000 tries) at which keypoint_training_ref.conditions accepts the float64 oracle against its
  float32 run: every discrete choice safe by 100 x that quantity's own float32 error (find_seed; the CPU module asserts the
  conditions for the constants kept here).
* The placed cases stand on arithmetic that is exact in float32 and float64: cell 5 (step 2, reach 4), shifts on a grid of
  1 / 256, the identity homography, a frame and a descriptor map of 129 x 129 ((W - 1) / 2 = 64), so that a pixel coordinate
  of the map IS the cell's coordinate; 12 x 25 cells (N = 300, n = 230), C = 16.
    Ta        target cells 255 and 256 (row 10, columns 5 and 6) decode to the one point (30, 53): 27 + 0.75 * 4 and
              32 - 0.5 * 4; the source's cell 255 lands next to it: a tie of a_i across the tile boundary at 256.
    Tb<k1>-<k2>  the source cells of anchors k1 and k2 have shift 0 and so sample one pixel each with weight exactly 1; both
              pixels of the target map hold one vector u, the rest of it is noise, the source map is u plus small noise
              everywhere.  The two tar rows are bit-identical, every anchor's nearest column is the tied pair, its negative is
              k1 outside the relax field of k1 and k2 inside it (and outside that of k2).  k2 = 6: the same lane, the next
              register; 9: another lane group; 21: another 16-row product tile; 69: another candidate tile; 229: the ragged
              last tile.  In all five the lane group of k1 = 5 (group 1) is not above that of k2, and the lane that writes the
              result (group 0) then keeps the lower index even under a plain "<" in take_lower: measured, that mutation of the
              kernel passes them.  Tb5-16 (16: group 0 of the next product tile, met by the xor-16 exchange) and Tb13-16
              (13: group 3, met by the xor-32 exchange after group 2 took it) put the lower index in the HIGHER group.  The same cases make k1 the negative of most anchors: several set bits per ballot in every ballot
              chunk of kd_tar_grad (check_placed asserts at least 65 active ones, in at least three chunks).
  The oracle forms these cases' products elementwise (blas=False); check_placed asserts the construction on the oracle.
* Error measure and bounds: E as test_gpu_keypoint_training.py defines it (an array: max|G - G64| / max|G64|; a scalar:
  relative; usp and a pair's sum S (d - mean): against the summands' magnitudes).  The bound of a quantity of a case is
  max(8 x the error of the oracle's own float32 run of that case against its float64 run, 16 x 2^-24); of a placed case
  16 x 2^-24 alone.  Nothing of a bound comes from the device.
  The one exception: dfeat_t and dfeat_s of the tied cases, whose bound is max(8 x the error of device_order32, a float32
  numpy restatement of the device's own order, 16 x 2^-24): 1.1e-4 to 1.6e-4 for dfeat_t, 1.0e-5 to 1.7e-5 for dfeat_s.
* evaluate(case, got) is what both test modules call; emulate(case, mut) forms, by numpy on the oracle's float32 data, what a
  wrong walk would leave in the scratch and the outputs (MUTANTS); none is undetected.
"""
import functools

import numpy as np

import keypoint_training_ref as kr
from loss_shapes_ref import ALIGN, carve, carve_offsets          # noqa: F401

FLOOR = kr.FLOOR
TILE_CELLS, TILE_ANCHORS, CHUNK, PASS, BALLOT = 256, 64, 64, 256, 64

SWEEP = (48, 80, 112, 128, 144, 192, 208, 256)
SHAPES = {"K1": (2, 18, 18, 4, 128, 36, 36), "K2": (1, 16, 16, 4, 80, 16, 16), "K3": (1, 20, 30, 4, 256, 40, 60),
          "K4": (1, 32, 33, 4, 32, 32, 33), "K5": (1, 16, 32, 8, 16, 32, 64), "K6": (2, 12, 14, 4, 80, 24, 28)}
SHAPES.update({f"S{c}": (1, 10, 10, 4, c, 20, 20) for c in SWEEP + (96,)})        # 96: the last-chunk width 32, which SWEEP lacks
STRONG = {"K6": (1,)}
DRAWN = tuple(SHAPES)
T_SHAPE = (1, 12, 25, 5, 16, 129, 129)
T_SIZE = 129
TIES = ((5, 6), (5, 9), (5, 21), (5, 69), (5, 229))
# the lower index in a HIGHER lane group than the higher one: the only ties at which the merge across lane groups decides
LANE_TIES = ((5, 16), (13, 16))
PLACED = ("Ta",) + tuple(f"Tb{a}-{b}" for a, b in TIES + LANE_TIES)
CASES = DRAWN + PLACED
_LATE = ["S96", "Tb5-16", "Tb13-16"]          # added after the others had their base seeds
BASE_SEED = {name: 601 + i for i, name in enumerate([c for c in CASES if c not in _LATE] + _LATE)}
# find_seed(name) of every case (python3 tests/keypoint_shapes_ref.py prints them)
SEEDS = {"K1": 6601, "K2": 602, "K3": 31603, "K4": 484604, "K5": 9605, "K6": 606, "S48": 607, "S80": 608, "S112": 1609, "S128": 1610,
         "S144": 611, "S192": 612, "S208": 1613, "S256": 614, "Ta": 17615, "Tb5-6": 3616, "Tb5-9": 4617, "Tb5-21": 6618, "Tb5-69": 2619,
         "Tb5-229": 1620, "S96": 621, "Tb5-16": 3622, "Tb13-16": 22623}
TRIES = {"K1": 7, "K3": 32, "K4": 485, "K5": 10, "Ta": 18, "Tb13-16": 23}          # the cases that took more than a handful of seeds

QUANTITIES = kr.LOSS_KEYS + ("d", "hinge", "r", "t", "fsum0", "fsum1", "fsum2", "fsum3", "fsum4")
MUTANTS = ("first_chunk_products", "stale_anchor_chunk", "first_pass_rows", "no_ragged_cell_tile", "higher_index_a", "higher_index_neg", "plain_less_merge",
           "first_feat_pass", "first_ballot_chunk", "one_bit_per_ballot")
UNDETECTED = ()
# the smallest cases that can show each
MUTANT_CASES = {"first_chunk_products": ("S80",), "stale_anchor_chunk": ("K6",), "first_pass_rows": ("S80",), "no_ragged_cell_tile": ("K3",),
                "higher_index_a": ("Ta",), "higher_index_neg": ("Tb5-6", "Tb5-229"), "plain_less_merge": ("Tb5-16", "Tb13-16"),
                "first_feat_pass": ("K3",),
                "first_ballot_chunk": ("Tb5-6",), "one_bit_per_ballot": ("Tb5-6",)}


def shape_of(case):
    return SHAPES[case] if case in SHAPES else T_SHAPE


def tie_of(case):
    k1, k2 = case[2:].split("-")
    return int(k1), int(k2)


def geometry(case):
    B, Hc, Wc, cell, C, Hf, Wf = shape_of(case)
    N, n = Hc * Wc, (Hc - 2) * (Wc - 2)
    up = lambda a, b: -(-a // b)
    return dict(N=N, n=n, cell_tiles=up(N, TILE_CELLS), last_cell_tile=N - (up(N, TILE_CELLS) - 1) * TILE_CELLS,
                anchor_tiles=up(n, TILE_ANCHORS), last_anchor_tile=n - (up(n, TILE_ANCHORS) - 1) * TILE_ANCHORS, chunks=up(C, CHUNK),
                kc=C - (up(C, CHUNK) - 1) * CHUNK, passes=up(n, PASS), ballots=up(n, BALLOT), feat_groups=up(Hf * Wf, 256))


def pieces(B, Hc, Wc, C):
    """make_plan's walk as (count, itemsize): ct, cs, wn, w (float2), jac (float4), d, a, diff, send (float4), fsum (double
    [B][6]), fcnt (int64 [B][2]), coef (double [8]), xr, xt, r, t, gr, gt (float [B][n][C]), neg, hit, cp, cn, hinge [B][n]."""
    N, n = Hc * Wc, (Hc - 2) * (Wc - 2) if Hc > 2 and Wc > 2 else 0
    BN, Bn = B * N, B * (n if n >= kr.MIN_ANCHORS else 0)
    return ([(BN, 8)] * 4 + [(BN, 16), (BN, 4), (BN, 4), (BN, 4), (BN, 16), (B * 6, 8), (B * 2, 8), (8, 8)] + [(Bn * C, 4)] * 6 + [(Bn, 4)] * 5)


PIECE_NAMES = ("ct", "cs", "wn", "w", "jac", "d", "a", "diff", "send", "fsum", "fcnt", "coef", "xr", "xt", "r", "t", "gr", "gt",
               "neg", "hit", "cp", "cn", "hinge")
PIECE_DTYPES = dict(ct=np.float32, cs=np.float32, wn=np.float32, w=np.float32, jac=np.float32, d=np.float32, a=np.int32, diff=np.float32,
                    send=np.float32, fsum=np.float64, fcnt=np.int64, coef=np.float64, xr=np.float32, xt=np.float32, r=np.float32,
                    t=np.float32, gr=np.float32, gt=np.float32, neg=np.int32, hit=np.int32, cp=np.float32, cn=np.float32, hinge=np.float32)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def anchor_yx(k, Wc):
    return k // (Wc - 2) + 1, k % (Wc - 2) + 1


def _placed_base(seed):
    """Drawn maps on exact coordinates: shifts on a grid of 1 / 256, the identity, a 129 x 129 frame."""
    B = T_SHAPE[0]
    inp = kr.draw_loss_inputs(T_SHAPE + (kr.WEIGHTS,), seed)
    inp.update(H=T_SIZE, W=T_SIZE, hom=np.eye(3, dtype=np.float32)[None].repeat(B, 0))
    for view in ("tgt", "src"):
        inp[view]["shift"] = (np.round(inp[view]["shift"] * 256.0) / 256.0).astype(np.float32)
    return inp


def make_inputs(case, seed):
    if case in SHAPES:
        return kr.draw_loss_inputs(SHAPES[case] + (kr.WEIGHTS,), seed, strong=STRONG.get(case, ()))
    inp = _placed_base(seed)
    Wc, C = T_SHAPE[2], T_SHAPE[4]
    if case == "Ta":
        inp["tgt"]["shift"][0, 0, 10, 5], inp["tgt"]["shift"][0, 0, 10, 6] = 0.75, -0.5
        inp["tgt"]["shift"][0, 1, 10, 5] = inp["tgt"]["shift"][0, 1, 10, 6] = 0.25
        inp["src"]["shift"][0, :, 10, 5] = np.asarray([0.8125, 0.3125], np.float32)
        return inp
    rng = np.random.default_rng(seed + 7)
    u = rng.standard_normal(C).astype(np.float32)
    ft = rng.standard_normal(inp["tgt"]["feat"].shape).astype(np.float32)
    for k in tie_of(case):
        y, x = anchor_yx(k, Wc)
        inp["src"]["shift"][0, :, y, x] = 0.0
        ft[0, :, 5 * y + 2, 5 * x + 2] = u
    inp["tgt"]["feat"] = ft
    inp["src"]["feat"] = (u[None, :, None, None] + np.float32(0.05) * rng.standard_normal(ft.shape).astype(np.float32)).astype(np.float32)
    return inp


def _run(case, inp, dtype, grads=True):
    return kr.keypoint_loss(inp["tgt"], inp["src"], inp["hom"], inp["H"], inp["W"], inp["cell"], inp["weights"], dtype=dtype, grads=grads,
                            blas=not case.startswith("Tb"))


def _within(o, b=0):
    """bool [n, n]: the relax field, from the oracle's warped coordinates (the placed cases' 12 x 25 cells)."""
    inner = kr.interior_mask(*T_SHAPE[1:3]).ravel()
    kx, ky = o["q"]["w"][0][b][inner], o["q"]["w"][1][b][inner]
    return (np.abs(kx[None, :] - kx[:, None]) <= kr.RELAX) & (np.abs(ky[None, :] - ky[:, None]) <= kr.RELAX)


def exemptions(case, o64):
    """The placed ties, whose own gap is 0 on purpose."""
    if case == "Ta":
        m = np.zeros(o64["a"].shape, bool)
        m[0, 255] = True
        return {"a": m}
    if case.startswith("Tb"):
        k1, k2 = tie_of(case)
        w = _within(o64)
        return {"neg": [~w[:, k1] & ~w[:, k2]]}
    return None


def check_placed(case, o64):
    """-> None, or what of the construction does not hold on the oracle."""
    if case == "Ta":
        u = o64["q"]["u"]
        if not (u[0, 0, 255] == u[0, 0, 256] == 30.0 and u[1, 0, 255] == u[1, 0, 256] == 53.0):
            return "cells 255 and 256 do not decode to (30, 53)"
        if not (o64["a"][0, 255] == 255 and o64["valid"][0, 255] and o64["d"][0, 255] < 0.5):
            return "the source's cell 255 does not take 255"
        return None
    k1, k2 = tie_of(case)
    p, dmat, w = o64["stages"]["pairs"][0], o64["q"]["dmat"][0], _within(o64)
    if not (np.array_equal(p["t"][k1].view(np.uint64), p["t"][k2].view(np.uint64)) and np.array_equal(dmat[:, k1].view(np.uint64), dmat[:, k2].view(np.uint64))):
        return "the tied columns are not equal bit for bit"
    if not (p["best"] == k1).all():
        return "an anchor's nearest column is not k1"
    if w[k1, k2] or not (p["neg"][~w[:, k1]] == k1).all() or not (p["neg"][w[:, k1] & ~w[:, k2]] == k2).all() or p["neg"][k1] != k2:
        return "the negatives are not k1 outside its field and k2 inside it"
    mine = np.flatnonzero((p["neg"] == k1) & (p["cn"] != 0))
    per = np.bincount(mine // BALLOT, minlength=4)
    if not (mine.size >= 65 and (per > 0).sum() >= 3 and per.max() >= 2):
        return f"k1 is the negative of {mine.size} active anchors, per ballot chunk {per.tolist()}"
    return None


def refusal(case, seed):
    """-> None, or the reason the seed is refused (keypoint_training_ref.conditions, and the construction of a placed case)."""
    inp = make_inputs(case, seed)
    o64, o32 = _run(case, inp, np.float64, grads=case in PLACED), _run(case, inp, np.float32, grads=False)
    return (check_placed(case, o64) if case in PLACED else None) or kr.conditions(o64, o32, exemptions(case, o64))


def find_seed(case):
    seed = BASE_SEED[case]
    for tries in range(1000):
        why = refusal(case, seed)
        if why is None:
            return seed, tries + 1
        seed += 1000
    raise SystemExit(f"case {case}: 1000 seeds refused")


@functools.lru_cache(maxsize=None)
def inputs(case):
    inp = make_inputs(case, SEEDS[case])
    for view in ("tgt", "src"):
        for v in inp[view].values():
            v.setflags(write=False)
    inp["hom"].setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def oracle(case, dtype=np.float64):
    """The oracle's run of the case, computed once and shared: nobody writes to it."""
    return _run(case, inputs(case), dtype)


# ---- what a run leaves: one layout for the device, the oracle and the wrong walks -------------------------------------------------
def as_got(o):
    """The oracle's result in the layout evaluate takes: counts (M, n, hits), fcnt [B, 2], a [B, N], d [B, N], neg, hit, hinge
    [B, n], r, t [B, n, C], fsum [B, 5], loss, parts [4], the six gradients."""
    st = o["stages"]
    B = o["a"].shape[0]
    got = {"counts": (o["M"], o["n"], o["hits"]), "a": o["a"], "d": o["d"], "fsum": st["fsum"], "loss": o["loss"],
           "parts": np.asarray([o[k] for k in kr.PARTS]), **{k: o[k] for k in kr.GRADS}}
    pairs = st["pairs"]
    hits_b = [int(p["hit"].sum()) for p in pairs] if pairs else [0] * B
    got["fcnt"] = np.stack([st["M_b"], hits_b], axis=1).astype(np.int64)
    for k in ("neg", "hit", "hinge", "r", "t"):
        got[k] = np.stack([np.asarray(p[k]) for p in pairs])
    return got


def _scalar(v, v64, scale=None):
    scale = abs(v64) if scale is None else scale
    diff = abs(float(v) - float(v64))
    return diff / scale if scale > 0 else (0.0 if diff == 0 else np.inf)


def errors(case, got):
    """-> {quantity: E} of what ``got`` holds, against the float64 oracle."""
    ref, o = as_got(oracle(case)), oracle(case)
    out = {}
    if "loss" in got:
        out["loss"] = _scalar(got["loss"], ref["loss"])
    if "parts" in got:
        for i, k in enumerate(kr.PARTS):
            out[k] = _scalar(got["parts"][i], ref["parts"][i], o["usp_abs"] if k == "usp" else None)
    for k in kr.GRADS + ("d", "hinge", "r", "t"):
        if k in got:
            want = np.asarray(ref[k], np.float64)
            g = np.asarray(got[k], np.float64).reshape(want.shape)
            scale, diff = np.abs(want).max(), np.abs(g - want).max()
            out[k] = diff / scale if scale > 0 else (0.0 if diff == 0 else np.inf)
    if "fsum" in got:
        f, usp_abs = np.asarray(got["fsum"], np.float64), o["stages"]["usp_abs_b"]
        for i in range(5):
            out[f"fsum{i}"] = max(_scalar(f[b, i], ref["fsum"][b, i], usp_abs[b] if i == 3 else None) for b in range(f.shape[0]))
    return out


@functools.lru_cache(maxsize=None)
def own_errors(case):
    """The oracle's float32 run of the case against its float64 run."""
    return errors(case, as_got(oracle(case, np.float32)))


@functools.lru_cache(maxsize=None)
def device_order32(case):
    """The descriptor term's gradient restated in numpy in the device's own order and precision, on the oracle's decisions:
    kd_sample (float32 taps, the norm in float64, the row times a float32 reciprocal), kd_hinge (float32 differences, float64
    norms, float32 coefficients), kd_tar_grad (a column's own anchor, then its anchors in ascending order, float32),
    kd_norm_back (float64 from the stored float32 rows, rounded once) and kd_feat_grad (a pixel's anchors in ascending order,
    float32) -> dict(dfeat_t, dfeat_s, r, t, hinge).  What it is for: in the tied cases one column is the negative of some
    225 anchors and sums as many largely cancelling float32 differences r_q - t; dfeat_t then misses 16 x 2^-24 by a factor
    11 to 21 on the device, and this restatement gives the device's error to three digits (2.01e-05 for 2.00e-05 on Tb5-6):
    the excess is rounding in the order the header documents.  On Ta it stays below 16 x 2^-24 like the device."""
    f, d64 = np.float32, np.float64
    inp, o = inputs(case), oracle(case, np.float32)
    B, Hc, Wc, cell, C, Hf, Wf = shape_of(case)
    n = (Hc - 2) * (Wc - 2)
    lw, dw, sw, kw = inp["weights"]
    scale, eps8, eps6, margin = f(kw * dw * 2.0 / (B * n)), f(1e-8), f(1e-6), d64(f(kr.MARGIN))
    out = {k: np.zeros((B, C, Hf, Wf), f) for k in ("dfeat_t", "dfeat_s")}
    out.update(r=np.zeros((B, n, C), f), t=np.zeros((B, n, C), f), hinge=np.zeros((B, n), f))

    def rows(feat, pts):
        x = np.zeros((C, n), f)
        for yy, xx, w, inside in kr._taps(pts[0], pts[1], Hf, Wf):
            x = x + np.where(inside, feat[:, yy, xx], f(0)) * w
        sq = ((x.astype(d64) + d64(eps8)) ** 2).sum(0)
        return x, x * (1.0 / (np.sqrt(sq) + d64(eps8))).astype(f)

    def back(g, x):
        g, x = g.astype(d64), x.astype(d64)
        s = np.sqrt(((x + d64(eps8)) ** 2).sum(0))
        D = s + d64(eps8)
        return (g / D - (g * x).sum(0) / (D * D * s) * (x + d64(eps8))).astype(f)

    for b, p in enumerate(o["stages"]["pairs"]):
        (xr, r), (xt, t) = rows(np.asarray(inp["src"]["feat"][b]), p["pts"][0]), rows(np.asarray(inp["tgt"]["feat"][b]), p["pts"][1])
        neg = p["neg"]
        ep, en = (r - t) + eps6, (r - t[:, neg]) + eps6
        dp, dn = np.sqrt((ep.astype(d64) ** 2).sum(0)), np.sqrt((en.astype(d64) ** 2).sum(0))
        h = np.maximum((margin + dp) - dn, 0.0).astype(f)
        cp = np.where((h > 0) & (dp > 0), d64(scale) / np.where(dp > 0, dp, 1), 0).astype(f)
        cn = np.where((h > 0) & (dn > 0), d64(scale) / np.where(dn > 0, dn, 1), 0).astype(f)
        gr, gt = cp * ep - cn * en, -cp * ((r - t) + eps6)
        for q in np.flatnonzero(cn != 0):
            gt[:, neg[q]] = gt[:, neg[q]] + cn[q] * ((r[:, q] - t[:, neg[q]]) + eps6)
        for key, g, pts in (("dfeat_s", back(gr, xr), p["pts"][0]), ("dfeat_t", back(gt, xt), p["pts"][1])):
            taps = kr._taps(pts[0], pts[1], Hf, Wf)
            for q in range(n):
                for yy, xx, w, inside in taps:
                    if inside[q]:
                        out[key][b, :, yy[q], xx[q]] = out[key][b, :, yy[q], xx[q]] + g[:, q] * w[q]
        out["r"][b], out["t"][b], out["hinge"][b] = r.T, t.T, h
    assert all(v.dtype == f for v in out.values())
    return out


WIDENED = ("dfeat_t", "dfeat_s")


@functools.lru_cache(maxsize=None)
def bounds(case):
    """Per quantity of the case.  A drawn case: max(8 x the oracle's own float32 error, 16 x 2^-24); a placed case: 16 x 2^-24
    alone, but for dfeat of the tied cases, where the device's own order restated in float32 (device_order32) misses the
    floor by rounding alone: max(8 x that restatement's error, 16 x 2^-24)."""
    if case in PLACED:
        b = {k: FLOOR for k in QUANTITIES}
        if case.startswith("Tb"):
            e = errors(case, device_order32(case))
            b.update({k: max(8.0 * e[k], FLOOR) for k in WIDENED})
        return b
    return {k: max(8.0 * e, FLOOR) for k, e in own_errors(case).items()}


@functools.lru_cache(maxsize=None)
def touched(case):
    """bool [B, Hf, Wf] per view (target, source): the pixels of the descriptor maps that a tap of an anchor falls on, in the
    oracle's float64 or float32 run; every other pixel's gradient is exactly 0."""
    B, Hc, Wc, cell, C, Hf, Wf = shape_of(case)
    masks = np.zeros((2, B, Hf, Wf), bool)
    for dtype in (np.float64, np.float32):
        for b, p in enumerate(oracle(case, dtype)["stages"]["pairs"]):
            for view, pts in ((1, p["pts"][0]), (0, p["pts"][1])):
                for yy, xx, _, inside in kr._taps(pts[0], pts[1], Hf, Wf):
                    masks[view, b, yy[inside], xx[inside]] = True
    return masks


def _first(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def evaluate(case, got):
    """What test_gpu_keypoint_shapes.py asks of a device run and test_keypoint_shapes_cpu.py of a wrong walk -> (failures,
    {quantity: E / bound})."""
    o = oracle(case)
    ref, fails, ratios = as_got(o), [], {}
    if tuple(int(v) for v in got["counts"]) != tuple(ref["counts"]):
        fails.append(f"counts {tuple(int(v) for v in got['counts'])}, not {tuple(ref['counts'])}")
    if not np.array_equal(np.asarray(got["fcnt"]), ref["fcnt"]):
        fails.append(f"fcnt {np.asarray(got['fcnt']).tolist()}, not {ref['fcnt'].tolist()}")
    bad = (np.asarray(got["a"]) != ref["a"]) & o["valid"]
    if bad.any():
        fails.append(f"a differs on {int(bad.sum())} valid cells, first at (pair, cell) {_first(bad)}")
    for k in ("neg", "hit"):
        bad = np.asarray(got[k]).astype(np.int64) != np.asarray(ref[k]).astype(np.int64)
        if bad.any():
            fails.append(f"{k} differs on {int(bad.sum())} anchors, first at (pair, anchor) {_first(bad)}")
    b = bounds(case)
    for k, e in errors(case, got).items():
        ratios[k] = e / b[k]
        if not e <= b[k]:
            fails.append(f"{k}: E {e:.3e} above its bound {b[k]:.3e}")
    mask = touched(case)
    for view, k in ((0, "dfeat_t"), (1, "dfeat_s")):
        stray = np.asarray(got[k]).any(axis=1) & ~mask[view]
        if stray.any():
            fails.append(f"{k} is not exactly 0 at {int(stray.sum())} pixels no tap touches, first at (pair, y, x) {_first(stray)}")
    inner = kr.interior_mask(*shape_of(case)[1:3])
    for k in ("dscore_t", "dscore_s"):
        if np.asarray(got[k])[:, 0][:, ~inner].any():
            fails.append(f"{k} is not exactly 0 on the border ring")
    return fails, ratios


# ---- the ways the walk could be wrong ------------------------------------------------------------------------------------------
def _search(dmat, within, kx, ky, higher=False):
    """best, neg and hit from a distance matrix; higher: the higher index among equal values."""
    n = dmat.shape[0]
    arg = (lambda m: n - 1 - m[:, ::-1].argmin(axis=1)) if higher else (lambda m: m.argmin(axis=1))
    best = arg(dmat)
    neg = np.where(within.all(axis=1), best, arg(np.where(within, np.inf, dmat)))
    return best, neg, (kx[best] == kx) & (ky[best] == ky)


def _search_plain_less(dmat, within, kx, ky):
    """kd_search with take_lower as a plain "<": a lane group (candidates j with j % 16 / 4 == group) keeps its lowest index
    among equal values, the exchanges (group 0 with 1 and 2 with 3, then 0 with 2) keep the lane's own value at a tie, and
    group 0 writes."""
    n = dmat.shape[0]
    grp = np.arange(n) % 16 // 4

    def merged(m):
        v = np.stack([np.where(grp[None, :] == g, m, np.inf).min(axis=1) for g in range(4)])
        j = np.stack([np.where(grp[None, :] == g, m, np.inf).argmin(axis=1) for g in range(4)])
        pick = lambda a, b: (np.where(v[b] < v[a], v[b], v[a]), np.where(v[b] < v[a], j[b], j[a]))
        (v[0], j[0]), (v[2], j[2]) = pick(0, 1), pick(2, 3)
        return pick(0, 2)

    (_, best), (nv, neg) = merged(dmat), merged(np.where(within, np.inf, dmat))
    return best, np.where(np.isfinite(nv), neg, best), (kx[best] == kx) & (ky[best] == ky)


def _dmat(dots):
    f = dots.dtype.type
    return np.sqrt(f(2) - f(2) * np.clip(dots, -1, 1) + f(1e-8))


def _feat_grads(o, b, g_ref, g_tar, anchors=None):
    """Back through the normalisation and the sampling; anchors: the ones kd_feat_grad reaches."""
    p = o["stages"]["pairs"][b]
    shape = o["dfeat_t"].shape[1:]
    keep = slice(None) if anchors is None else anchors
    gs, gt = kr.norm_back(g_ref, p["xr"], p["sr"])[:, keep], kr.norm_back(g_tar, p["xt"], p["st"])[:, keep]
    return (kr.sample_backward(gt, p["pts"][1][0][keep], p["pts"][1][1][keep], shape),
            kr.sample_backward(gs, p["pts"][0][0][keep], p["pts"][0][1][keep], shape))


def emulate(case, mut=None):
    """What the wrong walk ``mut`` leaves, formed by numpy from the oracle's float32 run of the case; None: that run itself."""
    assert mut is None or mut in MUTANTS
    o = oracle(case, np.float32)
    got = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in as_got(o).items()}
    if mut is None:
        return got
    B, Hc, Wc, cell, C, Hf, Wf = shape_of(case)
    inner = kr.interior_mask(Hc, Wc).ravel()
    for b, p in enumerate(o["stages"]["pairs"]):
        kx, ky = o["q"]["w"][0][b][inner], o["q"]["w"][1][b][inner]
        within = (np.abs(kx[None, :] - kx[:, None]) <= np.float32(kr.RELAX)) & (np.abs(ky[None, :] - ky[:, None]) <= np.float32(kr.RELAX))
        r, t, n = p["r"], p["t"], p["r"].shape[0]
        if mut == "first_chunk_products":
            _, got["neg"][b], got["hit"][b] = _search(_dmat(r[:, :CHUNK] @ t[:, :CHUNK].T), within, kx, ky)
        elif mut == "stale_anchor_chunk":
            # LDS keeps what candidate tile 0 left: the last chunk's columns over those of the chunk before it
            chunks, kc = geometry(case)["chunks"], geometry(case)["kc"]
            stale = np.zeros((n, CHUNK), r.dtype)
            for ch in range(chunks):
                w = min(CHUNK, C - CHUNK * ch)
                stale[:, :w] = r[:, CHUNK * ch:CHUNK * ch + w]
            dots = r @ t.T
            wrong = sum(stale[:, :min(CHUNK, C - CHUNK * ch)] @ t[:, CHUNK * ch:CHUNK * (ch + 1)].T for ch in range(chunks))
            dots[:, TILE_ANCHORS:] = wrong[:, TILE_ANCHORS:]
            _, got["neg"][b], got["hit"][b] = _search(_dmat(dots), within, kx, ky)
        elif mut == "first_pass_rows":
            for key, x in (("r", p["xr"]), ("t", p["xt"])):
                x = np.where(np.arange(C)[:, None] < CHUNK, x, 0)
                got[key][b] = (x / (np.sqrt(((x[:CHUNK] + np.float32(1e-8)) ** 2).sum(0)) + np.float32(1e-8))).T
        elif mut == "higher_index_neg":
            dots = (r[:, None, :] * t[None, :, :]).sum(axis=2)
            _, got["neg"][b], got["hit"][b] = _search(_dmat(dots), within, kx, ky, higher=True)
        elif mut == "plain_less_merge":
            dots = (r[:, None, :] * t[None, :, :]).sum(axis=2)
            _, got["neg"][b], got["hit"][b] = _search_plain_less(_dmat(dots), within, kx, ky)
        elif mut == "first_feat_pass":
            g_tar = -p["g_pos"].copy()
            np.add.at(g_tar.T, p["neg"], p["g_neg"].T)
            got["dfeat_t"][b], got["dfeat_s"][b] = _feat_grads(o, b, p["g_pos"] - p["g_neg"], g_tar, slice(0, PASS))
        elif mut in ("first_ballot_chunk", "one_bit_per_ballot"):
            g_tar = -p["g_pos"].copy()
            i = np.flatnonzero(p["cn"] != 0)
            if mut == "first_ballot_chunk":
                i = i[i < BALLOT]
            else:                   # per ballot chunk and column the lowest set bit only
                _, first = np.unique(np.stack([i // BALLOT, p["neg"][i]]), axis=1, return_index=True)
                i = i[np.sort(first)]
            np.add.at(g_tar.T, p["neg"][i], p["g_neg"].T[i])
            got["dfeat_t"][b], _ = _feat_grads(o, b, p["g_pos"] - p["g_neg"], g_tar)
    if mut in ("no_ragged_cell_tile", "higher_index_a"):
        w, u = o["q"]["w"], o["q"]["u"]
        N = Hc * Wc
        top = np.asarray([inputs(case)["W"] - 1, inputs(case)["H"] - 1], np.float32)
        ct = np.clip(u[:2], 0, top[:, None, None])
        d2 = (w[0][:, :, None] - ct[0][:, None, :]) ** 2 + (w[1][:, :, None] - ct[1][:, None, :]) ** 2
        if mut == "no_ragged_cell_tile":
            d2 = d2[:, :, :N // TILE_CELLS * TILE_CELLS]
            got["a"] = d2.argmin(axis=2)
        else:
            got["a"] = d2.shape[2] - 1 - d2[:, :, ::-1].argmin(axis=2)
        got["d"] = np.sqrt(np.take_along_axis(d2, got["a"][:, :, None], 2)[:, :, 0])
    return got


if __name__ == "__main__":
    import sys
    for name in sys.argv[1:] or CASES:
        print(f'"{name}": {find_seed(name)},', flush=True)
