"""float64 numpy oracle of the keypoint heads' training step (nano_vs_slam_amd.keypoint_training, csrc/keypoint_train.hip):
the self-supervised keypoint loss and its gradient by the formulas of include/kp2d.h, the walk over score_head, loc_head
(SimpleTaskHead) and desc_head (UpscaleHead) on running-statistic BatchNorm, and Adam.  Also the seeded inputs of the test
cases: fixtures under tests/golden/keypoint_training/ hold outputs, settings and seeds only (written by
tools/make_keypoint_training_golden.py from the reference's own KeypointNetwithIOLoss.forward under torch autograd); the
inputs are regenerated here from the seeds that generator kept (seeds.json).
"""
import json
import os

import numpy as np

import seg_training_ref as sr

hr, vr = sr.hr, sr.vr
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keypoint_training")

VALID_DIST, MARGIN, MIN_ANCHORS = 4.0, 0.2, 20        # KP2D_KEYPOINT_VALID_DIST, _MARGIN, _MIN_ANCHORS
CROSS_RATIO, RELAX = 2.0, 4.0
WEIGHTS = (1.0, 2.0, 1.0, 1.0)                        # loc, descriptor, score, keypoint: train_multitask.py's defaults
SLOPE, BN_EPS, LR = sr.SLOPE, sr.BN_EPS, sr.LR
MAX_STORED, TRAJ_STORED, FLOOR = sr.MAX_STORED, sr.TRAJ_STORED, sr.FLOOR
stride_of, stored, rel_err = sr.stride_of, sr.stored, sr.rel_err

# the loss alone: name -> (B, Hc, Wc, cell, C, Hf, Wf, weights)
LOSS_CASES = {
    "A": (1, 6, 7, 8, 16, 6, 7, WEIGHTS),            # n = 20: the smallest frame the descriptor term takes
    "B": (2, 7, 9, 4, 16, 14, 18, WEIGHTS),          # n = 35: ragged against the 64-anchor tile and the 16-wide MFMA tile
    "C": (3, 15, 20, 4, 32, 30, 40, WEIGHTS),        # n = 234, N = 300: several tiles; frame 1 under a strong homography
    "D": (2, 6, 6, 4, 16, 12, 12, WEIGHTS),          # n = 16: the descriptor term is skipped
    "E": (1, 8, 12, 4, 64, 16, 24, (0.7, 1.5, 1.3, 0.5)),
}
# the trainer: config S's heads on 2 pairs of 32 x 48 frames
TRAINER = {"B": 2, "Hc": 8, "Wc": 12, "cell": 4, "c3": 32, "c4": 64, "nfeat": 32}
STEPS = 5
BASE_SEED = {"A": 501, "B": 502, "C": 503, "D": 504, "E": 505, "T": 511}
GRADS = ("dscore_t", "dshift_t", "dfeat_t", "dscore_s", "dshift_s", "dfeat_s")
PARTS = ("loc", "metric", "usp", "con")
HEADS = ("score", "loc", "desc")
SIMPLE = ("convDa.conv.weight", "convDa.bn.weight", "convDa.bn.bias", "convDb.weight", "convDb.bias")
UPSCALE = ("convA.conv.weight", "convA.bn.weight", "convA.bn.bias", "convB.weight", "convB.bias",
           "confAa.conv.weight", "confAa.bn.weight", "confAa.bn.bias", "confBb.weight", "confBb.bias")
PARAMS = tuple(f"score_head.{p}" for p in SIMPLE) + tuple(f"loc_head.{p}" for p in SIMPLE) + tuple(f"desc_head.{p}" for p in UPSCALE)
HEAD_SLICE = {"score": slice(0, 5), "loc": slice(5, 10), "desc": slice(10, 20)}


def seed_of(name):
    with open(os.path.join(GOLDEN, "seeds.json")) as f:
        return int(json.load(f)[name])


def _homographies(rng, B, strong=()):
    """Normalised-coordinate homographies within 0.05 of the identity; ``strong``: frames pushed far enough that many warped
    points leave the image."""
    h = np.eye(3)[None].repeat(B, 0) + rng.uniform(-0.05, 0.05, (B, 3, 3))
    h[:, 2, 2] = 1.0
    for b in strong:
        h[b] = np.array([[0.8, -0.35, 0.55], [0.3, 0.85, -0.4], [0.08, -0.05, 1.0]]) + rng.uniform(-0.02, 0.02, (3, 3))
    return h.astype(np.float32)


def _views(rng, B, Hc, Wc, C, Hf, Wf):
    out = []
    for _ in range(2):
        out.append({"score": rng.uniform(0.02, 0.98, (B, 1, Hc, Wc)).astype(np.float32),
                    "shift": rng.uniform(-0.9, 0.9, (B, 2, Hc, Wc)).astype(np.float32),
                    "feat": rng.standard_normal((B, C, Hf, Wf)).astype(np.float32)})
    return out


def make_loss_inputs(name, seed=None):
    """-> dict(tgt, src: {score [B,1,Hc,Wc], shift [B,2,Hc,Wc], feat [B,C,Hf,Wf]} float32, hom [B,3,3] float32, H, W, cell,
    weights): uniform scores, shifts in +-0.9, normal descriptors.  The source's descriptor map is the target's plus noise
    in its second half of the channels, so that the triplet hinge has both active and inactive anchors."""
    return draw_loss_inputs(LOSS_CASES[name], seed_of(name) if seed is None else seed, strong=(1,) if name == "C" else ())


def draw_loss_inputs(shape, seed, strong=()):
    """make_loss_inputs' draw for any (B, Hc, Wc, cell, C, Hf, Wf, weights); ``strong``: the pairs under case C's strong
    homography."""
    B, Hc, Wc, cell, C, Hf, Wf, weights = shape
    rng = np.random.default_rng(seed)
    tgt, src = _views(rng, B, Hc, Wc, C, Hf, Wf)
    src["feat"] = (0.6 * tgt["feat"] + 0.8 * src["feat"]).astype(np.float32)
    hom = _homographies(rng, B, strong=strong)
    return {"tgt": tgt, "src": src, "hom": hom, "H": Hc * cell, "W": Wc * cell, "cell": cell, "weights": weights}


# ---- the loss --------------------------------------------------------------------------------------------------------------
def interior_mask(Hc, Wc):
    m = np.zeros((Hc, Wc), bool)
    m[1:Hc - 1, 1:Wc - 1] = True
    return m


def _taps(nx, ny, Hh, Ww):
    """grid_sample's four taps (bilinear, zeros, align_corners=True) of normalised points -> [(y, x, weight, inside)]"""
    dt = nx.dtype.type
    px, py = (nx + dt(1)) / dt(2) * dt(Ww - 1), (ny + dt(1)) / dt(2) * dt(Hh - 1)
    x0, y0 = np.floor(px), np.floor(py)
    out = []
    for ey in (0, 1):
        for ex in (0, 1):
            wx = (px - x0) if ex else (x0 + dt(1) - px)
            wy = (py - y0) if ey else (y0 + dt(1) - py)
            xx, yy = x0 + ex, y0 + ey
            inside = (xx >= 0) & (xx < Ww) & (yy >= 0) & (yy < Hh)
            out.append((np.where(inside, yy, 0).astype(np.int64), np.where(inside, xx, 0).astype(np.int64), wx * wy, inside))
    return out


def sample(img, nx, ny):
    """img [C, Hh, Ww], points [n] -> [C, n]"""
    out = np.zeros((img.shape[0], nx.size), img.dtype)
    for yy, xx, w, inside in _taps(nx, ny, img.shape[1], img.shape[2]):
        out += img[:, yy, xx] * (w * inside)
    return out


def sample_backward(g, nx, ny, shape):
    """g [C, n] -> d img [C, Hh, Ww]"""
    d = np.zeros(shape, g.dtype)
    for yy, xx, w, inside in _taps(nx, ny, shape[1], shape[2]):
        np.add.at(d, (slice(None), yy[inside], xx[inside]), g[:, inside] * w[inside])
    return d


def keypoint_loss(tgt, src, hom, H, W, cell, weights=WEIGHTS, relax=RELAX, cross_ratio=CROSS_RATIO, dtype=np.float64, grads=True, grids=None, blas=True):
    """include/kp2d.h's kp2d_keypoint_loss -> dict(loss, loc, metric, usp, con (unweighted), the six GRADS, M, n, hits, recall,
    usp_abs (the mean of |summand| behind usp), gaps and q (the generator's margins and the quantities they guard)).
    ``dtype=np.float32`` runs the forward quantities in float32 (the generator's estimate of a float32 run's decisions).
    ``grids``: an earlier result's ``["grids"]``, held fixed for the three samplings: the reference detaches them, so a finite
    difference of the loss agrees with the gradient only when they do not move.  ``blas=False`` forms the descriptor products
    elementwise, summed over the channel axis: equal columns then give equal values bit for bit, which a blocked GEMM does not
    promise.  ``stages`` holds what the device keeps in its scratch: per pair M_b, the matches and the sums fsum[0..4] (sum d,
    sum S, the consistency sum, sum S (d - mean), the hinge sum; ``usp_abs_b`` the sum of |S (d - mean)|), and per pair of the
    descriptor term a dict: neg, best, hit, hinge, cn (the negative's coefficient, 0 on an inactive hinge), the normalised
    rows r and t [n, C], and for the gradient walk the sampled rows, their norms, the points, g_pos and g_neg."""
    f = dtype
    st, ht, ft = (np.asarray(tgt[k], f) for k in ("score", "shift", "feat"))
    ss, hs, fs = (np.asarray(src[k], f) for k in ("score", "shift", "feat"))
    hom = np.asarray(hom, f)
    lw, dw, sw, kw = (float(v) for v in weights)
    B, _, Hc, Wc = st.shape
    C, Hf, Wf = ft.shape[1:]
    N = Hc * Wc
    inner = interior_mask(Hc, Wc).ravel()
    n = int(inner.sum())
    step = f((cell - 1) / 2.0)
    reach = f(cross_ratio * ((cell - 1) / 2.0))
    sx, sy = f((W - 1) / 2.0), f((H - 1) / 2.0)
    rows, cols = np.meshgrid(np.arange(Hc, dtype=f), np.arange(Wc, dtype=f), indexing="ij")

    def decode(shift):
        ux = (cols * f(cell) + step)[None] + shift[:, 0] * reach
        uy = (rows * f(cell) + step)[None] + shift[:, 1] * reach
        return (ux.reshape(B, N), uy.reshape(B, N), np.clip(ux, 0, f(W - 1)).reshape(B, N), np.clip(uy, 0, f(H - 1)).reshape(B, N))

    utx, uty, ctx, cty = decode(ht)
    usx, usy, csx, csy = decode(hs)
    nx, ny = csx / sx - f(1), csy / sy - f(1)
    h = hom.reshape(B, 9)[:, :, None]
    X = h[:, 2] + (nx * h[:, 0] + ny * h[:, 1])
    Y = h[:, 5] + (nx * h[:, 3] + ny * h[:, 4])
    Z = h[:, 8] + (nx * h[:, 6] + ny * h[:, 7])
    iz = f(1) / Z
    wnx, wny = X * iz, Y * iz
    wx, wy = (wnx + f(1)) * sx, (wny + f(1)) * sy
    gnx, gny, gwx_, gwy_ = (nx, ny, wnx, wny) if grids is None else grids
    ex, ey = wx[:, :, None] - ctx[:, None, :], wy[:, :, None] - cty[:, None, :]
    d2 = ex * ex + ey * ey
    a = d2.argmin(axis=2)                                     # the lowest index among equal values
    d = np.sqrt(np.take_along_axis(d2, a[:, :, None], 2)[:, :, 0])
    valid = (d < VALID_DIST) & inner[None]
    M = int(valid.sum())
    stm, ssm = st.reshape(B, N) * inner, ss.reshape(B, N) * inner
    S = np.take_along_axis(stm, a, 1) + ssm
    loc = float(d[valid].astype(np.float64).sum() / M) if M else 0.0
    summand = S[valid].astype(np.float64) * (d[valid].astype(np.float64) - loc)
    usp = float(summand.sum() / M) if M else 0.0
    usp_abs = float(np.abs(summand).mean()) if M else 0.0
    v = np.stack([sample(stm[b].reshape(1, Hc, Wc), gwx_[b], gwy_[b])[0] for b in range(B)])
    diff = (v - ss.reshape(B, N)) * inner
    con = float(2.0 * (diff.astype(np.float64) ** 2).sum() / (B * n)) if n else 0.0

    # ---- the descriptor term
    do_desc = n >= MIN_ANCHORS
    metric, hits = 0.0, 0
    cells = np.flatnonzero(inner)
    dfeat_t, dfeat_s = np.zeros(ft.shape, f), np.zeros(fs.shape, f)
    neg_gap, hinge_gap, relax_gap, pairs = [], [], [], []
    hinge_b = np.zeros(B)
    q_dmat, q_harg = [], []
    eps = f(1e-8)
    for b in range(B if do_desc else 0):
        pts = (gnx[b, cells], gny[b, cells]), (gwx_[b, cells], gwy_[b, cells])
        xr, xt = sample(fs[b], *pts[0]), sample(ft[b], *pts[1])
        sr_, st_ = np.sqrt(((xr + eps) ** 2).sum(0)), np.sqrt(((xt + eps) ** 2).sum(0))
        ref, tar = xr / (sr_ + eps), xt / (st_ + eps)
        dots = ref.T @ tar if blas else (ref.T[:, None, :] * tar.T[None, :, :]).sum(axis=2)
        dmat = np.sqrt(f(2) - f(2) * np.clip(dots, -1, 1) + eps)
        best = dmat.argmin(axis=1)
        kx, ky = wx[b, cells], wy[b, cells]
        hit = (kx[best] == kx) & (ky[best] == ky)
        hits += int(hit.sum())
        ax, ay = np.abs(kx[None, :] - kx[:, None]), np.abs(ky[None, :] - ky[:, None])
        within = (ax <= f(relax)) & (ay <= f(relax))
        masked = np.where(within, np.inf, dmat)
        neg = np.where(within.all(axis=1), best, masked.argmin(axis=1))
        ep, en = ref - tar + f(1e-6), ref - tar[:, neg] + f(1e-6)
        dp, dn = np.sqrt((ep * ep).sum(0)), np.sqrt((en * en).sum(0))
        harg = f(MARGIN) + dp - dn
        hinge = np.maximum(harg, 0)
        metric += float(hinge.astype(np.float64).mean() / B)
        hinge_b[b] = hinge.astype(np.float64).sum()
        pairs.append({"neg": neg, "best": best, "hit": hit, "hinge": hinge, "r": ref.T, "t": tar.T, "xr": xr, "xt": xt, "sr": sr_, "st": st_,
                      "pts": pts, "cn": np.zeros(n, f)})
        part = np.partition(masked, 1, axis=1)[:, :2]
        has_two = np.isfinite(part[:, 1])
        neg_gap.append(np.where(has_two, np.where(has_two, part[:, 1], 0) - np.where(has_two, part[:, 0], 0), np.inf))
        hinge_gap.append(np.abs(harg))
        # the margin of the pair's DECISION: inside the field by the smaller slack, outside it by the larger excess
        relax_gap.append(np.where(within, np.minimum(f(relax) - ax, f(relax) - ay), np.maximum(ax - f(relax), ay - f(relax))))
        q_dmat.append(dmat)
        q_harg.append(harg)
        if grads:
            scale = f(kw * dw * 2.0 / (B * n))            # (a Python float times the bool ``on`` would be float64 in either mode)
            on = hinge > 0
            g_pos, g_neg = scale * on * ep / np.where(dp > 0, dp, 1), scale * on * en / np.where(dn > 0, dn, 1)
            g_ref, g_tar = g_pos - g_neg, -g_pos
            np.add.at(g_tar.T, neg, g_neg.T)
            pairs[-1].update(g_pos=g_pos, g_neg=g_neg, cn=(scale * on / np.where(dn > 0, dn, 1) * (dn > 0)).astype(f))
            dfeat_s[b] = sample_backward(norm_back(g_ref, xr, sr_), *pts[0], fs[b].shape)
            dfeat_t[b] = sample_backward(norm_back(g_tar, xt, st_), *pts[1], ft[b].shape)

    loss = kw * (lw * loc + dw * 2.0 * metric + sw * usp + sw * con)
    out = {"loss": float(loss), "loc": loc, "metric": metric, "usp": usp, "con": con, "usp_abs": usp_abs, "M": M,
           "n": n if do_desc else 0, "hits": hits, "recall": hits / (B * n) if do_desc else 0.0, "a": a, "d": d, "valid": valid,
           "grids": (gnx, gny, gwx_, gwy_)}
    s64, d64 = S.astype(np.float64) * valid, (d.astype(np.float64) - loc) * valid
    out["stages"] = {"M_b": valid.sum(axis=1), "fsum": np.stack([(d.astype(np.float64) * valid).sum(axis=1), s64.sum(axis=1),
                                                                  (diff.astype(np.float64) ** 2).sum(axis=1), (s64 * d64).sum(axis=1), hinge_b], axis=1),
                     "usp_abs_b": np.abs(s64 * d64).sum(axis=1), "pairs": pairs}
    # ---- the margins of every discrete choice (the generator's conditions) and the quantities whose float32 error they face
    two = np.sqrt(np.partition(d2, 1, axis=2)[:, :, :2])
    u = np.stack([utx, uty, usx, usy])
    top = np.asarray([W - 1, H - 1, W - 1, H - 1], f)[:, None, None]
    out["gaps"] = {"a": np.where(valid, two[:, :, 1] - two[:, :, 0], np.inf), "valid": np.where(inner[None], np.abs(d - VALID_DIST), np.inf),
                   "relax": relax_gap, "neg": neg_gap, "hinge": hinge_gap, "clamp": np.minimum(np.abs(u), np.abs(u - top)),
                   "dmin": np.where(valid, d, np.inf)}
    out["q"] = {"d": d, "w": np.stack([wx, wy]), "wn": np.stack([wnx, wny]), "u": u, "dmat": q_dmat, "harg": q_harg}
    if not grads:
        return out

    # ---- gradients
    iM = 1.0 / M if M else 0.0
    Sbar = float(S[valid].astype(np.float64).sum() * iM)
    gd = kw * (lw * iM + sw * (S - Sbar) * iM) * valid
    safe = np.where(d > 0, d, 1)
    ux = np.where(d > 0, (wx - np.take_along_axis(ctx, a, 1)) / safe, 0)
    uy = np.where(d > 0, (wy - np.take_along_axis(cty, a, 1)) / safe, 0)
    gwx, gwy = gd * ux, gd * uy
    dS = kw * sw * (d - loc) * iM * valid
    gcon = (kw * sw * 4.0 / (B * n) if n else 0.0) * diff
    dctx, dcty, dst = np.zeros((B, N), f), np.zeros((B, N), f), np.zeros((B, N), f)
    for b in range(B):
        np.add.at(dctx[b], a[b], -gwx[b])
        np.add.at(dcty[b], a[b], -gwy[b])
        np.add.at(dst[b], a[b], dS[b])
        dst[b] += sample_backward(gcon[b][None], gwx_[b], gwy_[b], (1, Hc, Wc))[0].ravel()
    dss = dS - gcon
    # d w / d cs
    jxx, jxy = (h[:, 0] - wnx * h[:, 6]) * iz, (h[:, 1] - wnx * h[:, 7]) * iz * (sx / sy)
    jyx, jyy = (h[:, 3] - wny * h[:, 6]) * iz * (sy / sx), (h[:, 4] - wny * h[:, 7]) * iz
    open_ = lambda u, top: (u >= 0) & (u <= top)
    dshift_s = np.stack([(gwx * jxx + gwy * jyx) * open_(usx, W - 1), (gwx * jxy + gwy * jyy) * open_(usy, H - 1)], 1) * reach
    dshift_t = np.stack([dctx * open_(utx, W - 1), dcty * open_(uty, H - 1)], 1) * reach
    out.update(dscore_t=(dst * inner).reshape(B, 1, Hc, Wc), dshift_t=dshift_t.reshape(B, 2, Hc, Wc), dfeat_t=dfeat_t,
               dscore_s=(dss * inner).reshape(B, 1, Hc, Wc), dshift_s=dshift_s.reshape(B, 2, Hc, Wc), dfeat_s=dfeat_s)
    return out


def conditions(r64, r32, exempt=None):
    """-> None, or the reason the seed is refused: the oracle's margins (float64) against 100 x the float32 error of the
    quantity each guards, element by element.  ``exempt``: {"a": bool [B, N], "neg": [bool [n] per pair]}: the placed ties,
    whose own gap is 0 on purpose; no other choice is exempt."""
    q64, q32, g = r64["q"], r32["q"], r64["gaps"]
    exempt = exempt or {}
    err_d = np.abs(q32["d"].astype(np.float64) - q64["d"])
    err_w = np.abs(q32["w"].astype(np.float64) - q64["w"])
    err_u = np.abs(q32["u"].astype(np.float64) - q64["u"])
    gap_a = np.where(exempt["a"], np.inf, g["a"]) if "a" in exempt else g["a"]
    checks = [("the gap behind a_i", gap_a, err_d), ("|d - 4|", g["valid"], err_d), ("d away from 0", g["dmin"], err_d),
              ("a clamp end", g["clamp"], err_u)]
    inner = np.isfinite(g["valid"][0])
    for b in range(len(q64["dmat"])):
        ew = err_w[:, b][:, inner]
        pair = np.maximum(ew[0][:, None] + ew[0][None, :], ew[1][:, None] + ew[1][None, :])
        gap_neg = np.where(exempt["neg"][b], np.inf, g["neg"][b]) if "neg" in exempt else g["neg"][b]
        checks.append((f"a relax_field edge of pair {b}", g["relax"][b], pair))
        checks.append((f"the negative's gap of pair {b}", gap_neg, np.abs(q32["dmat"][b].astype(np.float64) - q64["dmat"][b]).max(axis=1)))
        checks.append((f"a hinge argument of pair {b}", g["hinge"][b], np.abs(q32["harg"][b].astype(np.float64) - q64["harg"][b])))
    for what, gap, err in checks:
        bad = ~(gap > 100.0 * err)
        if bad.any():
            k = np.unravel_index(int(np.argmax(bad)), bad.shape)
            return f"{what}: {gap[k]:.3e} within 100 x its float32 error {err[k]:.3e}"
    if (r64["M"], r64["hits"]) != (r32["M"], r32["hits"]) or not np.array_equal(r64["a"][r64["valid"]], r32["a"][r64["valid"]]):
        return "the float32 oracle run decides differently"
    return None


def norm_back(g, x, s, eps=1e-8):
    """Back through y = x / (|x + eps| + eps), per column: g, x [C, n], s [n] = |x + eps|."""
    eps = g.dtype.type(eps)
    D = s + eps
    return g / D - (g * x).sum(0) / (D * D * s) * (x + eps)


# ---- the trainer -------------------------------------------------------------------------------------------------------------
def head_channels(c3=32, c4=64, nfeat=32):
    """(Cin, Cout) of the conv of every parameter group, in PARAMS order: score (2 layers), loc (2), desc (4)."""
    return ((c4, c4), (c4, 1), (c4, c4), (c4, 2), (c4, c4), (c4, 4 * c3), (c3 + c4, c4), (c4, nfeat))


def make_trainer_inputs(seed=None):
    """-> dict: x [2B, c4, Hc, Wc] and skip [2B, c4, 2Hc, 2Wc] (the target view's B frames, then the source view's), hom,
    params (20 float32 arrays in PARAMS order), stats [(running_mean, running_var)] of the four BatchNorm layers (score, loc,
    desc.convA, desc.confAa), and the sizes.  The source view's maps are the target's plus noise."""
    t = TRAINER
    B, Hc, Wc, c3, c4 = t["B"], t["Hc"], t["Wc"], t["c3"], t["c4"]
    rng = np.random.default_rng(seed_of("T") if seed is None else seed)

    def maps(h, w):
        base = np.abs(rng.standard_normal((B, c4, h, w))) * 0.8 + 0.3 * rng.standard_normal((B, c4, 1, 1))
        return np.concatenate([base, base + 0.3 * rng.standard_normal(base.shape)]).astype(np.float32)

    x, skip = maps(Hc, Wc), maps(2 * Hc, 2 * Wc)
    params, stats = [], []
    for i, (ci, co) in enumerate(head_channels(c3, c4, t["nfeat"])):
        wgt = (rng.standard_normal((co, ci, 3, 3)) * np.sqrt(2.0 / (9 * ci))).astype(np.float32)
        if i in (0, 2, 4, 6):
            stats.append(((0.3 * rng.standard_normal(co)).astype(np.float32), rng.uniform(0.5, 1.5, co).astype(np.float32)))
            params += [wgt, rng.uniform(0.5, 1.5, co).astype(np.float32), (0.2 * rng.standard_normal(co)).astype(np.float32)]
        else:
            params += [wgt, (0.2 * rng.standard_normal(co)).astype(np.float32)]
    return {"x": x, "skip": skip, "hom": _homographies(rng, B), "params": params, "stats": stats, "B": B, "H": Hc * t["cell"],
            "W": Wc * t["cell"], "cell": t["cell"], "weights": WEIGHTS}


def heads_forward(inp, params):
    """-> dict(score, shift [2B, ., Hc, Wc] after the sigmoid / tanh, feat [2B, nfeat, 2Hc, 2Wc], acts)"""
    p, stats = params, inp["stats"]
    x, skip = np.asarray(inp["x"], np.float64), np.asarray(inp["skip"], np.float64)
    acts = {}

    def cbr(key, xin, i, s):
        y, c, scale, invstd = hr.cbr_forward(xin, p[i], p[i + 1], p[i + 2], stats[s][0], stats[s][1], SLOPE)
        acts[key] = (xin, y, c, scale, invstd)
        return y

    zs = sr.conv_bias(cbr("score", x, 0, 0), p[3], p[4])
    zl = sr.conv_bias(cbr("loc", x, 5, 1), p[8], p[9])
    up = sr.conv_bias(cbr("descA", x, 10, 2), p[13], p[14])
    cat = sr.shuffle_cat(up, skip)
    feat = sr.conv_bias(cbr("descAa", cat, 15, 3), p[18], p[19])
    return {"score": 1.0 / (1.0 + np.exp(-zs)), "shift": np.tanh(zl), "feat": feat, "acts": acts, "up": up}


def step_gradients(inp, params=None, train=HEADS):
    """One forward / loss / backward -> heads_forward's dict plus the loss dict and grads (PARAMS order; None for a head
    outside ``train``)."""
    params = [np.asarray(q, np.float64) for q in (inp["params"] if params is None else params)]
    f = heads_forward(inp, params)
    B = inp["B"]
    tgt = {k: f[k][:B] for k in ("score", "shift", "feat")}
    src = {k: f[k][B:] for k in ("score", "shift", "feat")}
    ls = keypoint_loss(tgt, src, inp["hom"], inp["H"], inp["W"], inp["cell"], inp["weights"])
    f.update({k: ls[k] for k in ("loss", "M", "n", "hits", "recall", "grids") + PARTS})
    g = {k: np.concatenate([ls["d" + k + "_t"], ls["d" + k + "_s"]]) for k in ("score", "shift", "feat")}
    grads = [None] * 20
    stats = inp["stats"]

    def simple(key, dz, i, s):
        lx, y, c, scale, invstd = f["acts"][key]
        grads[i + 3], grads[i + 4], dy = sr.conv_bias_backward(y, params[i + 3], dz)
        grads[i:i + 3] = hr.cbr_backward(lx, params[i], scale, stats[s][0], invstd, SLOPE, y, c, dy, need_dx=False)[:3]

    if "score" in train:
        simple("score", g["score"] * f["score"] * (1.0 - f["score"]), 0, 0)
    if "loc" in train:
        simple("loc", g["shift"] * (1.0 - f["shift"] ** 2), 5, 1)
    if "desc" in train:
        lx, y, c, scale, invstd = f["acts"]["descAa"]
        grads[18], grads[19], dy = sr.conv_bias_backward(y, params[18], g["feat"])
        *grads[15:18], dcat = hr.cbr_backward(lx, params[15], scale, stats[3][0], invstd, SLOPE, y, c, dy)
        dup = sr.shuffle_cat_backward(dcat, params[13].shape[0] // 4)
        simple("descA", dup, 10, 2)
    f["grads"] = grads
    f["maps"] = g
    return f


def loss_from(inp, params, grids=None):
    f = heads_forward(inp, params)
    B = inp["B"]
    tgt = {k: f[k][:B] for k in ("score", "shift", "feat")}
    src = {k: f[k][B:] for k in ("score", "shift", "feat")}
    return keypoint_loss(tgt, src, inp["hom"], inp["H"], inp["W"], inp["cell"], inp["weights"], grads=False, grids=grids)["loss"]


def trajectory(inp, train=HEADS, steps=STEPS, lr=LR):
    """Adam on one batch -> (losses [steps], the 20 parameters after every step)"""
    params = [p.astype(np.float64) for p in inp["params"]]
    trained = [i for hname in HEADS if hname in train for i in range(20)[HEAD_SLICE[hname]]]
    opt = vr.Adam([params[i] for i in trained], lr=lr)
    losses, after = [], []
    for _ in range(steps):
        s = step_gradients(inp, params, train)
        losses.append(s["loss"])
        opt.step([np.asarray(s["grads"][i]).reshape(params[i].shape) for i in trained])
        after.append([q.copy() for q in params])
    return np.asarray(losses), after


# ---- fixtures and bounds -------------------------------------------------------------------------------------------------------
def load_fixture(name):
    return np.load(os.path.join(GOLDEN, f"case_{name}.npz"))


def load_trainer():
    return np.load(os.path.join(GOLDEN, "trainer.npz"))


LOSS_KEYS = ("loss",) + PARTS + GRADS


def bounds():
    """Per quantity of LOSS_KEYS the bound on E = max|G - G64| / max|G64| (loss, loc, metric, con: |v - v64| / |v64|; usp:
    |v - v64| / mean|summand|): max(8 x the reference's own float32 error of that quantity, the maximum over the loss
    cases, 16 x 2^-24)."""
    fx = [load_fixture(n) for n in LOSS_CASES]
    return {k: max(8.0 * max(float(f["err32_" + k]) for f in fx), FLOOR) for k in LOSS_KEYS}


def trainer_bounds():
    """The same for the trainer's fixture: every key err32_* of trainer.npz."""
    fx = load_trainer()
    return {k[6:]: max(8.0 * float(fx[k]), FLOOR) for k in fx.files if k.startswith("err32_")}
