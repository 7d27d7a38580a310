"""Float64 reference, inputs and comparison of the LightGlue launch-form tests.  Test infrastructure, shared by
test_lightglue_forms.py (CPU: the form headers against the table below, the input conditions, E32) and
test_gpu_lightglue_forms.py (GPU: one child process per form).

FORMS   the process-wide knobs of csrc/options.h that choose the matcher's kernels, one setting each.
CASES   the smallest shapes at which each path can still go wrong, with the reason of each row.
Reference: oracle/lightglue_oracle.py evaluated on float64 copies of the data and the weights.  While it runs, lg.linear and
the two blocks are wrapped to record the largest |value| of any linear output and of the residual stream: the quantity that
reaches the fp16 hi halves of the device's split products (finite up to 65504).

Two weight families.  "spread": the seeded weights of every other LightGlue test (broad scores, almost no matches: the
transformer arithmetic).  "corresponding": the same with damped ffn.3 / final_proj bias / matchability weight, final_proj =
damp * seeded + diag * I and matchability bias + 3, on data whose set 1 is a permuted, noisy subset of set 0: the
descriptors survive the layers, corresponding points win both arg-maxima with scores from just above the threshold to
about 0.9, so the mutual check, the threshold and the score write of the filter are exercised on real matches.

Tolerance.  E32 = the error of the oracle's own float32 evaluation against its float64 one, in the same metric, measured
per case on the CPU.  The device may be FACTOR x E32 away from float64: its split products x w = xh wh + xh wl + xl wh drop
xl wl, at most 2^-22 relative = 4 x the fp32 unit roundoff 2^-24; every other operation is fp32 with fp32 accumulation as in
the float32 oracle.  The absolute bounds of test_lightglue_gpu.py (5e-5 on log_assignment, 2e-4 on the descriptors) hold
too on the unit-scale cases."""
import functools
import os
import sys

import numpy as np

from oracle import lightglue_oracle as lg

FACTOR = 4.0                      # device bound = FACTOR x E32 (derivation above); a case may carry its own, with the reason
ABS_LA, ABS_DESC = 5e-5, 2e-4     # test_lightglue_gpu.py check()
PEAK_LIMIT = 2.0 ** 15            # the device is checked while the intermediate peak stays below: a factor 2 under fp16's 65504
SWEEP_K = (-16, -8, 0, 4, 8, 12)  # descriptors of case "a" times 2^k
SWEEP_FORMS = ("default", "never_ksplit")

# every attention grid of the table stays below this many workgroups (case g: 3 x 4 x 64 = 768)
KSPLIT_ALWAYS = 1 << 20
FORMS = {
    "default": {},
    "unfused_tails": {"KP2D_LG_FUSE": "0"},
    "unfused_projections": {"KP2D_LG_FUSE_NEXT": "0"},
    "one_wave_tails": {"KP2D_LG_TAIL_NW": "1"},
    "never_ksplit": {"KP2D_ATT_KSPLIT": "0"},
    "always_ksplit": {"KP2D_ATT_KSPLIT": str(KSPLIT_ALWAYS)},
    "q128": {"KP2D_ATT_Q": "128"},
    "plain_grid": {"KP2D_ATT_AFFINE": "0"},
}
KNOBS = sorted({k for env in FORMS.values() for k in env})

S, F = lg.LIGHT_GLUE_CONFIGS["S"], lg.LIGHT_GLUE_CONFIGS["F"]
CASES = {
    # T = 130 (a wave without keys under key-split); ragged 16-row tail groups (460 rows); M != N with even B (affine grid)
    "a": dict(conf=S, B=2, M=130, N=100, family="corresponding", th=0.1, noise=0.05, seed=31),
    # several 32-key rounds per wave; B odd and M != N (non-affine grid); ragged 128-query tile
    "b": dict(conf=S, B=1, M=300, N=257, family="corresponding", th=0.1, noise=0.1, seed=32),
    # M = N: one launch of 2B sequences, kv_bshift; T < 128
    "c": dict(conf=S, B=3, M=96, N=96, family="spread", th=0.1, seed=11),
    # M = N with long T
    "d": dict(conf=S, B=1, M=200, N=200, family="corresponding", th=0.0, noise=0.05, seed=34),
    # D = 64 with head dim 16; the plain lg_linear path with real matches
    "e": dict(conf=F, B=2, M=96, N=130, family="corresponding", th=0.1, noise=0.05, seed=35, damp=0.1, diag=5.0),
    # the input_proj path
    "f": dict(conf=dict(input_dim=64, descriptor_dim=32, n_layers=2), B=2, M=90, N=75, family="spread", th=0.05, seed=5),
    # attention_split_kernel<512, 6>: 2 tiles x 4 heads x 64 sequences = 512 workgroups.  One layer keeps the CPU
    # reference to a few seconds
    "g": dict(conf=dict(S, n_layers=1), B=32, M=257, N=257, family="spread", th=0.1, seed=37),
    # padded sets through num_keypoints0 / num_keypoints1; each non-empty pair against the reference of its sliced sets
    "h": dict(conf=S, B=3, M=160, N=160, family="corresponding", th=0.1, noise=0.05, seed=38,
              counts=((130, 160), (160, 1), (0, 57))),
}


def conf_in(case):
    c = CASES[case]
    return dict(c["conf"], filter_threshold=c["th"])


# ---------------------------------------------------------------------------------------------------------------------
# weights and data
# ---------------------------------------------------------------------------------------------------------------------
def corresponding_state_dict(conf, damp=0.3, diag=4.0):
    sd = {k: np.array(v, copy=True) for k, v in lg.seeded_state_dict(conf).items()}
    d = conf["descriptor_dim"]
    for k in sd:
        if ".ffn.3." in k or k.endswith("final_proj.bias") or k.endswith("matchability.weight"):
            sd[k] = (damp * sd[k]).astype(np.float32)
        elif k.endswith("final_proj.weight"):
            sd[k] = (damp * sd[k] + diag * np.eye(d, dtype=np.float32)).astype(np.float32)
        elif k.endswith("matchability.bias"):
            sd[k] = (sd[k] + 3.0).astype(np.float32)
    return sd


def corresponding_data(B, M, N, din, seed, noise, size=(320.0, 240.0)):
    """Set 1 = a permuted subset of set 0 (all of it plus unrelated points when N > M), descriptors + noise * N(0, 1)
    renormalised, keypoints + 2 px of jitter."""
    g = np.random.default_rng(seed)
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    d0 = unit(g.standard_normal((B, M, din)))
    k0 = g.random((B, M, 2)) * np.asarray(size)
    d1, k1 = np.empty((B, N, din)), np.empty((B, N, 2))
    nc = min(M, N)
    for b in range(B):
        src = g.permutation(M)[:nc]
        dd = np.concatenate([d0[b, src], unit(g.standard_normal((N - nc, din)))], 0)
        kk = np.concatenate([k0[b, src], g.random((N - nc, 2)) * np.asarray(size)], 0)
        perm = g.permutation(N)
        d1[b] = unit(dd + noise * g.standard_normal((N, din)))[perm]
        k1[b] = (kk + 2.0 * g.standard_normal((N, 2)))[perm]
    sz = np.broadcast_to(np.asarray(size, np.float32), (B, 2)).copy()
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"keypoints0": f(k0), "keypoints1": f(k1), "descriptors0": f(d0), "descriptors1": f(d1),
            "view0": {"image_size": sz}, "view1": {"image_size": sz}}


def spread_data(B, M, N, din, seed, size=(320.0, 240.0)):
    """test_lightglue_oracle.make_data."""
    g = np.random.default_rng(seed)
    d = lambda n: (lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True))(g.standard_normal((B, n, din))).astype(np.float32)
    k = lambda n: (g.random((B, n, 2)) * np.asarray(size)).astype(np.float32)
    sz = np.broadcast_to(np.asarray(size, np.float32), (B, 2)).copy()
    return {"keypoints0": k(M), "keypoints1": k(N), "descriptors0": d(M), "descriptors1": d(N),
            "view0": {"image_size": sz}, "view1": {"image_size": sz}}


@functools.lru_cache(maxsize=None)
def weights(case):
    c = CASES[case]
    conf = lg.get_config(conf_in(case))
    if c["family"] == "spread":
        return lg.seeded_state_dict(conf)
    return corresponding_state_dict(conf, c.get("damp", 0.3), c.get("diag", 4.0))


def slice_pair(data, b, n0, n1):
    return {"keypoints0": data["keypoints0"][b:b + 1, :n0], "keypoints1": data["keypoints1"][b:b + 1, :n1],
            "descriptors0": data["descriptors0"][b:b + 1, :n0], "descriptors1": data["descriptors1"][b:b + 1, :n1],
            "view0": {"image_size": data["view0"]["image_size"][b:b + 1]}, "view1": {"image_size": data["view1"]["image_size"][b:b + 1]}}


@functools.lru_cache(maxsize=None)
def inputs(case, k=0):
    """The case's data, its descriptors times 2^k.  Padded sets (counts): pair b's existing rows correspond, the padding
    rows hold garbage (what a replayed graph's static buffers keep from earlier frames)."""
    c = CASES[case]
    din = lg.get_config(conf_in(case))["input_dim"]
    if c["family"] == "spread":
        data = spread_data(c["B"], c["M"], c["N"], din, c["seed"])
    else:
        data = corresponding_data(c["B"], c["M"], c["N"], din, c["seed"], c["noise"])
    if "counts" in c:
        g = np.random.default_rng(c["seed"] + 1000)
        for b, (n0, n1) in enumerate(c["counts"]):
            if n0 and n1:
                one = corresponding_data(1, n0, n1, din, c["seed"] + 10 + b, c["noise"])
                for key, n in (("keypoints0", n0), ("keypoints1", n1), ("descriptors0", n0), ("descriptors1", n1)):
                    data[key][b, :n] = one[key][0]
            for s, n in ((0, n0), (1, n1)):
                cap = data[f"keypoints{s}"].shape[1]
                data[f"keypoints{s}"][b, n:] = g.random((cap - n, 2)).astype(np.float32) * 500
                data[f"descriptors{s}"][b, n:] = g.standard_normal((cap - n, din)).astype(np.float32)
    if k:
        data["descriptors0"] = data["descriptors0"] * np.float32(2.0 ** k)
        data["descriptors1"] = data["descriptors1"] * np.float32(2.0 ** k)
    return data


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def la_error(a, ref):
    """the suite's metric on log_assignment (test_lightglue_gpu.py check())"""
    return float(np.max(np.abs(a - ref) / (1.0 + np.abs(ref))))


def desc_error(a, ref):
    return float(np.max(np.abs(a - ref)) / max(1.0, float(np.abs(ref).max())))


def forward64(data, sd, conf):
    """(lg.forward on float64 copies, the largest |value| of any linear output and of the residual stream)"""
    p64 = {k: v.astype(np.float64) for k, v in sd.items()}
    d64 = {k: ({"image_size": v["image_size"].astype(np.float64)} if isinstance(v, dict) else v.astype(np.float64))
           for k, v in data.items()}
    peak = [float(max(np.abs(d64["descriptors0"]).max(initial=0.0), np.abs(d64["descriptors1"]).max(initial=0.0)))]
    saved = lg.linear, lg.self_block, lg.cross_block

    def seen(y):
        for t in (y if isinstance(y, tuple) else (y,)):
            peak[0] = max(peak[0], float(np.abs(t).max(initial=0.0)))
        return y
    lg.linear = lambda *a: seen(saved[0](*a))
    lg.self_block = lambda *a: seen(saved[1](*a))
    lg.cross_block = lambda *a: seen(saved[2](*a))
    try:
        out = lg.forward(d64, p64, conf)
    finally:
        lg.linear, lg.self_block, lg.cross_block = saved
    return out, peak[0]


def _one_reference(data, sd, conf):
    ref, peak = forward64(data, sd, conf)
    rec = {"ref": ref, "peak": peak, "finite": bool(all(np.isfinite(ref[k]).all() for k in ("log_assignment", "ref_descriptors0")))}
    with np.errstate(all="ignore"):
        r32 = lg.forward(data, sd, conf)
    rec["e32_la"] = la_error(r32["log_assignment"].astype(np.float64), ref["log_assignment"])
    rec["e32_desc"] = max(desc_error(r32[k].astype(np.float64), ref[k]) for k in ("ref_descriptors0", "ref_descriptors1"))
    return rec


@functools.lru_cache(maxsize=None)
def reference(case, k=0):
    """[(b, n0, n1, record)]: one record for the whole batch (b = None), or one per non-empty pair of a padded case.
    record: ref (the float64 prediction), peak, e32_la, e32_desc.  Computed once per process and never modified."""
    c = CASES[case]
    conf = lg.get_config(conf_in(case))
    data, sd = inputs(case, k), weights(case)
    if "counts" not in c:
        return [(None, c["M"], c["N"], _one_reference(data, sd, conf))]
    return [(b, n0, n1, _one_reference(slice_pair(data, b, n0, n1), sd, conf))
            for b, (n0, n1) in enumerate(c["counts"]) if n0 and n1]


def comparison_mask(ref, th):
    """check()'s mask from the reference: rows whose top-2 gap is > 1e-3, whose score is not within 1e-4 of the threshold
    and whose column's arg-maximum is clear -> (ok [B, M], matched [B, M])."""
    inner = ref["log_assignment"][:, :-1, :-1]
    B, M, N = inner.shape
    ok = np.ones((B, M), bool)
    if N > 1:
        top2 = np.sort(inner, axis=2)[:, :, -2:]
        ok &= (top2[:, :, 1] - top2[:, :, 0]) > 1e-3
    rs0 = ref["matching_scores0"]
    ok &= ~((np.abs(rs0 - th) < 1e-4) & (rs0 > 0))
    if M > 1:
        top2c = np.sort(inner, axis=1)[:, -2:, :]
        clear1 = (top2c[:, 1] - top2c[:, 0]) > 1e-3
        ok &= np.take_along_axis(clear1, inner.argmax(2), 1)
    return ok, ref["matches0"] >= 0


def input_conditions(case):
    """(share of rows the mask keeps, share of rows kept AND matched in the reference), over every compared pair"""
    kept = matched = rows = 0
    for _b, _n0, _n1, rec in reference(case):
        ok, m = comparison_mask(rec["ref"], CASES[case]["th"])
        kept, matched, rows = kept + int(ok.sum()), matched + int((ok & m).sum()), rows + ok.size
    return kept / rows, matched / rows


def required_conditions(case):
    """what the inputs of a case must give before its match comparison means anything: (mask share, kept-and-matched share)"""
    return (0.95, 0.15) if CASES[case]["family"] == "corresponding" else (0.7, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# comparison of one child's outputs
# ---------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("log_assignment", "matches0", "matches1", "matching_scores0", "matching_scores1", "ref_descriptors0", "ref_descriptors1")


def compare(case, pred, k=0, matches=True, absolute=True):
    """pred: {output: array} of the device for the case.  Returns (figures, failures): the figures are printed by the
    tests before they assert that failures is empty."""
    c = CASES[case]
    th, M, N = c["th"], c["M"], c["N"]
    fig, bad = [], []
    if "counts" in c:
        for b, (n0, n1) in enumerate(c["counts"]):
            if n0 and n1:
                continue
            for key, want in (("matches0", -1), ("matches1", -1), ("matching_scores0", 0), ("matching_scores1", 0)):
                if not np.all(pred[key][b] == want):
                    bad.append(f"empty pair {b}: {key} is not all {want}")
    for b, n0, n1, rec in reference(case, k):
        ref = rec["ref"]
        tag = case if b is None else f"{case}[{b}]"
        if b is None:
            p = {key: pred[key] for key in OUTPUTS}
        else:   # the pair's existing rows / columns plus the dustbin row / column
            rows, cols = list(range(n0)) + [M], list(range(n1)) + [N]
            p = {"log_assignment": pred["log_assignment"][b][rows][:, cols][None],
                 "ref_descriptors0": pred["ref_descriptors0"][b:b + 1, :, :n0], "ref_descriptors1": pred["ref_descriptors1"][b:b + 1, :, :n1]}
            for s, n in ((0, n0), (1, n1)):
                for key in (f"matches{s}", f"matching_scores{s}"):
                    p[key] = pred[key][b:b + 1, :n]
                    if not np.all(pred[key][b, n:] == (-1 if key.startswith("matches") else 0)):
                        bad.append(f"{tag}: padding rows of {key}")
        finite = all(np.isfinite(p[key]).all() for key in OUTPUTS)
        if not finite:
            bad.append(f"{tag}: non-finite output")
            fig.append(dict(tag=tag, finite=False))
            continue
        la = la_error(p["log_assignment"].astype(np.float64), ref["log_assignment"])
        de = max(desc_error(p[key].astype(np.float64), ref[key]) for key in ("ref_descriptors0", "ref_descriptors1"))
        factor = c.get("factor", FACTOR)
        f = dict(tag=tag, finite=True, e32_la=rec["e32_la"], la=la, e32_desc=rec["e32_desc"], desc=de, peak=rec["peak"])
        fig.append(f)
        if not la <= factor * rec["e32_la"]:
            bad.append(f"{tag}: log_assignment {la:.3e} > {factor:g} x E32 = {factor * rec['e32_la']:.3e}")
        if not de <= factor * rec["e32_desc"]:
            bad.append(f"{tag}: ref_descriptors {de:.3e} > {factor:g} x E32 = {factor * rec['e32_desc']:.3e}")
        if absolute and not (la < ABS_LA and de < ABS_DESC):
            bad.append(f"{tag}: over the absolute bounds: log_assignment {la:.3e} (5e-5), ref_descriptors {de:.3e} (2e-4)")
        if not matches:
            continue
        ok, _ = comparison_mask(ref, th)
        m0, rm0, s0, rs0 = p["matches0"], ref["matches0"], p["matching_scores0"], ref["matching_scores0"]
        m1, rm1 = p["matches1"], ref["matches1"]
        f["compared"], f["matched"] = int(ok.sum()), int((ok & (rm0 >= 0)).sum())
        if not np.array_equal(m0[ok], rm0[ok]):
            bad.append(f"{tag}: matches0 differ on {int((m0[ok] != rm0[ok]).sum())} of {int(ok.sum())} clear rows")
        f["score"] = float(np.max(np.abs(s0[ok] - rs0[ok]), initial=0.0))
        if not f["score"] < 1e-4:
            bad.append(f"{tag}: matching_scores0 off by {f['score']:.3e} on the clear rows")
        if not (m1 == rm1).mean() > 0.97:
            bad.append(f"{tag}: matches1 agree on {(m1 == rm1).mean():.3f} of the rows")
        for bb in range(m0.shape[0]):      # the device's own outputs: matches are mutual and one-to-one
            i = np.nonzero(m0[bb] >= 0)[0]
            if not (np.all(m0[bb][i] < m1.shape[1]) and np.array_equal(m1[bb][m0[bb][i]], i) and len(set(m0[bb][i].tolist())) == len(i)):
                bad.append(f"{tag}: matches of pair {bb} are not mutual and one-to-one")
    return fig, bad


def format_figures(form, case, fig, k=None):
    out = []
    for f in fig:
        head = f"{form:20s} {f['tag']:5s}" + ("" if k is None else f" 2^{k:<3d}")
        if not f["finite"]:
            out.append(head + " NON-FINITE")
            continue
        out.append(head + f" la E32 {f['e32_la']:.2e} dev {f['la']:.2e} ({f['la'] / f['e32_la']:.2f}x)  desc E32 {f['e32_desc']:.2e} dev {f['desc']:.2e} "
                   f"({f['desc'] / f['e32_desc']:.2f}x)  peak {f['peak']:.3g}"
                   + (f"  rows {f['compared']} matched {f['matched']} score {f['score']:.1e}" if "score" in f else ""))
    return "\n".join(out)


# ---------------------------------------------------------------------------------------------------------------------
# the child process: every case (and the sweep's scales) through the product module, one .npz
# ---------------------------------------------------------------------------------------------------------------------
def device_run(out_path, sweep_ks=()):
    import torch
    from lightglue.lightglue import LightGlue
    dev = "cuda:0"
    res = {}

    def run(case, k, prefix):
        c = CASES[case]
        model = LightGlue(conf_in(case))
        model.load_state_dict({key: torch.from_numpy(v) for key, v in weights(case).items()}, strict=True)
        model = model.to(dev).eval()
        data = inputs(case, k)
        dd = {key: ({"image_size": torch.from_numpy(v["image_size"]).to(dev)} if isinstance(v, dict) else torch.from_numpy(v).to(dev))
              for key, v in data.items()}
        if "counts" in c:
            dd["num_keypoints0"] = torch.tensor([n[0] for n in c["counts"]], dtype=torch.int32, device=dev)
            dd["num_keypoints1"] = torch.tensor([n[1] for n in c["counts"]], dtype=torch.int32, device=dev)
        with torch.no_grad():
            pred = model(dd)
        torch.cuda.synchronize()
        for key in OUTPUTS:
            res[f"{prefix}/{key}"] = pred[key].cpu().numpy()

    for case in CASES:
        run(case, 0, case)
    for k in sweep_ks:
        run("a", int(k), f"sweep{int(k)}")
    np.savez(out_path, **res)


CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import lightglue_fp64_ref as R
R.device_run(sys.argv[2], sys.argv[3:])
"""


def child_env(form):
    """the parent's environment without any of the knobs, plus the form's setting"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(FORMS[form])
    return env


def unpack(z, prefix):
    return {key: z[f"{prefix}/{key}"] for key in OUTPUTS}
