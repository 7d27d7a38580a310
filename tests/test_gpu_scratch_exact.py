"""Every entry point that takes a scratch buffer, handed exactly the bytes its *_scratch_bytes query names, between two
4 KiB guard bands: the guards stay intact and every output is bit-identical to the same call with eight times the scratch.
One test per feature family, at the smallest shapes that reach each path of the layouts.  Equality only, no tolerance."""
import numpy as np
import pytest
import torch

from nano_vs_slam_amd import _dev, _lib
from nano_vs_slam_amd._dev import ptr as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, PATTERN = 4096, 0xA5


class Guarded:
    """``nbytes`` of scratch (``.mid``) inside a buffer whose first and last GUARD bytes hold PATTERN."""

    def __init__(self, nbytes):
        self.buf = torch.full((2 * GUARD + nbytes,), PATTERN, dtype=torch.uint8, device=DEV)
        self.mid = self.buf[GUARD:GUARD + nbytes]
        assert self.mid.data_ptr() % 256 == 0 and self.mid.numel() == nbytes

    def intact(self):
        n = self.mid.numel()
        return bool((self.buf[:GUARD] == PATTERN).all()) and bool((self.buf[GUARD + n:] == PATTERN).all())


def exact_vs_roomy(nbytes, call):
    """call(scratch tensor) -> dict of output tensors, run with exactly ``nbytes`` between guards and with 8 x as much."""
    assert nbytes > 0
    g = Guarded(nbytes)
    got = call(g.mid)
    torch.cuda.synchronize()
    assert g.intact(), "the call wrote outside the scratch it asked for"
    want = call(torch.empty(8 * nbytes, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert_same(got, want)
    return got


def assert_same(got, want, keys=None):
    for k in keys or want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k


def rand(gen, *shape):
    return torch.from_numpy(gen.standard_normal(shape).astype(np.float32)).to(DEV)


def unit(gen, *shape):
    d = rand(gen, *shape)
    return (d / d.norm(dim=-1, keepdim=True)).contiguous()


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)      # (zeros: rows a kernel leaves alone compare equal too)


def i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def match_call(lib, d0, n0, d1, n1, flags):
    B, k0, C = d0.shape
    k1 = d1.shape[1]

    def call(scratch):
        o = {"nn_idx": zeros(B, k0, dtype=torch.int32), "nn_dist": zeros(B, k0), "nn_dist2": zeros(B, k0),
             "match_q": zeros(B, k1, dtype=torch.int32), "match_d": zeros(B, k1)}
        _lib.check(lib.kp2d_match_descriptors_ex(P(d0), P(n0), P(d1), P(n1), B, k0, k1, C, 1.0, None, None, flags, P(o["nn_idx"]),
                                                 P(o["nn_dist"]), P(o["nn_dist2"]), P(o["match_q"]), P(o["match_d"]), P(scratch),
                                                 scratch.numel(), _dev.stream(DEV)))
        return o
    return call


@pytest.mark.parametrize("B,k0,k1", [(2, 37, 53), (512, 8, 8)])        # with partial arrays (sliced search) / without
def test_matcher(B, k0, k1):
    lib = _lib.load()
    gen = np.random.default_rng(5)
    d0, d1 = unit(gen, B, k0, 32), unit(gen, B, k1, 32)
    n0 = i32([k0 - b % 3 for b in range(B)])
    n1 = i32([k1 - b % 2 for b in range(B)])
    need = int(lib.kp2d_match_scratch_bytes(B, k0, k1))
    sliced = need > ((B * k1 * 16 + 255) & ~255)
    assert sliced == (B == 2)
    full = {}
    for flags in (0, 1):                                                # ratio test + one-to-one / mutual (the reverse arrays)
        full[flags] = exact_vs_roomy(need, match_call(lib, d0, n0, d1, n1, flags))
        assert int((full[flags]["match_q"] >= 0).sum()) > B            # (the comparison is not between empty results)
    if sliced:
        # the documented degradation: the base arrays alone, no partials -> the unsliced search, the same neighbours
        for flags in (0, 1):
            g = Guarded(B * k1 * 16)
            got = match_call(lib, d0, n0, d1, n1, flags)(g.mid)
            torch.cuda.synchronize()
            assert g.intact()
            assert_same(got, full[flags], ("nn_idx", "match_q"))


@pytest.mark.parametrize("mode", [0, 1])                                # KP2D_TOPK_BF / KP2D_TOPK_LG
def test_topk_pairs(mode):
    lib = _lib.load()
    gen = np.random.default_rng(6)
    B, k0, k1, k = 2, 37, 53, 10
    pts0, pts1 = rand(gen, B, k0, 2), rand(gen, B, k1, 2)
    n = k1 if mode == 0 else k0
    other = k0 if mode == 0 else k1
    rows = torch.from_numpy(gen.integers(-1, other, (B, n))).to(DEV)      # -1: no match
    assert int((rows >= 0).sum(1).min()) > k
    val = rand(gen, B, n).abs()
    match_q = rows.to(torch.int32) if mode == 0 else None
    matches0 = rows.to(torch.int64) if mode == 1 else None

    def call(scratch):
        o = {"pairs": zeros(B, k, 4), "idx": zeros(B, k, 2, dtype=torch.int32), "val": zeros(B, k), "count": zeros(B, dtype=torch.int32)}
        _lib.check(lib.kp2d_match_topk_pairs(mode, P(match_q), P(matches0), P(val), P(pts0), P(pts1), B, k0, k1, k, P(o["pairs"]),
                                             P(o["idx"]), P(o["val"]), P(o["count"]), P(scratch), scratch.numel(), _dev.stream(DEV)))
        return o

    got = exact_vs_roomy(int(lib.kp2d_match_topk_scratch_bytes(B, k0, k1)), call)
    assert got["count"].tolist() == [k, k]


def test_vpr_search():
    lib = _lib.load()
    gen = np.random.default_rng(7)
    nq, ndb, dim, k = 3, 3000, 32, 5        # 24 database tiles -> 24 slices' lists -> one merge level (2048 / k lists at a time)
    db, q = rand(gen, ndb, dim), rand(gen, nq, dim)
    packed = torch.empty(int(lib.kp2d_vpr_packed_bytes(ndb, dim)), dtype=torch.uint8, device=DEV)
    _lib.check(lib.kp2d_vpr_pack(P(db), ndb, dim, P(packed), _dev.stream(DEV)))

    def call(scratch):
        o = {"dist": zeros(nq, k), "idx": zeros(nq, k, dtype=torch.int64)}
        _lib.check(lib.kp2d_vpr_search(P(packed), P(db), ndb, dim, P(q), nq, None, k, 0, P(o["dist"]), P(o["idx"]), P(scratch),
                                       scratch.numel(), _dev.stream(DEV)))
        return o

    need = int(lib.kp2d_vpr_scratch_bytes(nq, ndb, dim, k))
    assert need > int(lib.kp2d_vpr_scratch_bytes(nq, 128, dim, k))      # (more than one slice: the merge buffer exists)
    got = exact_vs_roomy(need, call)
    want = ((q[:, None, :].double() - db[None].double()) ** 2).sum(2).topk(k, dim=1, largest=False).indices
    assert got["idx"].tolist() == want.tolist()


def test_kmeans_train():
    lib = _lib.load()
    gen = np.random.default_rng(8)
    n, dim, k, niter = 700, 16, 5, 3
    x = rand(gen, n, dim)

    def call(scratch):
        o = {"centroids": x[:k].clone(), "obj": zeros(niter), "assign": zeros(n, dtype=torch.int64), "dist": zeros(n),
             "counts": zeros(k, dtype=torch.int64)}
        _lib.check(lib.kp2d_kmeans_train(P(x), n, dim, P(o["centroids"]), k, niter, 0, 1234, P(o["obj"]), P(o["assign"]), P(o["dist"]),
                                         P(o["counts"]), P(scratch), scratch.numel(), _dev.stream(DEV)))
        return o

    got = exact_vs_roomy(int(lib.kp2d_kmeans_scratch_bytes(n, dim, k)), call)
    assert int(got["counts"].sum()) == n and float(got["obj"][2]) < float(got["obj"][0])


def test_keypoint_scores():
    lib = _lib.load()
    gen = np.random.default_rng(9)
    B, k0, k1, C, keep = 2, 37, 53, 32, 20

    def rows(k):
        xy = torch.from_numpy(gen.random((B, k, 2)).astype(np.float32) * np.float32([240.0, 320.0]))
        return torch.cat([xy, torch.from_numpy(gen.random((B, k, 1)).astype(np.float32))], 2).to(DEV).contiguous()

    pts0, pts1 = rows(k0), rows(k1)
    pts1[:, :k0, :2] = pts0[:, :, :2] + 0.5                             # (pairs within the distance threshold exist)
    d0, d1 = unit(gen, B, k0, C), unit(gen, B, k1, C)
    cnt0, cnt1 = i32([k0, k0 - 4]), i32([k1 - 3, k1])
    hom = torch.eye(3, dtype=torch.float64, device=DEV).repeat(B, 1, 1).contiguous()

    def repeatability(scratch):
        o = {"counts": zeros(B, 4, dtype=torch.int64), "le": zeros(B, 2, dtype=torch.float64)}
        _lib.check(lib.kp2d_kp_repeatability(P(pts0), P(cnt0), P(pts1), P(cnt1), P(hom), B, k0, k1, 240.0, 320.0, keep, 3.0,
                                             P(o["counts"]), P(o["le"]), P(scratch), scratch.numel(), _dev.stream(DEV)))
        return o

    def matching_score(scratch):
        o = {"counts": zeros(B, 4, dtype=torch.int64)}
        _lib.check(lib.kp2d_kp_matching_score(P(pts0), P(cnt0), P(d0), P(pts1), P(cnt1), P(d1), P(hom), B, k0, k1, C, 240.0, 320.0,
                                              keep, P(o["counts"]), P(scratch), scratch.numel(), _dev.stream(DEV)))
        return o

    got = exact_vs_roomy(int(lib.kp2d_kp_scratch_bytes(B, k0, k1, 0, keep)), repeatability)
    assert got["counts"][:, :2].tolist() == [[keep, keep]] * B
    got = exact_vs_roomy(int(lib.kp2d_kp_scratch_bytes(B, k0, k1, C, keep)), matching_score)
    assert int(got["counts"][:, 0].min()) > 0


def test_depth_sums():
    lib = _lib.load()
    gen = np.random.default_rng(10)
    B, n = 2, 10000
    gt, pred = rand(gen, B, n).abs() + 0.5, rand(gen, B, n).abs() + 0.5

    def call(scratch):
        o = {"sums": zeros(B, 11, dtype=torch.float64)}
        _lib.check(lib.kp2d_depth_sums(P(gt), P(pred), None, B, n, float("nan"), float("nan"), P(o["sums"]), P(scratch),
                                       scratch.numel(), _dev.stream(DEV)))
        return o

    got = exact_vs_roomy(int(lib.kp2d_depth_scratch_bytes(B, n)), call)
    assert got["sums"][:, 0].tolist() == [float(n)] * B


def test_lightglue_forward():
    from lightglue.lightglue import LightGlue
    from lightglue.lightglue_configs import get_light_glue_config
    from oracle import lightglue_oracle as lg
    from test_lightglue_oracle import make_data
    conf_in = dict(get_light_glue_config("S"), filter_threshold=0.1)
    conf = lg.get_config(conf_in)
    model = LightGlue(conf_in)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in lg.seeded_state_dict(conf).items()}, strict=True)
    model = model.to(DEV).eval()
    B, M, N, d = 2, 37, 53, conf["descriptor_dim"]
    data = make_data(B, M, N, conf["input_dim"], seed=11)
    k0, k1, d0, d1 = (torch.from_numpy(data[k]).to(DEV) for k in ("keypoints0", "keypoints1", "descriptors0", "descriptors1"))
    size = torch.from_numpy(data["view0"]["image_size"]).to(DEV)
    n0, n1 = i32([M, M - 5]), i32([N - 7, N])                           # padded sets: the counts are the layout's last piece
    lib, h = model._engine(DEV)

    def call(ws):
        o = {"scores": zeros(B, M + 1, N + 1), "m0": zeros(B, M, dtype=torch.int64), "m1": zeros(B, N, dtype=torch.int64),
             "ms0": zeros(B, M), "ms1": zeros(B, N), "ref0": zeros(B, M, d), "ref1": zeros(B, N, d)}
        _lib.check(lib.kp2d_lg_forward_counts(h, P(k0), P(k1), P(d0), P(d1), P(size), P(size), P(n0), P(n1), B, M, N, 0.1,
                                              P(o["scores"]), P(o["m0"]), P(o["m1"]), P(o["ms0"]), P(o["ms1"]), P(o["ref0"]),
                                              P(o["ref1"]), P(ws), ws.numel(), _dev.stream(DEV)))
        return o

    got = exact_vs_roomy(int(lib.kp2d_lg_workspace_bytes(h, B, M, N)), call)
    assert int((got["m0"] >= 0).sum()) > 0 and int(got["m0"][1, M - 5:].max()) == -1
