"""The view-pair calls on the device (nano_vs_slam_amd.augment, csrc/augment.hip) against the float64 numpy oracle
tests/augment_ref.py, which tests/test_augment_cpu.py holds to the reference's sampler and to torch's grid_sample.

Nearest warps and the backward's float32 sums are compared for EXACT equality at every pixel: the device and the oracle run the
same double arithmetic in the same order, so there are no exemptions for near-ties.  The workgroup tile is
augment_ref.TILE_H x augment_ref.TILE_W = 4 rows x 64 columns of pixels (KP2D_WARP_TILE_H / _W); 70 x 130 is past one tile in
both directions, with ragged last tiles.  Bounds: bilinear 16 x 2^-24 of the source's largest magnitude; the backward against
float64 fan-in x 2^-24 x max|dy|; the cross-view term max(8 x the float32 torch formulation's own error against float64,
16 x 2^-24 of the quantity's largest magnitude).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import augment_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
FLOOR = 16 * EPS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _aug():
    from nano_vs_slam_amd import augment
    return augment


def _homs(name, shape, N=1):
    one = {"sampled": ar.reference_homography(shape), "general": ar.GENERAL, "identity": np.eye(3), "halves": ar.HALVES,
           "zoom": ar.ZOOM_IN, "full_scan": ar.FULL_SCAN}[name]
    return np.broadcast_to(one, (N, 3, 3)).copy()


def _source(dtype, shape, seed=1):
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        return rng.standard_normal(shape).astype(np.float32)
    return rng.integers(0, 255, shape).astype(dtype)          # 255 itself is kept for the fill


# ---- 1. the sampler ------------------------------------------------------------------------------------------------------------
def test_draws_equal_the_restatement():
    got = _np(_aug().homography_draws(33, seed=11, step=2, device=DEV))
    want = ar.homography_draws(33, 11, 2)
    print("draws: max|diff|", np.abs(got - want).max())
    assert got.shape == (33, 9) and np.abs(got - want).max() <= 1e-12
    assert np.array_equal(got[:, [4, 6, 7, 8]], want[:, [4, 6, 7, 8]])          # the uniforms are integers scaled: exact
    assert np.array_equal(got, _np(_aug().homography_draws(33, seed=11, step=2, device=DEV)))


def test_sampler_against_the_reference_fixtures():
    fx, cases = ar.load_sampler(), ar.sampler_cases()
    worst = 0.0
    for name, case in cases.items():
        draws = _dev(fx["draws_" + name])
        h64 = _aug().sample_homographies(16, case["shape"], draws=draws, dtype=torch.float64, **case["options"])
        h32 = _aug().sample_homographies(16, case["shape"], draws=draws, **case["options"])
        err = np.abs(_np(h64) - fx["hom_" + name]).max()
        worst = max(worst, err)
        assert h64.shape == (16, 3, 3) and err <= 1e-9, (name, err)
        assert h32.dtype == torch.float32 and torch.equal(h32, h64.float())
    print("sampler: largest |device - reference|", worst)


def test_sampled_views_stay_inside():
    for shape in ((120, 160), (100, 100), (17, 23)):
        homs = _np(_aug().sample_homographies(64, shape, seed=5, step=3, device=DEV, dtype=torch.float64))
        want = ar.sample_homographies(ar.homography_draws(64, 5, 3), shape)
        assert np.abs(homs - want).max() <= 1e-9
        for h in homs:
            assert (np.abs(ar.view_corners(h)) <= 1.0 + 1e-12).all()


# ---- 2. the nearest warp: exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(17, 23), (70, 130)])
@pytest.mark.parametrize("name", ["sampled", "general", "identity"])
@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_nearest_warp_is_exact(kind, name, shape):
    dtype, C_, fill = (np.float32, 3, -1.0) if kind == "f32" else (np.uint8, 1, 255)
    x = _source(dtype, (1, C_) + shape)
    hom = _homs(name, shape)
    got = _np(_aug().warp(_dev(x), _dev(hom), fill=fill))
    want = ar.warp(x, hom, fill=fill)
    assert got.dtype == x.dtype and np.array_equal(got, want)
    if name == "identity":
        assert np.array_equal(got, x)
    if name == "general":
        assert (want == fill).any() and 0.1 < 1 - ar.nearest(hom[0], *shape)[0].mean() < 0.3


def test_exact_halves_go_to_even():
    x = _source(np.float32, (1, 3, 9, 17))
    hom = _homs("halves", (9, 17))
    assert np.array_equal(_np(_aug().warp(_dev(x), _dev(hom), fill=7.0)), ar.warp(x, hom, fill=7.0))


@pytest.mark.parametrize("f64", [False, True])
def test_three_frames_three_matrices(f64):
    x = _source(np.float32, (3, 2, 17, 23))
    hom = np.stack([ar.GENERAL, ar.reference_homography((17, 23), 1), ar.ZOOM_IN])
    hom = hom if f64 else hom.astype(np.float32)
    got = _np(_aug().warp(_dev(x), _dev(hom), fill=0.0))
    assert np.array_equal(got, ar.warp(x, hom.astype(np.float64), fill=0.0))
    lab = _source(np.int64, (3, 17, 23), seed=2)                # [N, H, W] labels, int64 and int32
    assert np.array_equal(_np(_aug().warp(_dev(lab), _dev(hom), fill=0)), ar.warp(lab[:, None], hom.astype(np.float64), fill=0)[:, 0])
    lab32 = lab.astype(np.int32)
    assert np.array_equal(_np(_aug().warp(_dev(lab32), _dev(hom), fill=-3)), ar.warp(lab32[:, None], hom.astype(np.float64), fill=-3)[:, 0])


def test_stride_four_is_the_full_warp_subsampled():
    x = _source(np.uint8, (2, 1, 32, 48))
    d = _source(np.float32, (2, 1, 32, 48))
    hom = np.stack([ar.GENERAL, ar.reference_homography((32, 48))]).astype(np.float32)
    hd = _dev(hom)
    got = _aug().warp(_dev(x), hd, fill=0, stride=4)
    assert got.shape == (2, 1, 8, 12) and torch.equal(got, _aug().warp(_dev(x), hd, fill=0)[:, :, ::4, ::4])
    assert np.array_equal(_np(got), ar.warp(x, hom.astype(np.float64), fill=0, stride=4))
    assert np.array_equal(_np(_aug().warp(_dev(d), hd, fill=0.0, stride=4)), ar.warp(d, hom.astype(np.float64), fill=0.0, stride=4))


# ---- 3. the bilinear warp ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(17, 23), (70, 130)])
def test_bilinear_warp(shape):
    x = _source(np.float32, (2, 3) + shape)
    hom = np.stack([ar.GENERAL, ar.reference_homography(shape)])
    got = _np(_aug().warp(_dev(x), _dev(hom), mode="bilinear", fill=9.0)).astype(np.float64)
    want = ar.warp(x, hom, mode="bilinear")
    err, bound = np.abs(got - want).max(), FLOOR * np.abs(x).max()
    print(f"bilinear {shape}: {err:.3e} of {bound:.3e}")
    assert err <= bound


# ---- 4. the backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("zoom", (17, 23), 1), ("general", (17, 23), 1), ("sampled", (17, 23), 1), ("zoom", (70, 130), 1),
                                  ("general", (70, 130), 1), ("zoom", (32, 48), 4), ("sampled", (32, 48), 4), ("full_scan", (6, 8), 1)],
                         ids=lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}-s{c[2]}")
def test_backward_is_exact(case):
    name, (H, W), stride = case
    hom = _homs(name, (H, W), 2)
    hom[1] = ar.GENERAL if name != "general" else ar.ZOOM_IN      # the second frame under another matrix
    dy = _source(np.float32, (2, 3, H // stride, W // stride), seed=3)
    got = _aug().warp_backward(_dev(dy), _dev(hom), (H, W), stride=stride)
    want32 = ar.warp_backward(dy, hom, (H, W), stride, dtype=np.float32)
    want64 = ar.warp_backward(dy, hom, (H, W), stride, dtype=np.float64)
    fan = np.stack([ar.fan_in(h, H, W, stride) for h in hom])
    assert np.array_equal(_np(got), want32)
    bound = fan[:, None] * EPS * np.abs(dy).max()
    assert (np.abs(_np(got).astype(np.float64) - want64) <= bound).all()
    assert (fan == 0).any() and not _np(got)[:, :, fan[0] == 0][0].any()          # source pixels with no preimage get 0
    if name == "zoom" and stride == 1:
        assert fan[0].max() >= 4
    if name == "full_scan":
        assert int(ar.nearest(hom[0], H, W)[0].sum()) == 31 and int((ar.inverse_corner_w(hom[0], H, W) <= 0).sum()) == 92
    assert torch.equal(got, _aug().warp_backward(_dev(dy), _dev(hom), (H, W), stride=stride))      # two runs: the same bits
    g32 = _aug().warp_backward(_dev(dy), _dev(hom.astype(np.float32)), (H, W), stride=stride)    # float32 matrices: their own decisions
    assert np.array_equal(_np(g32), ar.warp_backward(dy, hom.astype(np.float32).astype(np.float64), (H, W), stride, dtype=np.float32))


# ---- 5. the cross-view term ----------------------------------------------------------------------------------------------------
def _torch32(depth, aug, homs, weight, inside_only):
    """The float32 torch formulation on the CPU (the nearest decisions are the float64 grid's, the gather is then exact):
    weight x mse over the counted pixels under autograd -> (loss, d_depth, d_depth_aug)."""
    N, H, W = depth.shape
    near = [ar.nearest(h, H, W) for h in homs]
    inside = torch.from_numpy(np.stack([n[0] for n in near]))
    at = torch.from_numpy(np.stack([n[1] for n in near])).reshape(N, -1)
    a, b = torch.from_numpy(depth).requires_grad_(True), torch.from_numpy(aug).requires_grad_(True)
    warped = a.reshape(N, -1).gather(1, at).reshape(N, H, W) * inside
    diff = b - warped
    if inside_only:
        diff = diff * inside
    M = int(inside.sum()) if inside_only else N * H * W
    loss = np.float32(weight) * (diff * diff).sum() / M
    loss.backward()
    return float(loss.detach()), a.grad.numpy(), b.grad.numpy()


def _rel(got, want):
    scale = np.abs(want).max()
    return np.abs(np.asarray(got, np.float64) - want).max() / scale if scale > 0 else float(np.abs(got).max() > 0)


@pytest.mark.parametrize("inside_only", [False, True])
@pytest.mark.parametrize("shape", [(2, 16, 24), (3, 41, 53)])
def test_cross_view_mse(shape, inside_only):
    N, H, W = shape
    rng = np.random.default_rng(12)
    depth, aug = rng.random(shape).astype(np.float32), rng.random(shape).astype(np.float32)
    homs = np.stack([ar.GENERAL, ar.reference_homography((H, W)), ar.ZOOM_IN][:N]).astype(np.float32)
    ref = ar.cross_view_mse(depth, aug, homs.astype(np.float64), 0.5, inside_only)
    t32 = _torch32(depth, aug, homs.astype(np.float64), 0.5, inside_only)
    loss, d_depth, d_aug, inside = _aug().cross_view_mse(_dev(depth), _dev(aug), _dev(homs), weight=0.5, inside_only=inside_only)
    assert int(inside) == ref["inside"] and loss.shape == () and d_depth.shape == shape and d_aug.shape == shape
    worst = 0.0
    for key, got, want, yard in (("loss", float(loss), np.float64(ref["loss"]), t32[0]), ("d_depth", _np(d_depth), ref["d_depth"], t32[1]),
                                 ("d_depth_aug", _np(d_aug), ref["d_depth_aug"], t32[2])):
        bound = max(8 * _rel(yard, want), FLOOR)
        e = _rel(got, want)
        worst = max(worst, e / bound)
        print(f"cross view {shape} inside_only={inside_only}: E({key}) {e:.3e} of {bound:.3e}")
        assert e <= bound, key
    print(f"cross view {shape} inside_only={inside_only}: largest share of a bound {worst:.3f}")
    again = _aug().cross_view_mse(_dev(depth), _dev(aug), _dev(homs), weight=0.5, inside_only=inside_only)
    assert all(torch.equal(x, y) for x, y in zip((loss, d_depth, d_aug, inside), again))
    l4 = _aug().cross_view_mse(_dev(depth)[:, None], _dev(aug)[:, None], _dev(homs), weight=0.5, inside_only=inside_only)
    assert l4[1].shape == (N, 1, H, W) and torch.equal(l4[0], loss) and torch.equal(l4[1][:, 0], d_depth)


def test_cross_view_wholly_outside():
    rng = np.random.default_rng(13)
    depth, aug = rng.random((2, 16, 24)).astype(np.float32), rng.random((2, 16, 24)).astype(np.float32)
    far = np.broadcast_to(np.array([[1.0, 0.0, 5.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], np.float32), (2, 3, 3)).copy()
    loss, d_depth, d_aug, inside = _aug().cross_view_mse(_dev(depth), _dev(aug), _dev(far), inside_only=True)
    assert int(inside) == 0 and float(loss) == 0.0 and not d_depth.any() and not d_aug.any()
    loss, d_depth, d_aug, inside = _aug().cross_view_mse(_dev(depth), _dev(aug), _dev(far))      # the reference: depth_aug towards 0
    ref = ar.cross_view_mse(depth, aug, far.astype(np.float64), 0.5)
    assert int(inside) == 0 and _rel(float(loss), np.float64(ref["loss"])) <= FLOOR and not d_depth.any()
    assert _rel(_np(d_aug), ref["d_depth_aug"]) <= FLOOR


# ---- 6. view_pair ---------------------------------------------------------------------------------------------------------------
def test_view_pair_is_the_reference_batch():
    rng = np.random.default_rng(14)
    N, H, W = 2, 32, 48
    frames = rng.random((N, 3, H, W)).astype(np.float32)
    labels = rng.integers(1, 28, (N, H, W)).astype(np.int64)
    depth = (0.1 + rng.random((N, H, W))).astype(np.float32)
    batch = _aug().view_pair(_dev(frames), seg=_dev(labels), depth=_dev(depth), d_f=4, seed=3, step=1)
    assert sorted(batch) == ["depth", "depth_aug", "homography", "image", "image_aug", "seg", "seg_aug"]
    hom = batch["homography"]
    assert hom.dtype == torch.float32 and torch.equal(hom, _aug().sample_homographies(N, (H, W), seed=3, step=1, device=DEV))
    h64 = _np(hom).astype(np.float64)
    image = frames * np.float32(2.0) - np.float32(1.0)
    assert np.array_equal(_np(batch["image"]), image)
    assert np.array_equal(_np(batch["image_aug"]), ar.warp(frames, h64, fill=0.0) * np.float32(2.0) - np.float32(1.0))     # the reference's order
    assert np.array_equal(_np(batch["seg"]), labels[:, ::4, ::4]) and np.array_equal(_np(batch["depth"]), depth[:, ::4, ::4])
    assert np.array_equal(_np(batch["seg_aug"]), ar.warp(labels[:, None], h64, fill=0)[:, 0, ::4, ::4])
    assert np.array_equal(_np(batch["depth_aug"]), ar.warp(depth[:, None], h64, fill=0.0)[:, 0, ::4, ::4])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    aug = _aug()
    x = torch.zeros(2, 1, 8, 12, device=DEV)
    hom = torch.eye(3, device=DEV).expand(2, 3, 3).contiguous()
    bad = [lambda: aug.warp(x.cpu(), hom), lambda: aug.warp(x, hom.cpu()), lambda: aug.warp(x[:, :, :1], hom), lambda: aug.warp(x[:, :, :, :1], hom),
           lambda: aug.warp(x, hom, stride=5), lambda: aug.warp(x, hom, stride=0), lambda: aug.warp(x.to(torch.uint8), hom, mode="bilinear"),
           lambda: aug.warp(x, hom[:1]), lambda: aug.warp(x, hom.reshape(2, 9)), lambda: aug.warp(x, hom.half()), lambda: aug.warp(x, hom, mode="cubic"),
           lambda: aug.warp(x.to(torch.uint8), hom, fill=256), lambda: aug.warp(x.double(), hom),
           lambda: aug.warp_backward(x, hom, (8, 13)), lambda: aug.warp_backward(x, hom, (16, 24)), lambda: aug.warp_backward(x, hom, (8, 12), stride=4),
           lambda: aug.warp_backward(x.cpu(), hom, (8, 12)), lambda: aug.warp_backward(x.double(), hom, (8, 12)),
           lambda: aug.cross_view_mse(x, x[:1], hom), lambda: aug.cross_view_mse(x.cpu(), x, hom), lambda: aug.cross_view_mse(x, x, hom, weight=-1.0),
           lambda: aug.cross_view_mse(x, x, hom.double()[:1]), lambda: aug.sample_homographies(2, (8, 12), draws=torch.zeros(2, 8, dtype=torch.float64, device=DEV)),
           lambda: aug.sample_homographies(2, (8, 12), draws=torch.zeros(2, 9, device=DEV)), lambda: aug.sample_homographies(2, (8, 12), device=DEV, angle=3),
           lambda: aug.homography_draws(0, device=DEV), lambda: aug.homography_draws(2, step=-1, device=DEV), lambda: aug.view_pair(x.cpu())]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    # the C ABI itself, before any launch
    from nano_vs_slam_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1 << 12, device=DEV)
    p, null = C.c_void_p(buf.data_ptr()), None
    ARG = -1
    assert lib.kp2d_warp(p, 0, p, 0, 1, 1, 1, 8, 1, 0, 0.0, p, null) == ARG               # H < 2
    assert lib.kp2d_warp(p, 0, p, 0, 1, 1, 8, 12, 5, 0, 0.0, p, null) == ARG              # the stride does not divide
    assert lib.kp2d_warp(p, 1, p, 0, 1, 1, 8, 12, 1, 1, 0.0, p, null) == ARG              # bilinear on uint8
    assert lib.kp2d_warp(p, 4, p, 0, 1, 1, 8, 12, 1, 0, 0.0, p, null) == ARG              # no such dtype
    assert lib.kp2d_warp(p, 1, p, 0, 1, 1, 8, 12, 1, 0, 0.5, p, null) == ARG              # fill is no uint8
    assert lib.kp2d_warp(p, 0, p, 0, 70000, 1, 8, 12, 1, 0, 0.0, p, null) == ARG
    assert lib.kp2d_warp(null, 0, p, 0, 1, 1, 8, 12, 1, 0, 0.0, p, null) == ARG and b"null" in lib.kp2d_last_error()
    assert lib.kp2d_warp_backward(p, p, 0, 1, 1, 8, 12, 3, p, null) == ARG
    assert lib.kp2d_warp_backward(p, null, 0, 1, 1, 8, 12, 1, p, null) == ARG
    assert lib.kp2d_cross_view_scratch_bytes(0, 96) == 0 and lib.kp2d_cross_view_scratch_bytes(2, 96) > 0
    assert lib.kp2d_cross_view_mse(p, p, p, 0, 1, 8, 12, 0.5, 0, p, p, p, p, p, 8, null) == ARG and b"scratch" in lib.kp2d_last_error()
    assert lib.kp2d_cross_view_mse(p, p, p, 0, 1, 8, 12, float("nan"), 0, p, p, p, p, p, 1 << 12, null) == ARG
    assert lib.kp2d_homography_draws(p, 0, 1, 0, null) == ARG and lib.kp2d_homography_draws(p, 1, 1, -1, null) == ARG
    assert lib.kp2d_homography_sample(p, 1, 8, 12, 1, 1, 1, 1, 0, 100, 0.2, 0.2, 0.7, 1.5, p, p, null) == ARG      # n_scales 0
    assert lib.kp2d_homography_sample(p, 1, 8, 12, 1, 1, 1, 1, 100, 100, 0.2, 0.2, 0.7, 1.5, null, null, null) == ARG
    torch.cuda.synchronize()
    assert not buf.any()


# ---- 8. the depth trainer's pair step ----------------------------------------------------------------------------------------------
def _pair():
    import depth_pair_ref as pr
    from test_gpu_depth_training import _stand_in
    inp = pr.make_inputs()
    t = {k: _dev(inp[k]) for k in ("x", "skip", "x_aug", "skip_aug", "gt", "gt_aug", "homography")}
    return pr, inp, _stand_in, t


class _Check:
    """E = max|G - G64| / max|G64| (a scalar: relative) against its bound; keeps the largest share."""

    def __init__(self, bounds):
        self.bounds, self.worst = bounds, (0.0, "")

    def __call__(self, key, got, want):
        e = _rel(got, np.asarray(want, np.float64))
        print(f"pair step: E({key}) {e:.3e} of {self.bounds[key]:.3e}")
        if e / self.bounds[key] > self.worst[0]:
            self.worst = (e / self.bounds[key], key)
        assert e <= self.bounds[key], key


def test_pair_gradients_against_the_reference():
    from nano_vs_slam_amd import depth_training as dt
    pr, inp, stand_in, t = _pair()
    fx, chk = pr.load_fixture(), _Check(pr.bounds())
    trainer = dt.DepthHeadTrainer(stand_in(inp), train="head")
    loss, logits, grads = trainer.pair_gradients((t["x"], t["skip"]), (t["x_aug"], t["skip_aug"]), t["gt"], t["gt_aug"], t["homography"],
                                                 cross_weight=float(fx["cross_weight"]))
    assert logits.shape == (2 * pr.N, 1, 2 * pr.H8, 2 * pr.W8) and len(grads) == 26 and trainer.pair_parts.shape == (5,)
    assert int(trainer.inside) == int(fx["inside"]) and int(trainer.stray) == 0
    assert int(trainer.valid) == int((inp["gt"] > 0).sum() + (inp["gt_aug"] > 0).sum())
    chk("loss", float(loss), fx["loss"])
    for j, name in enumerate(pr.PARTS):
        chk(name, float(trainer.pair_parts[j]), fx["parts"][j])
    for i in range(26):
        chk(f"g{i}", pr.stored(_np(grads[i])), fx[f"g{i}"])
    print(f"pair step: largest share of a bound {chk.worst[0]:.3f} ({chk.worst[1]})")
    again = trainer.pair_gradients((t["x"], t["skip"]), (t["x_aug"], t["skip_aug"]), t["gt"], t["gt_aug"], t["homography"])
    assert torch.equal(again[0], loss) and all(torch.equal(a, b) for a, b in zip(again[2], grads))
    # "last" mode on the last layer's input: the last layer's two gradients, the same bits
    feat = trainer._forward(torch.cat([t["x"], t["x_aug"]]), torch.cat([t["skip"], t["skip_aug"]]))[1]["feat"]
    last = dt.DepthHeadTrainer(stand_in(inp), train="last")
    l2, _, g2 = last.pair_gradients((feat[:pr.N], None), (feat[pr.N:], None), t["gt"], t["gt_aug"], t["homography"])
    assert torch.equal(l2, loss) and torch.equal(g2[0], grads[24]) and torch.equal(g2[1], grads[25])


def test_pair_without_cross_term_is_two_single_steps():
    from nano_vs_slam_amd import depth_training as dt
    pr, inp, stand_in, t = _pair()
    bounds = pr.bounds()
    trainer = dt.DepthHeadTrainer(stand_in(inp), train="head")
    loss, _, grads = trainer.pair_gradients((t["x"], t["skip"]), (t["x_aug"], t["skip_aug"]), t["gt"], t["gt_aug"], t["homography"], cross_weight=0.0)
    l0, _, g0 = trainer.gradients(t["x"], t["skip"], t["gt"])
    l1, _, g1 = trainer.gradients(t["x_aug"], t["skip_aug"], t["gt_aug"])
    assert _rel(float(loss), np.float64(float(l0) + float(l1))) <= bounds["loss"]
    for i in range(26):
        want = _np(g0[i]).astype(np.float64) + _np(g1[i]).astype(np.float64)
        assert _rel(_np(grads[i]), want) <= bounds[f"g{i}"], i


def test_pair_trajectory():
    from nano_vs_slam_amd import depth_training as dt
    pr, inp, stand_in, t = _pair()
    fx, chk = pr.load_fixture(), _Check(pr.bounds())
    model = stand_in(inp)
    trainer = dt.DepthHeadTrainer(model, lr=float(fx["lr"]), train="head")
    for step in range(pr.STEPS):
        versions = [p._version for p in trainer.parameters()]
        loss = trainer.step_pair_features((t["x"], t["skip"]), (t["x_aug"], t["skip_aug"]), t["gt"], t["gt_aug"], t["homography"])
        assert all(p._version == v + 1 for p, v in zip(trainer.parameters(), versions)) and trainer.steps == step + 1
        chk("loss_traj", float(loss), fx["losses_traj"][step])
        for i, p in enumerate(trainer.parameters()):
            chk(f"p{i}_traj", pr.stored(_np(p), pr.TRAJ_STORED), fx[f"p{i}_traj"][step])
    print(f"pair trajectory: largest share of a bound {chk.worst[0]:.3f} ({chk.worst[1]})")


def test_step_features_keeps_its_bits():
    """The single-view step after this change: the chained layer calls of test_gpu_depth_training._run_step, which do not pass
    through the trainer, give the bits DepthHeadTrainer.gradients gives, and an Adam step from them the same parameters."""
    import depth_training_ref as dr
    from nano_vs_slam_amd import depth_training as dt, train_ops
    from test_gpu_depth_training import _run_step, _stand_in
    inp = dr.make_inputs("A")
    r = _run_step(inp)
    model = _stand_in(inp)
    trainer = dt.DepthHeadTrainer(model, train="head")
    x, skip, gt = _dev(inp["x"]), _dev(inp["skip"]), _dev(inp["gt"])
    params = [_dev(p).clone() for p in inp["params"]]
    loss = trainer.step_features(x, skip, gt)
    assert torch.equal(loss, r["loss"]) and torch.equal(trainer.parts, r["parts"]) and trainer.pair_parts is None
    for p, g, q in zip(params, r["grads"], trainer.parameters()):
        train_ops.adam_step(p, g.view(p.shape), torch.zeros_like(p), torch.zeros_like(p), 1, trainer.lr, trainer.betas, trainer.eps)
        assert torch.equal(p, q.detach())


def test_step_pair_on_a_model():
    """view_pair -> step_pair on a config-S depth model at 64 x 96, both modes: the loss falls over three steps."""
    from conftest import product_model
    from nano_vs_slam_amd import depth_training as dt
    from oracle.weights import synthetic_frames
    model, _ = product_model("S+depth", False, 28, DEV)
    model.set_precision("fp32")
    frames = (_dev(synthetic_frames(2, 64, 96, seed=43)) + 1.0) * 0.5
    rng = np.random.default_rng(43)
    depth = _dev((0.02 + 0.04 * rng.random((2, 64, 96))).astype(np.float32))
    batch = _aug().view_pair(frames, depth=depth, d_f=2, seed=1, step=0)
    for mode in ("head", "last"):
        trainer = dt.DepthHeadTrainer(model, lr=1e-4, train=mode)
        losses = [float(trainer.step_pair(batch["image"], batch["image_aug"], batch["depth"], batch["depth_aug"], batch["homography"]))
                  for _ in range(3)]
        print(f"step_pair {mode}: losses {losses}, parts {trainer.pair_parts.tolist()}, inside {int(trainer.inside)}")
        assert losses[2] < losses[0] and trainer.steps == 3 and trainer.pair_parts.shape == (5,)
    with pytest.raises(ValueError):
        trainer.step_pair(batch["image"].cpu(), batch["image_aug"], batch["depth"], batch["depth_aug"], batch["homography"])
    with pytest.raises(ValueError):
        trainer.step_pair(batch["image"], batch["image_aug"], batch["depth"], batch["depth_aug"][:1], batch["homography"])
