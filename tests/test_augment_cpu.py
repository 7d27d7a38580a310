"""The view-pair oracle (tests/augment_ref.py) held to what pins it, without a GPU: the sampler to the reference's own
sample_homography through the fixtures of tools/make_augment_golden.py; the warp to torch's grid_sample(align_corners=True,
padding_mode="zeros") in float64, forward and autograd backward (bit for bit in nearest mode, 1e-12 in bilinear); the backward
to the transpose of the forward; the draw function to its stated counter layout; and the header, the SOURCES list and the
bindings to each other.  The GPU tests (tests/test_gpu_augment.py) then hold the device to this oracle."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as ar
from conftest import ROOT


# ---- the sampler -----------------------------------------------------------------------------------------------------------------
def test_oracle_reproduces_the_reference_sampler():
    fx, cases = ar.load_sampler(), ar.sampler_cases()
    assert len(cases) == 7 and {tuple(c["shape"]) for c in cases.values()} == {(120, 160), (240, 320), (100, 100)}
    assert sorted(k for c in cases.values() for k in c["options"]) == ["perspective", "rotation", "scaling", "translation"]
    for name, case in cases.items():
        draws, homs = fx["draws_" + name], fx["hom_" + name]
        assert draws.shape == (16, 9) and homs.shape == (16, 3, 3)
        margins = []
        for d, h in zip(draws, homs):
            got = ar.sample_homography(d, case["shape"], margins=margins, **case["options"])
            assert np.abs(got - h).max() <= 1e-9, name
            corners = ar.view_corners(h)                         # every sampled view stays inside the image
            assert (np.abs(corners) <= 1.0 + 1e-12).all(), name
        assert min(margins) > 1e-9, name                         # no discrete choice of a kept seed is in doubt


# ---- the warp against torch ------------------------------------------------------------------------------------------------------
def _torch_pair(x, hom, mode):
    H, W = x.shape[2:]
    un, vn = ar.grid(hom, H, W)
    g = torch.from_numpy(np.stack([un, vn], -1))[None].expand(x.shape[0], H, W, 2)
    xt = torch.from_numpy(x).requires_grad_(True)
    return xt, F.grid_sample(xt, g, mode=mode, padding_mode="zeros", align_corners=True)


@pytest.mark.parametrize("name", ["halves", "general", "sampled"])
def test_oracle_agrees_with_grid_sample(name):
    hom, (H, W) = {"halves": (ar.HALVES, (9, 17)), "general": (ar.GENERAL, (17, 23)), "sampled": (ar.reference_homography((17, 23)), (17, 23))}[name]
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, 3, H, W))
    xt, y = _torch_pair(x, hom, "nearest")
    assert np.array_equal(y.detach().numpy(), ar.warp(x, hom, fill=0.0))
    dy = rng.standard_normal(y.shape)
    y.backward(torch.from_numpy(dy))
    assert np.array_equal(xt.grad.numpy(), ar.warp_backward(dy, hom, (H, W), dtype=np.float64))
    _, yb = _torch_pair(x, hom, "bilinear")
    assert np.abs(yb.detach().numpy() - ar.warp(x, hom, mode="bilinear")).max() <= 1e-12
    inside = ar.nearest(hom, H, W)[0]
    if name == "general":
        assert round(100 * (1 - inside.mean())) == 22
    if name == "halves":                                         # every coordinate is an exact half: the tie rule decides all
        px, py = ar.src_coords(hom, H, W)
        assert (px - np.floor(px) == 0.5).all() and (py - np.floor(py) == 0.5).all()


def test_stride_is_the_full_warp_subsampled():
    rng = np.random.default_rng(8)
    x = rng.integers(0, 255, (2, 1, 32, 48)).astype(np.uint8)
    for hom in (ar.GENERAL, ar.reference_homography((32, 48))):
        assert np.array_equal(ar.warp(x, hom, fill=255, stride=4), ar.warp(x, hom, fill=255)[:, :, ::4, ::4])


@pytest.mark.parametrize("stride", [1, 4])
def test_backward_is_the_transpose_of_the_forward(stride):
    rng = np.random.default_rng(9)
    H, W = 32, 48
    for hom in (ar.GENERAL, ar.ZOOM_IN, ar.reference_homography((H, W))):
        x = rng.standard_normal((2, 2, H, W))
        dy = rng.standard_normal((2, 2, H // stride, W // stride))
        lhs = (ar.warp(x, hom, fill=0.0, stride=stride) * dy).sum()
        rhs = (x * ar.warp_backward(dy, hom, (H, W), stride, dtype=np.float64)).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_full_scan_case_counts():
    """The 6 x 8 case of the backward's slow path: forward w' > 0 on the whole grid, 31 inside pixels, 92 source corners whose
    inverse w' is <= 0."""
    h = ar.FULL_SCAN
    gx, gy = 2.0 * np.arange(8) / 7 - 1.0, 2.0 * np.arange(6) / 5 - 1.0
    assert (h[2, 0] * gx[None] + h[2, 1] * gy[:, None] + h[2, 2] > 0).all()
    assert int(ar.nearest(h, 6, 8)[0].sum()) == 31
    assert int((ar.inverse_corner_w(h, 6, 8) <= 0).sum()) == 92
    assert ar.fan_in(ar.ZOOM_IN, 17, 23).max() >= 4 and (ar.fan_in(ar.ZOOM_IN, 17, 23) == 0).any()


def test_cross_view_oracle_against_autograd():
    rng = np.random.default_rng(10)
    N, H, W = 2, 16, 24
    depth, aug = rng.random((N, H, W)), rng.random((N, H, W))
    homs = np.stack([ar.GENERAL, ar.reference_homography((H, W))])
    a, b = torch.from_numpy(depth).requires_grad_(True), torch.from_numpy(aug).requires_grad_(True)
    g = torch.from_numpy(np.stack([np.stack(ar.grid(h, H, W), -1) for h in homs]))
    warped = F.grid_sample(a[:, None], g, mode="nearest", padding_mode="zeros", align_corners=True)[:, 0]
    loss = 0.5 * F.mse_loss(b, warped)
    loss.backward()
    ref = ar.cross_view_mse(depth, aug, homs, 0.5)
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-14
    assert np.abs(ref["d_depth"] - a.grad.numpy()).max() <= 1e-15 and np.abs(ref["d_depth_aug"] - b.grad.numpy()).max() <= 1e-15
    only = ar.cross_view_mse(depth, aug, homs, 0.5, inside_only=True)
    assert 0 < only["inside"] == ref["inside"] < N * H * W and only["loss"] != ref["loss"]


# ---- the draws -------------------------------------------------------------------------------------------------------------------
def test_draw_layout():
    """h = mix(mix(mix(seed + golden) ^ (step << 32 | frame)) ^ (slot << 32 | k)): every counter moves the value, the fields
    do not alias, uniforms are (h >> 11) 2^-53, normals Box-Muller."""
    assert ar.mix(0) == 0 and ar.mix(1) == 0x5692161D100B05E5          # splitmix64's finaliser
    base = ar.draw_hash(3, 5, 7, 2, 0)
    assert base == ar.mix(ar.mix(ar.mix(3 + 0x9E3779B97F4A7C15) ^ ((5 << 32) | 7)) ^ (2 << 32))
    others = {ar.draw_hash(4, 5, 7, 2, 0), ar.draw_hash(3, 6, 7, 2, 0), ar.draw_hash(3, 5, 8, 2, 0), ar.draw_hash(3, 5, 7, 3, 0),
              ar.draw_hash(3, 5, 7, 2, 1), ar.draw_hash(3, 7, 5, 2, 0), ar.draw_hash(3, 5, 2, 7, 0)}
    assert len(others) == 7 and base not in others
    d = ar.homography_draws(64, seed=11, step=2)
    assert d.shape == (64, 9) and np.isfinite(d).all()
    uni = d[:, [4, 6, 7, 8]]
    assert (uni >= 0).all() and (uni < 1).all() and abs(uni.mean() - 0.5) < 0.06
    nrm = d[:, list(ar.NORMAL_SLOTS)]
    assert abs(nrm.mean()) < 0.15 and 0.8 < nrm.std() < 1.2
    assert d[3, 4] == (ar.draw_hash(11, 2, 3, 4, 0) >> 11) * 2.0 ** -53
    assert not np.array_equal(d, ar.homography_draws(64, seed=11, step=3))
    homs = ar.sample_homographies(d, (120, 160))                         # the library's own stream gives views inside the image too
    assert all((np.abs(ar.view_corners(h)) <= 1.0 + 1e-12).all() for h in homs)


# ---- header, sources, bindings ---------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("kp2d_homography_draws", "kp2d_homography_sample", "kp2d_warp", "kp2d_warp_backward", "kp2d_cross_view_scratch_bytes",
               "kp2d_cross_view_mse")


def test_header_sources_and_bindings_agree():
    from nano_vs_slam_amd import _lib
    text = open(os.path.join(ROOT, "include", "kp2d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in NEW_SYMBOLS:
        m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % sym, code, flags=re.S)
        assert m, sym
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[sym][1]), sym
    for name, value in (("KP2D_WARP_TILE_W", ar.TILE_W), ("KP2D_WARP_TILE_H", ar.TILE_H), ("KP2D_HOMOGRAPHY_DRAWS", ar.SLOTS)):
        assert re.search(r"#define %s %d\b" % (name, value), code), name
    import __graft_entry__ as g
    assert "augment.hip" in g._load_build_module().SOURCES
    src = open(os.path.join(ROOT, "nano-vs-slam_amd", "csrc", "augment.hip")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, src), sym
    from nano_vs_slam_amd import augment
    assert augment.DRAWS == ar.SLOTS and augment._SAMPLER == ar.DEFAULTS


def test_cpu_tensors_are_refused():
    from nano_vs_slam_amd import augment
    x, hom = torch.zeros(1, 1, 4, 4), torch.eye(3)[None]
    with pytest.raises(ValueError):
        augment.warp(x, hom)
    with pytest.raises(ValueError):
        augment.warp_backward(x, hom, (4, 4))
    with pytest.raises(ValueError):
        augment.cross_view_mse(x[:, 0], x[:, 0], hom)
    with pytest.raises(ValueError):
        augment.sample_homographies(1, (4, 4), draws=torch.zeros(1, 9, dtype=torch.float64))
    with pytest.raises(ValueError):
        augment.view_pair(x)
