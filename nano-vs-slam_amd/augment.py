"""View pairs on the device: what the reference's dataset transforms do between "a batch of frames" and the batch its losses
read (``image, image_aug, seg, seg_aug, depth, depth_aug, homography``; src/data/dataset_utils.py:9-136 and :198-266,
nyuv2.py:183-257), on the HIP kernels of csrc/augment.hip (include/kp2d.h states every formula).

* ``homography_draws`` / ``sample_homographies`` — the reference's ``sample_homography``, one thread per frame in double.  The
  randomness enters through ``draws`` [B, 9] (float64), so the reference's own function, fed the same draws, pins the kernel;
  ``homography_draws`` fills them from the library's counter stream (not numpy's: the stated deviation of k-means, mining and
  dropout).
* ``warp`` — ``tgm.HomographyWarper(H, W, mode=...)(x, hom)`` as the reference uses it, i.e.
  ``grid_sample(x, hom · grid, align_corners=True, padding_mode="zeros")``; with ``stride`` the nearest ``Resize`` to
  ``1 / stride`` that follows it in the reference, in the same launch.  float32, uint8, int32 and int64 sources.
* ``warp_backward`` — the gradient of the nearest warp, added in a fixed order without atomics.
* ``cross_view_mse`` — the depth head's cross-view term ``weight · MSE(depth_aug, warp(depth, hom))`` with both gradients.
* ``view_pair`` — the whole stage: one call from frames, labels and depth to the reference's batch.

The meaning of ``warper(x, H)`` and ``align_corners=True`` is read from the reference's use of torchgeometry, not run against
it (torchgeometry is not a dependency).  Not built: the photometric half of the transforms (ColorJitter, GaussianBlur,
RandomGrayscale, RandomEqualize), image decoding and resizing from files, the bilinear warp's backward.

There is no CPU path: CPU tensors raise ValueError.
"""
from __future__ import annotations

import math

import torch

from . import _dev, _lib
from ._dev import ptr as _ptr, stream as _stream

DRAWS = 9            # KP2D_HOMOGRAPHY_DRAWS: z0, z1, z2, z3, u_s, z_s, u_x, u_y, u_r
_DTYPES = {torch.float32: 0, torch.uint8: 1, torch.int32: 2, torch.int64: 3}     # KP2D_WARP_F32 / _U8 / _I32 / _I64
_MODES = {"nearest": 0, "bilinear": 1}                                            # KP2D_WARP_NEAREST / _BILINEAR
_SAMPLER = dict(perspective=True, scaling=True, rotation=True, translation=True, n_scales=100, n_angles=100, scaling_amplitude=0.2,
                perspective_amplitude=0.2, patch_ratio=0.7, max_angle=math.pi / 2)      # the reference's defaults


def _device_tensor(where, name, t):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"{where}: {name} must be a device tensor (there is no CPU path)")
    return t


def _device_of(device):
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise ValueError(f"augment: device {dev} is not a GPU (there is no CPU path)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _check_hom(where, hom, N, device):
    """-> (contiguous hom, hom_f64)"""
    _device_tensor(where, "homography", hom)
    if hom.dtype not in (torch.float32, torch.float64) or tuple(hom.shape) != (N, 3, 3):
        raise ValueError(f"{where}: homography must be float32 or float64 [{N}, 3, 3], got {hom.dtype} {tuple(hom.shape)}")
    if hom.device != device:
        raise ValueError(f"{where}: every tensor of a call must live on one device")
    return hom.contiguous(), int(hom.dtype == torch.float64)


def _check_size(where, N, H, W, stride):
    if not (1 <= N <= 65535):
        raise ValueError(f"{where}: needs 1 <= N <= 65535, got {N}")
    if H < 2 or W < 2:
        raise ValueError(f"{where}: the source map must be at least 2 x 2, got {H} x {W}")
    if not isinstance(stride, int) or stride < 1 or H % stride or W % stride:
        raise ValueError(f"{where}: stride {stride} must be a positive integer that divides {H} x {W}")


def homography_draws(B, seed=0, step=0, device=None):
    """-> float64 [B, 9]: per frame z0..z3, u_s, z_s, u_x, u_y, u_r from the library's counter stream at (seed, step)."""
    dev = _device_of(device)
    B, seed, step = int(B), int(seed), int(step)
    if B < 1 or not (0 <= step < 2 ** 32) or not (0 <= seed < 2 ** 64):
        raise ValueError(f"homography_draws: needs B >= 1, 0 <= step < 2^32, 0 <= seed < 2^64, got B {B}, step {step}, seed {seed}")
    draws = torch.empty(B, DRAWS, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().kp2d_homography_draws(_ptr(draws), B, seed, step, _stream(dev)))
    return draws


def sample_homographies(B, shape, seed=0, step=0, device=None, draws=None, dtype=torch.float32, **options):
    """The reference's ``sample_homography(shape)`` for B frames -> [B, 3, 3] of ``dtype`` (float32: what the reference feeds its
    warper and its losses; float64: before that rounding).  ``draws`` [B, 9] float64 injects the randomness (else
    ``homography_draws(B, seed, step)``); ``options``: perspective, scaling, rotation, translation, n_scales, n_angles,
    scaling_amplitude, perspective_amplitude, patch_ratio, max_angle, with the reference's defaults."""
    where = "sample_homographies"
    unknown = set(options) - set(_SAMPLER)
    if unknown:
        raise ValueError(f"{where}: unknown options {sorted(unknown)}")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{where}: dtype must be torch.float32 or torch.float64, got {dtype}")
    o = dict(_SAMPLER, **options)
    B, (H, W) = int(B), (int(v) for v in shape)
    if draws is None:
        draws = homography_draws(B, seed, step, device)
    else:
        _device_tensor(where, "draws", draws)
        if draws.dtype != torch.float64 or tuple(draws.shape) != (B, DRAWS):
            raise ValueError(f"{where}: draws must be float64 [{B}, {DRAWS}], got {draws.dtype} {tuple(draws.shape)}")
        draws = draws.contiguous()
    dev = draws.device
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"{where}: needs B >= 1 and a shape of positive extents, got B {B}, shape {(H, W)}")
    hom = torch.empty(B, 3, 3, dtype=dtype, device=dev)
    h64, h32 = (hom, None) if dtype == torch.float64 else (None, hom)
    _lib.check(_lib.load().kp2d_homography_sample(
        _ptr(draws), B, H, W, int(bool(o["perspective"])), int(bool(o["scaling"])), int(bool(o["rotation"])), int(bool(o["translation"])),
        int(o["n_scales"]), int(o["n_angles"]), float(o["scaling_amplitude"]), float(o["perspective_amplitude"]), float(o["patch_ratio"]),
        float(o["max_angle"]), _ptr(h64), _ptr(h32), _stream(dev)))
    return hom


def warp(x, hom, mode="nearest", fill=0, stride=1):
    """x [N, C, H, W] (or [N, H, W]) float32, uint8, int32 or int64; hom [N, 3, 3] float32 or float64 -> the warped map
    [N, C, H / stride, W / stride] of x's type: ``out(q) = x(hom · q)`` in normalised coordinates, the pixel of the full-size
    grid at ``q · stride``.  ``mode="nearest"``: ties to even, outside pixels get ``fill``; ``mode="bilinear"`` (float32
    only): taps outside the map count as zero."""
    where = "warp"
    _device_tensor(where, "x", x)
    if x.dtype not in _DTYPES or x.dim() not in (3, 4):
        raise ValueError(f"{where}: x must be float32, uint8, int32 or int64 [N, C, H, W] or [N, H, W], got {x.dtype} {tuple(x.shape)}")
    if mode not in _MODES:
        raise ValueError(f"{where}: mode must be 'nearest' or 'bilinear', got {mode!r}")
    if mode == "bilinear" and x.dtype != torch.float32:
        raise ValueError(f"{where}: bilinear takes float32 sources only, got {x.dtype}")
    x4 = x if x.dim() == 4 else x[:, None]
    N, C, H, W = x4.shape
    _check_size(where, N, H, W, stride)
    if C < 1:
        raise ValueError(f"{where}: x has no channel")
    hom, f64 = _check_hom(where, hom, N, x.device)
    fill = float(fill)
    if math.isnan(fill):
        raise ValueError(f"{where}: fill must not be NaN")
    if x.dtype != torch.float32 and not (math.isfinite(fill) and fill == math.floor(fill) and
                                         torch.iinfo(x.dtype).min <= fill <= torch.iinfo(x.dtype).max and abs(fill) <= 2.0 ** 53):
        raise ValueError(f"{where}: fill {fill} is not a value of {x.dtype}")
    x4 = x4.contiguous()
    out = torch.empty(N, C, H // stride, W // stride, dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().kp2d_warp(_ptr(x4), _DTYPES[x.dtype], _ptr(hom), f64, N, C, H, W, stride, _MODES[mode], fill, _ptr(out),
                                     _stream(x.device)))
    return out if x.dim() == 4 else out[:, 0]


def warp_backward(dy, hom, size, stride=1):
    """dy float32 [N, C, H / stride, W / stride] (or without C), the gradient of ``warp(x, hom, "nearest", stride=stride)``'s
    output; size = (H, W) of x -> dx [N, C, H, W]: per source pixel the sum of dy over the outputs that read it, added in
    ascending row-major order in float32 (bit-identical from run to run; no atomics)."""
    where = "warp_backward"
    _device_tensor(where, "dy", dy)
    if dy.dtype != torch.float32 or dy.dim() not in (3, 4):
        raise ValueError(f"{where}: dy must be float32 [N, C, Ho, Wo] or [N, Ho, Wo], got {dy.dtype} {tuple(dy.shape)}")
    d4 = dy if dy.dim() == 4 else dy[:, None]
    N, C = d4.shape[:2]
    H, W = (int(v) for v in size)
    _check_size(where, N, H, W, stride)
    if C < 1 or tuple(d4.shape[2:]) != (H // stride, W // stride):
        raise ValueError(f"{where}: dy must be [N, C, {H // stride}, {W // stride}] for size {(H, W)} at stride {stride}, got {tuple(dy.shape)}")
    hom, f64 = _check_hom(where, hom, N, dy.device)
    d4 = d4.contiguous()
    dx = torch.empty(N, C, H, W, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.load().kp2d_warp_backward(_ptr(d4), _ptr(hom), f64, N, C, H, W, stride, _ptr(dx), _stream(dy.device)))
    return dx if dy.dim() == 4 else dx[:, 0]


def cross_view_mse(depth, depth_aug, hom, weight=0.5, inside_only=False, scratch=None):
    """depth, depth_aug float32 [N, H, W] or [N, 1, H, W] (after the sigmoid), hom [N, 3, 3] -> (loss, d_depth, d_depth_aug,
    inside): the reference's ``weight · MSE(depth_aug, warp(depth, hom))`` (nearest, outside pixels 0), its gradients shaped
    like the inputs, and the int64 device scalar of inside pixels.  ``inside_only=True`` restricts the mean and both gradients
    to the inside pixels (none: loss 0, gradients 0); False is the reference, where an outside pixel pulls ``depth_aug``
    towards 0."""
    where = "cross_view_mse"
    for name, t in (("depth", depth), ("depth_aug", depth_aug)):
        _device_tensor(where, name, t)
        if t.dtype != torch.float32 or not (t.dim() == 3 or (t.dim() == 4 and t.shape[1] == 1)):
            raise ValueError(f"{where}: {name} must be float32 [N, H, W] or [N, 1, H, W], got {t.dtype} {tuple(t.shape)}")
    if depth.shape != depth_aug.shape or depth.device != depth_aug.device:
        raise ValueError(f"{where}: depth {tuple(depth.shape)} and depth_aug {tuple(depth_aug.shape)} must have one shape and one device")
    N, H, W = depth.shape[0], depth.shape[-2], depth.shape[-1]
    _check_size(where, N, H, W, 1)
    hom, f64 = _check_hom(where, hom, N, depth.device)
    weight = float(weight)
    if not (0.0 <= weight < float("inf")):
        raise ValueError(f"{where}: weight must be finite and >= 0, got {weight}")
    lib = _lib.load()
    dev = depth.device
    if scratch is None:
        nbytes = int(lib.kp2d_cross_view_scratch_bytes(N, H * W))
        if nbytes == 0:
            raise ValueError(f"{where}: maps {tuple(depth.shape)} are not supported")
        scratch = _dev.scratch(nbytes, dev)
    a, b = depth.contiguous(), depth_aug.contiguous()
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    inside = torch.empty(1, dtype=torch.int64, device=dev)
    da, db = torch.empty_like(a), torch.empty_like(b)
    _lib.check(lib.kp2d_cross_view_mse(_ptr(a), _ptr(b), _ptr(hom), f64, N, H, W, weight, int(bool(inside_only)), _ptr(loss), _ptr(da),
                                       _ptr(db), _ptr(inside), _ptr(scratch), scratch.numel(), _stream(dev)))
    return loss[0], da, db, inside[0]


def view_pair(frames, seg=None, depth=None, d_f=4, seed=0, step=0, homography=None, draws=None, **options):
    """frames float32 [N, 3, H, W] in [0, 1]; seg labels [N, H, W] (uint8, int32 or int64) and depth float32 [N, H, W] at the
    frames' size, both optional -> the reference's batch: ``image`` and ``image_aug`` in [-1, 1] (the reference's order: warp
    in [0, 1], zeros outside, then ``· 2 - 1``, so outside pixels are -1), ``seg``, ``seg_aug``, ``depth``, ``depth_aug`` at
    ``1 / d_f`` of the size (the warp at full size and the nearest Resize in one strided launch; the plain targets by the
    same call with unit homographies; outside labels and depth are 0), and ``homography`` float32 [N, 3, 3], the very matrix
    the warps used.  ``homography`` (or ``draws``, or seed and step) chooses the views; ``options`` go to the sampler."""
    where = "view_pair"
    _device_tensor(where, "frames", frames)
    if frames.dtype != torch.float32 or frames.dim() != 4:
        raise ValueError(f"{where}: frames must be float32 [N, C, H, W], got {frames.dtype} {tuple(frames.shape)}")
    N, _, H, W = frames.shape
    dev = frames.device
    if homography is None:
        homography = sample_homographies(N, (H, W), seed=seed, step=step, device=dev, draws=draws, **options)
    elif homography.dtype != torch.float32:
        raise ValueError(f"{where}: homography must be float32 (what the losses take), got {homography.dtype}")
    image = frames.contiguous() * 2.0 - 1.0
    out = {"image": image, "image_aug": warp(image, homography, "nearest", fill=-1.0), "homography": homography}
    unit = None
    for key, t in (("seg", seg), ("depth", depth)):
        if t is None:
            continue
        _device_tensor(where, key, t)
        if tuple(t.shape) not in ((N, H, W), (N, 1, H, W)):
            raise ValueError(f"{where}: {key} must have the frames' size {(N, H, W)}, got {tuple(t.shape)}")
        if unit is None:
            unit = torch.eye(3, dtype=torch.float32, device=dev).expand(N, 3, 3).contiguous()
        out[key] = warp(t, unit, "nearest", fill=0, stride=d_f)
        out[key + "_aug"] = warp(t, homography, "nearest", fill=0, stride=d_f)
    return out
