"""native.frame: post-processing of generated frames (reference: demo_interpolation.py:20-34, 79-86): range image ->
point cloud + normal colours in one launch, and the colour lookup of gans.utils.colorize.

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI, see the package docstring).  Inference only: none of
these records a gradient.
"""
import torch

import dgv2_native as N

BORDERS = {"zeros": 0, "ring": 1}


def frame_points(image, angle, min_depth, max_depth, border="zeros"):
    """image [B,1,H,W] (the generator's "image", [-1,1]), angle [1,2,H,W] -> (points, colors), each [B,H*W,3]:
    3x3-median-filtered points / max_depth and their normal colours (dgv2_frame_points, include/dgv2.h)."""
    if border not in BORDERS:
        raise ValueError(f"frame_points: border must be one of {sorted(BORDERS)}, got {border!r}")
    if image.ndim != 4 or image.shape[1] != 1:
        raise ValueError(f"frame_points: expected a [B,1,H,W] image batch, got {tuple(image.shape)}")
    B, _, H, W = image.shape
    if tuple(angle.shape) != (1, 2, H, W):
        raise ValueError(f"frame_points: angle must be [1,2,{H},{W}], got {tuple(angle.shape)}")
    image = image.detach().float().contiguous()
    angle = angle.detach().float().contiguous()
    N.check(image, angle)
    points = torch.empty((B, H * W, 3), device=image.device, dtype=torch.float32)
    colors = torch.empty_like(points)
    N.call("dgv2_frame_points", N.ptr(points), N.ptr(colors), N.ptr(image), N.ptr(angle), B, H, W, float(min_depth),
           float(max_depth), BORDERS[border], N.stream())
    return points, colors


def colorize_lut(x, lut):
    """x [B,H,W] fp32, lut [n,3] fp32 -> [B,3,H,W] = lut[(long) clamp(x * n, 0, n - 1)] (dgv2_colorize)."""
    B, H, W = x.shape
    x = x.detach().float().contiguous()
    lut = lut.detach().float().contiguous()
    if lut.ndim != 2 or lut.shape[1] != 3:
        raise ValueError(f"colorize_lut: lut must be [n,3], got {tuple(lut.shape)}")
    N.check(x, lut)
    out = torch.empty((B, 3, H, W), device=x.device, dtype=torch.float32)
    N.call("dgv2_colorize", N.ptr(out), N.ptr(x), N.ptr(lut), B, H, W, lut.shape[0], N.stream())
    return out


__all__ = ["frame_points", "colorize_lut"]
