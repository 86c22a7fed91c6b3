"""native.render: the bird's-eye-view splat of gans/render.py (reference: gans/render.py:21-127) on dgv2_bev_render and
dgv2_bilinear_splat (include/dgv2.h states the arithmetic, DESIGN.md section 37 the kernel).

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI, see the package docstring).  Forward only, float32.
Each call is three launches (clear, splat, resolve) whose output is bit-identical from run to run and under any
permutation of the points: the sums are 64-bit integers.  The accumulator is allocated here, per call, from torch's
caching allocator; its shape is the header's formula.
"""
import torch

import dgv2_native as N

BEV_C_MAX = 4
BEV_N_MAX = 2 ** 22   # exclusive: N * 2^40 must stay below 2^63


def _f32(name, t, shape):
    if t is None or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {None if t is None else tuple(t.shape)}")
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _check_sizes(what, B, n, C, *image):
    if not 1 <= C <= BEV_C_MAX:
        raise ValueError(f"{what}: {C} channels are outside the kernel's range (1 .. {BEV_C_MAX})")
    if min(B, n, *image) < 1:
        raise ValueError(f"{what}: empty input (B {B}, N {n}, image {image})")
    if n >= BEV_N_MAX:
        raise ValueError(f"{what}: {n} points per sample; the 64-bit sums hold fewer than {BEV_N_MAX}")


def bev_render(points, colors, size, R=None, t=None, focal=1.0):
    """points [B,N,3], colors [B,N,C] (1 <= C <= 4, values in [-1, 1]: an addend beyond saturates), R [3,3] or None,
    t [3] or None -> [B,C,size,size] float32 (dgv2_bev_render).  `points` is read, never written.  ValueError outside the
    kernel's range or for mismatched shapes; RuntimeError for CPU tensors."""
    if points.ndim != 3 or points.shape[-1] != 3:
        raise ValueError(f"bev_render: points must be [B,N,3], got {tuple(points.shape)}")
    if colors.ndim != 3 or colors.shape[:2] != points.shape[:2]:
        raise ValueError(f"bev_render: colors must be [B,N,C] over the same points, got {tuple(colors.shape)}")
    B, n, C = colors.shape
    size = int(size)
    _check_sizes("bev_render", B, n, C, size)
    points, colors = _f32("points", points, (B, n, 3)), _f32("colors", colors, (B, n, C))
    R = None if R is None else _f32("R", R, (3, 3))
    t = None if t is None else _f32("t", t, (3,))
    N.check(points, colors, R, t)
    out = torch.empty(B, C, size, size, device=points.device, dtype=torch.float32)
    acc = torch.empty(B, size, size, C + 1, device=points.device, dtype=torch.int64)
    N.call("dgv2_bev_render", N.ptr(out), N.ptr(acc), N.ptr(points), N.ptr(colors), N.ptr(R), N.ptr(t), B, n, C, size,
           float(focal), N.stream())
    return out


def bilinear_splat(coords, values, out_shape):
    """coords [B,N,2] = (row, col), values [B,N,C] (1 <= C <= 4, in [-1, 1]) -> [B,C,H,W] float32: every value spread
    over the four pixels around its coordinate with bilinear weights; a corner outside the image or with a weight below
    1e-3 is dropped (dgv2_bilinear_splat)."""
    if coords.ndim != 3 or coords.shape[-1] != 2:
        raise ValueError(f"bilinear_splat: coords must be [B,N,2], got {tuple(coords.shape)}")
    if values.ndim != 3 or values.shape[:2] != coords.shape[:2]:
        raise ValueError(f"bilinear_splat: values must be [B,N,C] over the same points, got {tuple(values.shape)}")
    B, n, C = values.shape
    H, W = (int(s) for s in out_shape)
    _check_sizes("bilinear_splat", B, n, C, H, W)
    coords, values = _f32("coords", coords, (B, n, 2)), _f32("values", values, (B, n, C))
    N.check(coords, values)
    out = torch.empty(B, C, H, W, device=coords.device, dtype=torch.float32)
    acc = torch.empty(B, H, W, C, device=coords.device, dtype=torch.int64)
    N.call("dgv2_bilinear_splat", N.ptr(out), N.ptr(acc), N.ptr(coords), N.ptr(values), B, n, C, H, W, N.stream())
    return out


__all__ = ["bev_render", "bilinear_splat", "BEV_C_MAX", "BEV_N_MAX"]
