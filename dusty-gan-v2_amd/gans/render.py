"""Bird's-eye-view rendering of point clouds (reference: gans/render.py:6-127), without kornia.

render_point_clouds and bilinear_rasterizer keep the reference's signatures and run on the splat kernels of
csrc/bev.hip (native.bev_render / native.bilinear_splat: three launches, 64-bit integer sums, the same bits on every
run and for every order of the points).  make_Rt is plain torch.  There is no CPU fallback
(package policy): CPU tensors raise."""
import math

import torch

from gans.models.ops import native


def make_Rt(roll=0, pitch=0, yaw=0, x=0, y=0, z=0, device="cpu"):
    """R [1,3,3] = Rz(yaw) . Ry(pitch) . Rx(roll), the right-handed rotations about the axes (what kornia's axis-angle
    conversion gives for an axis-aligned vector), and t [1,3] (reference: render.py:6-18)."""
    cr, sr = math.cos(roll), math.sin(roll)
    cp, sp = math.cos(pitch), math.sin(pitch)
    cy, sy = math.cos(yaw), math.sin(yaw)
    Rz = torch.tensor([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    Ry = torch.tensor([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]], dtype=torch.float64)
    Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]], dtype=torch.float64)
    R = (Rz @ Ry @ Rx).float()[None].to(device)
    t = torch.tensor([[x, y, z]], dtype=torch.float32, device=device)
    return R, t


def _pow2_bound(values):
    """The smallest power of two >= max |values| (1 for all zeros), as a 0-dim device tensor: dividing by it is exact and
    brings every value into the kernels' [-1, 1]; nothing is read back."""
    mantissa, exponent = torch.frexp(values.detach().abs().amax().float())   # max = m * 2^e with m in [0.5, 1)
    exponent = exponent - (mantissa == 0.5).to(exponent.dtype)               # a power of two is its own bound
    return torch.ldexp(torch.ones((), device=values.device), exponent)


def _one(name, v, shape):
    """An extrinsic shared by the batch: `shape` or [1, *shape]."""
    if v is None:
        return None
    if v.ndim == len(shape) + 1 and v.shape[0] == 1:
        v = v[0]
    if tuple(v.shape) != tuple(shape):
        raise ValueError(f"render_point_clouds: {name} must be {list(shape)} or {[1, *shape]} (one for the whole batch), "
                         f"got {list(v.shape)}")
    return v


def render_point_clouds(points, colors, size=512, R=None, t=None, focal_length=1.0):
    """points [B,N,3] (x, y, z; the camera looks down -z), colors [B,N,C] with C <= 4 -> the splatted view
    [B,C,size,size] (reference: render.py:21-67): pinhole projection with principal point 0.5, exp(-3 |p|) depth weights,
    bilinear splat, normalisation by the splatted weights.  R [3,3] or [1,3,3] and t [3] or [1,3] are shared by the
    batch.  `points` is not modified."""
    if colors.ndim != 3 or colors.shape[-1] > native.BEV_C_MAX or colors.numel() == 0:
        raise ValueError(f"render_point_clouds: colors must be a non-empty [B,N,C] with C <= {native.BEV_C_MAX}, "
                         f"got {list(colors.shape)}")
    R, t = _one("R", R, (3, 3)), _one("t", t, (3,))
    bound = _pow2_bound(colors)
    return native.bev_render(points, colors / bound, size, R, t, focal_length) * bound


def bilinear_rasterizer(coords, values, out_shape):
    """coords [B,N,2] = (row, col), values [B,N,C] -> [B,C,H,W]: every value spread over the four pixels around its
    coordinate (reference: render.py:70-127)."""
    if values.ndim != 3 or values.numel() == 0:
        raise ValueError(f"bilinear_rasterizer: values must be a non-empty [B,N,C], got {list(values.shape)}")
    bound = _pow2_bound(values)
    return native.bilinear_splat(coords, values / bound, out_shape) * bound
