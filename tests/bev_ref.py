"""Restatement, in plain torch, of what csrc/bev.hip computes (include/dgv2.h "Bird's-eye view"; reference:
gans/render.py:6-127, gans/utils.py:205-209), written from the contract and run in float64 as the tests' reference; in
float32 on the device it is also the tensor-op form that scripts/mb_bev.py times the kernels against.

render() also says which points are FRAGILE: so close to one of the contract's decision edges that float32 and float64
may legitimately decide differently (another corner, another side of the image border, a weight kept or dropped)."""
import math

import torch

W_MIN = 1e-3
EPS = 1e-8


def make_Rt(roll=0.0, pitch=0.0, yaw=0.0, x=0.0, y=0.0, z=0.0, dtype=torch.float64):
    """R [1,3,3] = Rz(yaw) Ry(pitch) Rx(roll) by Rodrigues' formula about the unit axes, t [1,3]."""
    def about(axis, angle):
        k = torch.zeros(3, 3, dtype=torch.float64)
        a = [0.0, 0.0, 0.0]
        a[axis] = 1.0
        k[0, 1], k[0, 2], k[1, 0], k[1, 2], k[2, 0], k[2, 1] = -a[2], a[1], a[2], -a[0], -a[1], a[0]
        return torch.eye(3, dtype=torch.float64) + math.sin(angle) * k + (1 - math.cos(angle)) * (k @ k)
    R = about(2, yaw) @ about(1, pitch) @ about(0, roll)
    return R[None].to(dtype), torch.tensor([[x, y, z]], dtype=dtype)


def power_spectrum_2d(x):
    """10 log10 |F|^2 of the forward-normalised, centred 2-D DFT, by two explicit DFT matrices in float64."""
    x = x.double()
    H, W = x.shape[-2:]

    def dft(n):
        k = torch.arange(n, dtype=torch.float64)
        ang = -2 * math.pi * torch.outer(k, k) / n
        return torch.complex(ang.cos(), ang.sin()) / n
    F = dft(H) @ x.to(torch.complex128) @ dft(W).T
    F = torch.roll(F, shifts=(H // 2, W // 2), dims=(-2, -1))
    return 10 * torch.log10(F.real ** 2 + F.imag ** 2)


def project(points, size, R=None, t=None, focal=1.0):
    """Steps 1-5 of the contract in points' dtype: dict(row, col, keep, e, ux, uy), each [B,N]."""
    p = points * points.new_tensor([1.0, 1.0, -1.0])
    if R is not None:
        p = p @ R.to(p).reshape(3, 3)
    if t is not None:
        p = p + t.to(p).reshape(3)
    pz = p[..., 2]
    s = torch.where(pz.abs() > EPS, 1.0 / (pz + EPS), torch.ones_like(pz))
    ux = (p[..., 0] * s * focal + 0.5) * size
    uy = (p[..., 1] * s * focal + 0.5) * size
    keep = (0 < ux) & (ux < size - 1) & (0 < uy) & (uy < size - 1)
    d = p.norm(dim=-1)
    e = torch.where(d > EPS, torch.exp(-3.0 * d), torch.zeros_like(d))
    return dict(row=size - ux, col=size - uy, keep=keep, e=e, ux=ux, uy=uy)


def corners(row, col, H, W):
    """The four corners of every point: a list of (r [B,N] long, c, b [B,N], ok [B,N] bool, inside); inside is False
    for a corner outside the image or of a non-finite coordinate, ok also for a weight below 1e-3."""
    finite = torch.isfinite(row) & torch.isfinite(col)
    row, col = torch.where(finite, row, torch.zeros_like(row)), torch.where(finite, col, torch.zeros_like(col))
    r0, c0 = row.floor(), col.floor()
    out = []
    for i in (0, 1):
        for j in (0, 1):
            r, c = r0 + i, c0 + j
            b = ((r0 + 1 - row) if i == 0 else (row - r0)) * ((c0 + 1 - col) if j == 0 else (col - c0))
            inside = finite & (r >= 0) & (r <= H - 1) & (c >= 0) & (c <= W - 1)
            out.append((r.clamp(0, H - 1).long(), c.clamp(0, W - 1).long(), b, inside & (b >= W_MIN), inside))
    return out


def splat(row, col, values, H, W):
    """sum over points and corners of b * values -> [B,C,H,W] (bilinear_rasterizer; values [B,N,C])."""
    B, N, C = values.shape
    out = values.new_zeros(B, H * W, C)
    for r, c, b, ok, _ in corners(row, col, H, W):
        w = torch.where(ok, b, torch.zeros_like(b))
        out.scatter_add_(1, (r * W + c)[..., None].expand(-1, -1, C), values * w[..., None])
    return out.reshape(B, H, W, C).permute(0, 3, 1, 2)


def render(points, colors, size, R=None, t=None, focal=1.0, dtype=torch.float64, details=False):
    """Steps 1-7 in `dtype` -> out [B,C,size,size].  details=True (float64 references): also
    den [B,size,size] = sum of e b, esum = sum of e over the same contributions, fragile [B,N] and the pixel masks
    exclude [B,size,size] (what the fragile points may change) and touched (den > 0)."""
    points, colors = points.to(dtype), colors.to(dtype)
    g = project(points, size, None if R is None else R.to(dtype), None if t is None else t.to(dtype), focal)
    e = g["e"][..., None]
    num = splat(g["row"], g["col"], e * colors * g["keep"][..., None].to(dtype), size, size)
    den = splat(g["row"], g["col"], e, size, size)
    out = num / (den + EPS)
    if not details:
        return out
    esum = torch.zeros_like(den).flatten(1)
    for r, c, b, ok, _ in corners(g["row"], g["col"], size, size):
        esum.scatter_add_(1, r * size + c, torch.where(ok, g["e"], torch.zeros_like(b)))
    fragile, exclude = fragile_points(points, g, size)
    return dict(out=out, den=den[:, 0], esum=esum.reshape(den[:, 0].shape), fragile=fragile, exclude=exclude,
                touched=den[:, 0] > 0)


def fragile_points(points, g, size):
    """delta = size * 2^-20, a few float32 ulps of a coordinate.  A point is fragile when a raster coordinate is within
    delta of an integer, u_x or u_y within delta of 0 or size - 1, or a corner weight within delta of 1e-3 -- except a
    dropped ray (x = y = 0 before the transform), which projects exactly in every precision.  The pixels such a point
    may change: the 3 x 3 block around its position for the first two kinds, the one corner for the third."""
    delta = size * 2.0 ** -20
    row, col = g["row"], g["col"]
    B, N = row.shape
    near_int = ((row - row.round()).abs() < delta) | ((col - col.round()).abs() < delta)
    near_border = torch.zeros_like(near_int)
    for u in (g["ux"], g["uy"]):
        near_border |= (u.abs() < delta) | ((u - (size - 1)).abs() < delta)
    exact = (points[..., 0] == 0) & (points[..., 1] == 0)
    block = (near_int | near_border) & ~exact & torch.isfinite(row) & torch.isfinite(col)
    exclude = torch.zeros(B, size, size, dtype=torch.bool)
    fragile = block.clone()
    for b_, n in block.nonzero().tolist():
        r, c = int(row[b_, n].floor().clamp(-2, size + 1)), int(col[b_, n].floor().clamp(-2, size + 1))
        exclude[b_, max(r - 1, 0):max(r + 2, 0), max(c - 1, 0):max(c + 2, 0)] = True
    for r, c, b, _, inside in corners(row, col, size, size):
        edge = ((b - W_MIN).abs() < delta) & ~exact & inside
        fragile |= edge
        for b_, n in edge.nonzero().tolist():
            exclude[b_, r[b_, n], c[b_, n]] = True
    return fragile, exclude
