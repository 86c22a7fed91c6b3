"""native.pointnet: one trunk of the FPD / KPD PointNet (reference: gans/metrics/pointnet.py:22-26, 46-55) -- the per-point
3 -> 64 -> 128 -> 1024 chain and the max over a cloud's points -- as dgv2_pointnet_trunk (include/dgv2.h states the
arithmetic, DESIGN.md section 40 the kernel).

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI, see the package docstring).  Forward only, float32
only; gans.metrics.pointnet calls this for CUDA inputs and runs the library-GEMM composition otherwise.  Nothing is
cached between calls and nothing is read back: the launch reads the tensors it is handed.
"""
import torch

import dgv2_native as N

P = 128                   # DGV2_POINTNET_TILE: the points of one cloud a workgroup carries through the three layers
S = P                     # the points of one cloud a workgroup covers: one tile (the workgroups of a cloud meet in feat)
FEATURES = 1024           # DGV2_POINTNET_FEATURES
MAX_TILES = 1 << 28       # DGV2_POINTNET_MAX_TILES: B * ceil(N / P) the entry takes; above it returns DGV2_ENOTSUP
_WIDTHS = (3, 64, 128, FEATURES)


def pointnet_supported(B, N_):
    """Whether dgv2_pointnet_trunk takes B clouds of N_ points (the cap of include/dgv2.h)."""
    return B >= 1 and N_ >= 1 and B * ((N_ + P - 1) // P) <= MAX_TILES


def _f32(name, t, shape):
    if t is None or tuple(t.shape) != tuple(shape):
        raise ValueError(f"pointnet_trunk: {name} must have shape {tuple(shape)}, got {None if t is None else tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"pointnet_trunk: {name} must be float32, got {t.dtype}")
    return t.detach()


def pointnet_trunk(pts, trans, l1, l2, l3, relu_last):
    """pts [B,N,3], trans [B,3,3] or None, l1 / l2 / l3 = (W, b) of the three affine maps with their batch norms folded
    (W [64,3], [128,64], [1024,128]) -> [B,1024]: max over the points of W3 relu(W2 relu(W1 (pts @ trans) + b1) + b2) + b3,
    through a ReLU when relu_last.  Everything float32, contiguous and on the device.  ValueError for other shapes or
    dtypes, an empty input or a size above pointnet_supported; RuntimeError for CPU or strided tensors.  No per-point
    activation and no workspace is allocated; no host synchronisation."""
    if pts.ndim != 3 or pts.shape[2] != 3:
        raise ValueError(f"pointnet_trunk: pts must be [B,N,3], got {tuple(pts.shape)}")
    B, n = pts.shape[0], pts.shape[1]
    if not pointnet_supported(B, n):
        raise ValueError(f"pointnet_trunk: {B} clouds of {n} points are outside the kernel's range (B, N >= 1, "
                         f"B * ceil(N / {P}) <= {MAX_TILES})")
    pts = _f32("pts", pts, (B, n, 3))
    trans = None if trans is None else _f32("trans", trans, (B, 3, 3))
    params = []
    for i, (w, b) in enumerate((l1, l2, l3)):
        params += [_f32(f"w{i + 1}", w, (_WIDTHS[i + 1], _WIDTHS[i])), _f32(f"b{i + 1}", b, (_WIDTHS[i + 1],))]
    N.check(pts, trans, *params)
    feat = torch.empty(B, FEATURES, device=pts.device, dtype=torch.float32)
    N.call("dgv2_pointnet_trunk", N.ptr(feat), N.ptr(pts), N.ptr(trans), *[N.ptr(t) for t in params], B, n,
           1 if relu_last else 0, N.stream())
    return feat


__all__ = ["pointnet_trunk", "pointnet_supported"]   # P, S, FEATURES, MAX_TILES: read as pointnet.<NAME>
