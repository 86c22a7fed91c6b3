"""Latent interpolation: a closed cubic walk through anchors in W space, rendered frame by frame
(reference: demo_interpolation.py:20-34, 73-86, 134-161, without its display code).

The path is the reference's scipy spline, built once on the host and kept as polynomial pieces on the device, so a
frame costs no host round trip; a batch of 3-D frames is one generator forward plus ONE post-processing launch
(native.frame_points: conversion, 3x3 median, normals, colours, point-set layout)."""
import numpy as np
import torch

from .models.ops import native
from .utils import colorize, tanh_to_sigmoid

__all__ = ["sample_anchors", "LatentPath", "interpolate"]


@torch.no_grad()
def sample_anchors(G, num_anchors, generator=None):
    """num_anchors latents z, each randn / sqrt(mean(z^2) + 1e-8), mapped to w: [N, num_styles, D]
    (demo_interpolation.py:143-150).  generator: the torch.Generator the draws come from; None = the global one of G's
    device."""
    dev = G.w_avg.device
    gdev = dev if generator is None else generator.device
    z_dim = G.mapping_network.in_ch
    zs = []
    for _ in range(num_anchors):
        noise = torch.randn(z_dim, generator=generator, device=gdev).to(dev)
        noise /= noise.pow(2).mean(dim=0, keepdim=True).add(1e-8).sqrt()
        zs.append(noise)
    return G.forward_mapping(torch.stack(zs)).contiguous()


class LatentPath:
    """The reference's closed path through N anchors (demo_interpolation.py:153-158): the not-a-knot cubic spline of
    scipy.interpolate.interp1d(kind="cubic", axis=0) over knots arange(-2N, 3N) with the anchors tiled five times.

    scipy runs once, here; what is kept is `coef` [N, 4, *anchor shape]: the cubic of each interval [k, k+1), k = 0 ..
    N-1, in powers of (t - k), as one tensor on the anchors' device (dtype: the anchors', or `dtype`).  path(t)
    evaluates positions t in [0, N) by Horner from that tensor with tensor ops only."""

    def __init__(self, anchors, dtype=None):
        from scipy.interpolate import make_interp_spline
        anchors = torch.as_tensor(anchors)
        n = anchors.shape[0]
        if n < 1:
            raise ValueError("LatentPath: no anchors")
        y = np.tile(anchors.detach().double().cpu().numpy(), [5] + [1] * (anchors.ndim - 1))
        # what interp1d(kind="cubic") builds: make_interp_spline(k=3) with its default not-a-knot ends
        spline = make_interp_spline(np.arange(-n * 2, n * 3), y, k=3, axis=0)
        k = np.arange(n, dtype=np.float64)
        # Taylor coefficients at the left knot; the third derivative is piecewise constant: taken at the midpoint
        coef = np.stack([spline(k), spline(k, 1), spline(k, 2) / 2.0, spline(k + 0.5, 3) / 6.0], axis=1)
        self.num_anchors = n
        self.coef = torch.from_numpy(coef).to(device=anchors.device, dtype=dtype or anchors.dtype)

    def __call__(self, t):
        t = torch.as_tensor(t).to(device=self.coef.device, dtype=self.coef.dtype).reshape(-1)
        k = t.floor().clamp_(0, self.num_anchors - 1)
        s = (t - k).reshape((-1,) + (1,) * (self.coef.ndim - 2))
        c = self.coef[k.long()]
        return ((c[:, 3] * s + c[:, 2]) * s + c[:, 1]) * s + c[:, 0]

    def steps(self, frames_per_anchor=90):
        """One lap: linspace(0, N, frames_per_anchor * N, endpoint=False) (demo_interpolation.py:153,160), float64."""
        n = self.num_anchors
        return torch.from_numpy(np.linspace(0, n, int(frames_per_anchor * n), endpoint=False))


@torch.no_grad()
def interpolate(G, coord, path, steps, truncation_psi=0.7, mode="3d", batch=8, border="zeros", u=None):
    """Generator of frames along `path` at the positions `steps` (a 1-D tensor / array in [0, N)).

    G: a generator in eval mode on the device of `coord` (the truncation trick applies in eval mode only).
    u [1,1,H,W]: the ray-drop uniforms, fixed for the whole walk (the reference's "make deterministic",
    demo_interpolation.py:134-139), drawn once when None; they reach the generator through its `noise` argument.
    mode "3d": yields (points [H*W,3], colors [H*W,3]) per frame -- median-filtered points / max_depth and their
      normal colours; `border`: what the median sees outside the image, "zeros" (kornia's median_blur) or "ring".
    mode "2d": yields one [3, R*H, W] turbo-coloured image per frame: the range image, under the image before ray-drop
      and the ray-drop probability when the generator returns them (R = 3, else 1), stacked along H.
    The walk runs `batch` frames per generator forward; the last batch may be shorter."""
    if mode not in ("2d", "3d"):
        raise ValueError(f"{mode=}")
    dev = coord.angle.device
    H, W = coord.angle.shape[2:]
    if u is None:
        u = native.gumbel_uniform((1, 1, H, W), dev)
    if tuple(u.shape) != (1, 1, H, W):
        raise ValueError(f"interpolate: u must be [1,1,{H},{W}], got {tuple(u.shape)}")
    u = u.to(dev).float()
    steps = torch.as_tensor(steps).reshape(-1)
    for i in range(0, len(steps), batch):
        w = path(steps[i:i + batch]).float()
        imgs = G(z=w, angle=coord.angle, truncation_psi=truncation_psi, input_w=True,
                 noise={"gumbel_u": u.expand(len(w), 1, H, W)})
        if mode == "3d":
            points, colors = native.frame_points(imgs["image"], coord.angle, coord.min_depth, coord.max_depth, border)
            yield from zip(points, colors)
        else:
            grid = [tanh_to_sigmoid(imgs["image"])]
            if "image_orig" in imgs:
                grid = [tanh_to_sigmoid(imgs["image_orig"]), imgs["raydrop_logit"].sigmoid()] + grid
            yield from colorize(torch.cat(grid, dim=2))
