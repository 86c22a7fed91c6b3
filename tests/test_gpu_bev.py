"""GPU checks of the bird's-eye-view splat (csrc/bev.hip, gans/render.py, CoordBridge.make_birds_eye_view; DESIGN.md
section 37) against the float64 restatement of tests/bev_ref.py, of its bit-reproducibility, and of
gans.utils.power_spectrum_2d."""
import math

import numpy as np
import pytest
import torch

import bev_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIN_DEPTH, MAX_DEPTH = 1.45, 80.0
BEV_T = (0.0, 0.0, 0.7)


# ---------------------------------------------------------------------------- a. constructed points
def constructed(B, N, C, size, R, t, focal, seed, pz_sign=1.0):
    """Points whose raster position has both fractional parts in [1/4, 3/4]: chosen in the raster, then taken back
    through the projection and the extrinsics in float64.  One in ten sits in raster row (0, 1): u_x > size - 1, so it is
    not kept and only dilutes.  Returns float32 (points, colors)."""
    g = torch.Generator().manual_seed(seed)
    frac = 0.25 + 0.5 * torch.rand(B, N, 2, generator=g, dtype=torch.float64)
    whole = torch.randint(1, size - 1, (B, N, 2), generator=g).double()
    whole[..., 0][torch.rand(B, N, generator=g) < 0.1] = 0.0
    u = size - (whole + frac)
    pz = pz_sign * (0.5 + torch.rand(B, N, generator=g, dtype=torch.float64))
    p = torch.cat([(u / size - 0.5) / focal * pz[..., None], pz[..., None]], dim=-1)
    if t is not None:
        p = p - t.double().reshape(3)
    if R is not None:
        p = p @ R.double().reshape(3, 3).T   # R is orthonormal: the inverse of "times R"
    points = (p * p.new_tensor([1.0, 1.0, -1.0])).float()
    return points, torch.rand(B, N, C, generator=g)


def extrinsics(kind):
    if kind == "plain":
        return None, None, 1.0
    R, t = bev_ref.make_Rt(roll=0.3, pitch=-0.2, yaw=0.5, x=0.05, y=-0.1, z=0.4)
    return R[0].float(), t[0].float(), 0.7 if kind == "focal" else 1.0


@pytest.mark.parametrize("kind", ["plain", "Rt", "focal"])
@pytest.mark.parametrize("shape", [(2, 300, 3, 32), (1, 1, 1, 8), (3, 257, 4, 24)], ids=lambda s: "x".join(map(str, s)))
def test_constructed_points(shape, kind):
    """Every point is far from every decision edge (fractions in [1/4, 3/4]: no corner flips, every bilinear factor is
    >= 1/4, every weight >= 1/16 >> 1e-3), so nothing is excluded.  atol 1e-3 against float64: a float32 coordinate is
    off by at most size * 2^-21, so a bilinear factor >= 1/4 carries a relative error of at most size * 2^-19 and a
    weight (two factors) size * 2^-18; the output is a convex combination of colours in [0, 1], normalised by the sum
    of the same weights, so its error is at most twice that: 64 * 2^-17 < 5e-4 at size <= 64."""
    from gans.render import render_point_clouds
    B, N, C, size = shape
    R, t, focal = extrinsics(kind)
    points, colors = constructed(B, N, C, size, R, t, focal, seed=B * 1000 + N)
    ref = bev_ref.render(points, colors, size, R, t, focal, details=True)
    assert not bool(ref["fragile"].any())
    dev = lambda v: None if v is None else v.to(DEV)
    out = render_point_clouds(dev(points), dev(colors), size=size, R=dev(R), t=dev(t), focal_length=focal)
    assert out.shape == (B, C, size, size) and out.dtype == torch.float32
    err = float((out.cpu().double() - ref["out"]).abs().max())
    print(f"constructed {shape} {kind}: max abs err {err:.3e}, touched pixels {int(ref['touched'].sum())}")
    assert bool(ref["touched"].any()) and float(ref["out"].max()) > 0.05
    assert err <= 1e-3


# ---------------------------------------------------------------------------- b. range-image points
def range_scene(B, H, W, seed):
    """inv_depth_norm [B,1,H,W] of a smooth synthetic scene with 10 % dropped rays (zeros), and the sensor's angle
    grid [H,W,2] with the azimuths offset by half a step: with an even size the image's centre lines are pixel edges,
    and a ray along an axis would sit on one by construction."""
    rng = np.random.RandomState(seed)
    elev = np.deg2rad(np.linspace(2.0, -24.8, H))[:, None].repeat(W, 1)
    azim = (np.pi - (np.arange(W) + 0.5) * 2 * np.pi / W)[None, :].repeat(H, 0)
    phase = rng.uniform(0, 2 * np.pi, (B, 1, 1))
    depth = 18.0 + 10.0 * np.sin(3 * azim[None] + phase) + 6.0 * np.cos(5 * azim[None] - phase) + rng.uniform(-1.5, 1.5, (B, H, W))
    inv = MIN_DEPTH / depth
    inv[rng.uniform(size=inv.shape) < 0.1] = 0.0
    return torch.from_numpy(inv[:, None]).float(), np.stack([elev, azim], axis=-1).astype(np.float32)


def bridge_for(H, W, angle):
    from gans.coords import CoordBridge
    return CoordBridge(H, W, MIN_DEPTH, MAX_DEPTH, angle_array=angle).to(DEV)


def flat(x):
    return x.flatten(2).transpose(1, 2).contiguous()


def check_against_restatement(out, points, colors, size, R, t, what):
    """The device output against the float64 restatement on the SAME float32 points.  Pixels that a fragile point may
    change are excluded (they must stay under 5 % of the pixels that receive weight); everywhere else the error must
    stay under 1e-6 + 4 delta sum(e_i) / (sum(e_i b_i) + 1e-8), delta = size * 2^-20, summed over the pixel's
    contributions: each weight e_i b_i carries an absolute error of at most 2 delta e_i (delta on a coordinate moves a
    bilinear factor by delta and the product of two by at most 2 delta), colours are in [0, 1], and numerator and
    denominator err alike.  Returns the worst error-to-bound ratio and the excluded share."""
    ref = bev_ref.render(points.cpu(), colors.cpu(), size, None if R is None else R.cpu(), None if t is None else t.cpu(),
                         details=True)
    delta = size * 2.0 ** -20
    tol = 1e-6 + 4 * delta * ref["esum"] / (ref["den"] + 1e-8)
    touched, exclude = ref["touched"], ref["exclude"] & ref["touched"]
    share = float(exclude.sum()) / float(touched.sum())
    err = (out.cpu().double() - ref["out"]).abs().amax(dim=1)
    ratio = float((err / tol)[~exclude].max())
    print(f"{what}: {int(ref['fragile'].sum())} fragile of {points.shape[0] * points.shape[1]} points, "
          f"{int(exclude.sum())} of {int(touched.sum())} touched pixels excluded ({100 * share:.2f} %), "
          f"worst error / bound {ratio:.3f}, worst error {float(err[~exclude].max()):.3e}")
    assert float(touched.sum()) > 0.2 * size * size
    assert share <= 0.05
    assert ratio <= 1.0
    return ratio, share


@pytest.mark.parametrize("H,W", [(8, 64), (16, 128)])
def test_range_image_points(H, W):
    from gans.render import render_point_clouds
    from gans.utils import points_to_normal_2d
    size = W // 2
    inv, angle = range_scene(2, H, W, seed=H)
    bridge = bridge_for(H, W, angle)
    points_map = bridge.convert(inv.to(DEV), "inv_depth_norm", "point_map") / MAX_DEPTH
    points, colors = flat(points_map), flat(points_to_normal_2d(points_map, mode="closest"))
    t = torch.tensor(BEV_T, device=DEV)
    out = render_point_clouds(points, colors, size=size, t=t)
    check_against_restatement(out, points, colors, size, None, t, f"range image {H}x{W} -> {size}")


# ---------------------------------------------------------------------------- c. reproducibility
def test_bits_do_not_depend_on_run_or_point_order():
    """Many points per pixel (5000 on 32 x 32): float atomics would differ in the last bits between two runs and
    between two orders; 64-bit integer sums cannot."""
    from gans.render import render_point_clouds
    g = torch.Generator().manual_seed(5)
    points = torch.cat([torch.rand(2, 5000, 2, generator=g) - 0.5, -0.6 - torch.rand(2, 5000, 1, generator=g)], dim=-1).to(DEV)
    colors = torch.rand(2, 5000, 3, generator=g).to(DEV)
    first = render_point_clouds(points, colors, size=32)
    assert float(first.max()) > 0.1
    assert torch.equal(first, render_point_clouds(points, colors, size=32))
    perm = torch.randperm(5000, generator=g).to(DEV)
    assert torch.equal(first, render_point_clouds(points[:, perm].contiguous(), colors[:, perm].contiguous(), size=32))


# ---------------------------------------------------------------------------- d. other cases
def test_bilinear_rasterizer_against_restatement():
    """Float32 against float64 on the same float32 inputs (floor decides alike on both).  Bound per pixel: an addend
    b_r b_c v carries two roundings in each factor's subtraction-and-product and one in each product, under
    5 * 2^-24 relative, and the output is rounded once more: 2^-21 sum |v_i| b_i + 1e-9 (the 2^-40 quantum of the
    integer sum is far below)."""
    from gans.render import bilinear_rasterizer
    H, W, N = 5, 9, 400
    g = torch.Generator().manual_seed(3)
    coords = torch.rand(2, N, 2, generator=g) * torch.tensor([H + 3.0, W + 3.0]) - 2.0
    coords[0, 0, 0], coords[0, 1, 1], coords[1, 0, 0] = float("nan"), 1e30, -1e30
    values = 3.0 * torch.randn(2, N, 2, generator=g)   # beyond [-1, 1]: the wrapper's power-of-two scaling is in play
    ref = bev_ref.splat(coords[..., 0].double(), coords[..., 1].double(), values.double(), H, W)
    mass = bev_ref.splat(coords[..., 0].double(), coords[..., 1].double(), values.double().abs(), H, W)
    out = bilinear_rasterizer(coords.to(DEV), values.to(DEV), (H, W))
    assert out.shape == (2, 2, H, W) and bool(torch.isfinite(out).all())
    err = (out.cpu().double() - ref).abs()
    print(f"bilinear_rasterizer: worst error / bound {float((err / (2.0 ** -21 * mass + 1e-9)).max()):.3f}")
    assert bool((err <= 2.0 ** -21 * mass + 1e-9).all()) and float(ref.abs().max()) > 1


def test_points_are_not_modified_and_one_point_behind_the_camera():
    from gans.render import render_point_clouds
    R, t, focal = extrinsics("Rt")
    points, colors = constructed(1, 1, 2, 16, R, t, focal, seed=11, pz_sign=-1.0)   # p_z < 0: projects mirrored
    assert bool(bev_ref.project(points.double(), 16, R.double(), t.double())["keep"].all())
    dp = points.to(DEV)
    before = dp.clone()
    out = render_point_clouds(dp, colors.to(DEV), size=16, R=R.to(DEV)[None], t=t.to(DEV)[None])   # [1,3,3] / [1,3] forms
    assert torch.equal(dp, before)
    ref = bev_ref.render(points, colors, 16, R, t)
    assert float(ref.max()) > 0.01 and float((out.cpu().double() - ref).abs().max()) <= 1e-3


def test_all_points_outside_give_zeros():
    from gans.render import render_point_clouds
    points = torch.tensor([[[5.0, 0.0, -1.0], [0.0, -7.0, -1.0], [1e30, 1e30, -1.0], [float("nan"), 0.0, -1.0]]], device=DEV)
    out = render_point_clouds(points, torch.ones(1, 4, 3, device=DEV), size=16)
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) == 0.0


# ---------------------------------------------------------------------------- e. make_birds_eye_view and the helpers
def test_make_birds_eye_view():
    from gans.render import make_Rt, render_point_clouds
    from gans.utils import points_to_normal_2d
    H, W = 8, 64
    inv, angle = range_scene(2, H, W, seed=21)
    bridge = bridge_for(H, W, angle)
    Rt = make_Rt(pitch=0.2, yaw=0.4, z=0.7, device=DEV)
    inv = inv.to(DEV)
    out = bridge.make_birds_eye_view(inv, Rt)
    assert out.shape == (2, 3, W, W)
    points_map = bridge.convert(inv, "inv_depth_norm", "point_map") / MAX_DEPTH
    points, colors = flat(points_map), flat(points_to_normal_2d(points_map, mode="closest"))
    assert torch.equal(out, render_point_clouds(points, colors, size=W, R=Rt[0], t=Rt[1]))
    check_against_restatement(out, points, colors, W, Rt[0][0], Rt[1][0], "make_birds_eye_view 8x64 -> 64")


def test_power_spectrum_2d():
    from gans.utils import power_spectrum_2d
    x = torch.rand(2, 1, 8, 64, generator=torch.Generator().manual_seed(9))
    ref = bev_ref.power_spectrum_2d(x)
    out = power_spectrum_2d(x.to(DEV)).cpu().double()
    big = ref > -100
    assert out.shape == ref.shape and int(big.sum()) > 0.9 * ref.numel()
    assert torch.allclose(out[big], ref[big], rtol=1e-4, atol=0)
    assert math.isfinite(float(out[big].min()))
