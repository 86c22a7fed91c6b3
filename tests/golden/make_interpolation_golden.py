#!/usr/bin/env python3
"""Generate tests/golden/interpolation.npz by running the REFERENCE's latent-walk post-processing on CPU (build machine
only).

    python tests/golden/make_interpolation_golden.py

The reference tree is imported through _refshim, as make_inversion_golden.py does; what is written is data only:
seeded inputs and the reference's results in float64 and float32 (the per-case deviation between the two is what the
GPU tests derive their tolerance from).

(a) demo_interpolation.py:79-86 -- tanh_to_sigmoid, CoordBridge.convert to a point map, median_blur (3, 3), convert to
    a normal map, tanh_to_sigmoid, / max_depth, point-set layout -- with the reference's own CoordBridge.convert and
    estimate_surface_normal.  kornia is not installed here, so the median is written out by its documented semantics:
    3x3 windows by unfold with ZERO padding, median over the window.  The "ring" variant pads rows by replication and
    columns circularly instead.  Also the chain without the median (convert(..., "normal_map") from every source).
(b) gans.utils.colorize with an ndarray LUT.
(c) scipy.interpolate.interp1d as demo_interpolation.py:154-159 builds it.

The script ASSERTS that its inputs keep the reference itself well-conditioned before it writes anything.  Two steps of
(a) are SELECTIONS, which a rounding error can flip to a different (equally valid) outcome:
  * the 3x3 median: the gaps between the 4th, 5th and 6th order statistic of a window;
  * the "closest" neighbour pair of the normal: the gap between the best and the second-best pair sum.
A pixel is FRAGILE when one of these gaps, evaluated in float64, is below 1e-4 of the local scale (the largest
magnitude in the window / the second-best sum).  An EXACT tie is not fragile where it cannot flip: equal order
statistics (the zeros of the border and of dropped rays, the copies of a replicated row: equal values are one value,
whichever copy is selected), pair sums that tie exactly in float64 AND in float32 (pairs made of the same points, as
at a clamped row between zero medians: "the first minimum" is then the same pair in every precision).  The mask is per pixel and not spread over the normal's stencil: an order statistic is 1-Lipschitz in
the sup norm, so a median that rounding flips between two near-equal values moves by less than the rounding that
flipped it and reaches its neighbours' normals as an ordinary perturbation, which the float32-vs-float64 deviation
measures; only the pair choice is discontinuous.  At most 2 % of a case's pixels may be fragile; the mask is stored
and the tests skip those pixels.
"""
import copy
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refshim  # noqa: E402

_refshim.install()

import scipy.interpolate  # noqa: E402

from gans.coords import CoordBridge  # noqa: E402
from gans.utils import colorize, tanh_to_sigmoid  # noqa: E402

torch.set_num_threads(8)
F = torch.nn.functional
MIN_DEPTH, MAX_DEPTH = 1.45, 80.0
SHAPES = [(2, 1, 8, 32), (1, 1, 5, 7), (3, 1, 3, 5), (1, 1, 16, 40)]
BORDERS = ("zeros", "ring")
SOURCES = ("depth", "depth_norm", "inv_depth_norm", "point_map")
REL_GAP, MAX_FRAGILE, D = 1e-4, 0.02, 2


def small_angle_file():
    rng = np.random.RandomState(0)
    elev = np.linspace(0.035, -0.43, 16)[:, None] + rng.randn(16, 96) * 1e-3
    azim = np.linspace(np.pi, -np.pi, 96, endpoint=False)[None, :] + rng.randn(16, 96) * 1e-3
    return np.stack([elev, azim], axis=-1).astype(np.float32)


def coord_bridge(angle_file, H, W):
    with tempfile.TemporaryDirectory() as tmp:      # the reference's CoordBridge reads its grid from a file only
        path = os.path.join(tmp, "angle.npy")
        np.save(path, angle_file)
        return CoordBridge(num_ring=H, num_points=W, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, angle_file=path)


def make_image(shape, seed):
    """A smooth range surface plus noise, as the generator's "image" in [-1,1]; a planted share of pixels outside the
    depth range: dropped rays (image = -1: inverse depth 0) and returns beyond max_depth."""
    B, _, H, W = shape
    g = torch.Generator().manual_seed(seed)
    hh = torch.linspace(0, 1, H)[None, None, :, None]
    ww = torch.linspace(0, 2 * np.pi, W + 1)[None, None, None, :W]
    ph = torch.linspace(0.3, 1.7, B)[:, None, None, None]
    depth = 8.0 + 25.0 * hh + 5.0 * torch.sin(2 * ww + ph) * (1 - hh) + 1.0 * torch.rand(B, 1, H, W, generator=g)
    assert float(depth.min()) > MIN_DEPTH + 1 and float(depth.max()) < MAX_DEPTH - 1
    r = torch.rand(B, 1, H, W, generator=g)
    depth = torch.where(r < 0.01, torch.full_like(depth, 100.0), depth)          # beyond max_depth: masked to 0
    x = MIN_DEPTH / depth
    x = torch.where((r >= 0.01) & (r < 0.04), torch.zeros_like(x), x)            # dropped rays
    for t in (0.0, MIN_DEPTH / MAX_DEPTH, 1.0):                                  # away from every threshold on the way
        assert float(((x - t).abs() + (x == 0).float()).min()) >= 1e-3, t
    planted = (r < 0.04).float().mean()
    return (x * 2.0 - 1.0).float(), float(planted)


def windows(pm, border):
    """[B,3,H,W] -> the 3x3 windows [B,3,9,H,W]."""
    B, C, H, W = pm.shape
    if border == "zeros":
        u = F.unfold(pm, 3, padding=1)
    else:
        p = F.pad(pm, (0, 0, 1, 1), mode="replicate")
        p = F.pad(p, (1, 1, 0, 0), mode="circular")
        u = F.unfold(p, 3)
    return u.view(B, C, 9, H, W)


def median3x3(pm, border):
    return windows(pm, border).median(dim=2).values


def flat(x):
    return x.flatten(2).permute(0, 2, 1).contiguous()


def chain(cb, image, border, dtype):
    c = copy.deepcopy(cb).to(dtype)
    x = tanh_to_sigmoid(image.to(dtype))
    pm = c.convert(x, "inv_depth_norm", "point_map")
    med = median3x3(pm, border)
    normal = c.convert(med, "point_map", "normal_map")
    return {"pm": pm, "med": med, "points": flat(med / c.max_depth), "colors": flat(tanh_to_sigmoid(normal))}


def neighbour(x, dh, dw):
    """x[..., clamp(h + dh), (w + dw) mod W]: the normal's topology."""
    H, W = x.shape[-2:]
    hi = (torch.arange(H) + dh).clamp(0, H - 1)
    wi = (torch.arange(W) + dw) % W
    return x[..., hi, :][..., wi]


OFFSETS = [(-D, 0), (-D, D), (0, D), (D, D), (D, 0), (D, -D), (0, -D), (-D, -D)]


def pair_sums(points):
    nrm = torch.stack([(neighbour(points, dh, dw) - points).norm(dim=1) for dh, dw in OFFSETS], dim=1)   # [B,8,H,W]
    return (nrm + nrm[:, [(k + 2) % 8 for k in range(8)]]).sort(dim=1).values


def fragile_closest(points, points32):
    """points [B,3,H,W] float64 (and the float32 evaluation of the same map) -> [B,H,W] bool."""
    s, s32 = pair_sums(points), pair_sums(points32)
    best, second = s[:, 0], s[:, 1]
    exact_tie = (second == best) & (s32[:, 1] == s32[:, 0])     # in both precisions: the first minimum wins in both
    return (second - best < REL_GAP * second) & ~exact_tie


def fragile_median(pm, border):
    """pm [B,3,H,W] float64 -> [B,H,W] bool."""
    win = windows(pm, border)
    s = win.sort(dim=2).values
    scale = win.abs().max(dim=2).values
    bad = torch.zeros_like(scale, dtype=torch.bool)
    for a, b in ((3, 4), (4, 5)):
        gap = s[:, :, b] - s[:, :, a]
        bad |= (gap > 0) & (gap < REL_GAP * scale)
    return bad.any(dim=1)


def dev_outside(a32, a64, keep):
    """max |float32 result - float64 result| over the kept pixels; a, [B,HW,3]; keep [B,H,W]."""
    d = (a32.double() - a64).abs().amax(dim=-1)
    return float((d * keep.flatten(1)).max())


def golden_chain(out, angle_file):
    names = []
    for ci, shape in enumerate(SHAPES):
        B, _, H, W = shape
        cb = coord_bridge(angle_file, H, W)
        image, planted = make_image(shape, 100 + ci)
        assert 0.0 < planted < 0.2 or B * H * W < 64, planted
        case = f"{B}x{H}x{W}"
        names.append(case)
        out[f"chain.{case}.image"] = image
        out[f"chain.{case}.angle"] = cb.angle.clone()           # what the reference's CoordBridge resampled (float32)
        for border in BORDERS:
            r64, r32 = chain(cb, image, border, torch.float64), chain(cb, image, border, torch.float32)
            f_med, f_pair = fragile_median(r64["pm"], border), fragile_closest(r64["med"] / MAX_DEPTH, r32["med"] / MAX_DEPTH)
            fragile = f_med | f_pair
            share = float(fragile.float().mean())
            # pixels whose normal is ZERO (colour 0.5): the chosen pair holds a zero vector, or -- at a clamped row
            # between equal medians -- two identical vectors.  The value is known there, and the reference's own float32
            # is no yardstick for it: torch's CPU cross contracts a*b - c*d to an FMA and leaves the rounding residue of
            # the product of identical vectors (~1e-17 in float64, ~1e-10 in float32), which n / (|n| + 1e-8) turns
            # into ~1e-9 and ~1e-2.  They are stored apart and kept out of the deviation; the tests hold them to 0.5
            # within the 1e-6 floor alone (they are checked, more tightly, not excluded: they do not count as fragile).
            zero_normal = ((r64["colors"] - 0.5).abs() < 1e-6).all(dim=-1).view(B, H, W) & ~fragile
            dp = dev_outside(r32["points"], r64["points"], ~fragile)
            dc = dev_outside(r32["colors"], r64["colors"], ~fragile & ~zero_normal)
            print(f"chain {case} {border}: planted {planted:.1%}; fragile {share:.2%} (median {int(f_med.sum())}, pair "
                  f"{int(f_pair.sum())} of {fragile.numel()} pixels); zero normals {int(zero_normal.sum())}; "
                  f"ref fp32-vs-fp64 points {dp:.2e} colors {dc:.2e}")
            assert share <= MAX_FRAGILE, (case, border, share)
            assert dp < 1e-6 and dc < 1e-4, (case, border, dp, dc)   # elsewhere the reference agrees with itself
            assert bool(torch.isfinite(r64["colors"]).all())
            # the masks and the zeros entering the median are exercised
            assert bool((r64["pm"] == 0).all(dim=1).any()) or B * H * W < 64
            k = f"chain.{case}.{border}"
            out[f"{k}.points"], out[f"{k}.colors"] = r64["points"], r64["colors"]
            out[f"{k}.points32"], out[f"{k}.colors32"] = r32["points"], r32["colors"]
            out[f"{k}.fragile"], out[f"{k}.zero_normal"] = fragile, zero_normal
            out[f"{k}.dev"] = np.array([dp, dc])
        # without the median: convert(..., "normal_map") from every source (coords.py:104-113, 142-151, 171-175)
        c64 = copy.deepcopy(cb).double()
        x64 = tanh_to_sigmoid(image.double())
        src = {"inv_depth_norm": x64, "depth": c64.convert(x64, "inv_depth_norm", "depth"),
               "point_map": c64.convert(x64, "inv_depth_norm", "point_map")}
        src["depth_norm"] = src["depth"] / MAX_DEPTH
        want = c64.convert(x64, "inv_depth_norm", "normal_map")
        f_n = fragile_closest(src["point_map"] / MAX_DEPTH, src["point_map"].float() / MAX_DEPTH)
        assert float(f_n.float().mean()) <= MAX_FRAGILE, (case, float(f_n.float().mean()))
        devs = []
        for s in SOURCES:
            v32 = src[s].float()                                 # what a float32 caller can hand in
            out[f"normal.{case}.src.{s}"] = v32
            c32 = copy.deepcopy(cb)
            if s == "depth_norm":                                # the reference has no depth_norm -> normal_map branch:
                got = c32.convert(c32.convert(v32, "depth_norm", "depth"), "depth", "normal_map")   # through depth
            else:
                got = c32.convert(v32, s, "normal_map")
            devs.append(float(((got.double() - want).abs().amax(dim=1) * ~f_n).max()))
            assert devs[-1] < 1e-4, (case, s, devs[-1])
        print(f"normal {case}: fragile {float(f_n.float().mean()):.2%}; ref fp32-vs-fp64 per source "
              + " ".join(f"{s} {d:.2e}" for s, d in zip(SOURCES, devs)))
        out[f"normal.{case}.value"], out[f"normal.{case}.fragile"] = want, f_n
        out[f"normal.{case}.dev"] = np.array(devs)
    out["chain.cases"] = np.array(names)
    out["chain.borders"] = np.array(BORDERS)
    out["normal.sources"] = np.array(SOURCES)
    out["depth_range"] = np.array([MIN_DEPTH, MAX_DEPTH])


def golden_colorize(out):
    g = torch.Generator().manual_seed(7)
    lut = np.random.RandomState(7).rand(256, 3)
    x = torch.rand(2, 1, 4, 16, generator=g) * 1.4 - 0.2
    special = [0.0, 1.0, -0.5, 1.5, 255.999 / 256, 1.0 / 256, 37.0 / 256, 128.0 / 256, 255.0 / 256, 254.999 / 256,
               -1e-9, 0.999999]
    x.view(-1)[:len(special)] = torch.tensor(special)
    x256 = (x * 256).view(-1)
    assert bool((x256[:len(special)] == x256[:len(special)].round())[[0, 1, 5, 6, 7, 8]].all())   # exactly on integers
    assert float(x.min()) < 0 and float(x.max()) > 1
    y = colorize(x, cmap=lut)
    assert tuple(y.shape) == (2, 3, 4, 16) and y.dtype == torch.float32
    assert torch.equal(colorize(x[:, 0], cmap=lut), y)
    out["colorize.lut"], out["colorize.x"], out["colorize.y"] = lut, x, y


def golden_interp(out):
    rng = np.random.RandomState(3)
    for n in (2, 3, 10):
        zs = rng.randn(n, 6)
        fn = scipy.interpolate.interp1d(x=np.arange(-n * 2, n * 3), y=np.tile(zs, [5, 1]), kind="cubic", axis=0)
        pos = np.concatenate([[0.0, n - 1e-6], np.arange(n, dtype=np.float64), rng.rand(17) * n])[:17]
        assert len(pos) == 17 and pos.min() >= 0 and pos.max() < n
        out[f"interp.{n}.anchors"], out[f"interp.{n}.pos"], out[f"interp.{n}.value"] = zs, pos, fn(pos)
    out["interp.sizes"] = np.array([2, 3, 10])


def main():
    out = {}
    angle_file = small_angle_file()
    out["angle_file"] = angle_file
    golden_chain(out, angle_file)
    golden_colorize(out)
    golden_interp(out)
    path = os.path.join(HERE, "interpolation.npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                                 for k, v in out.items()})
    print(f"interpolation.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
