"""Frame post-processing and the latent walk on the GPU (csrc/frame.hip, gans/interpolation.py, gans/utils.colorize,
CoordBridge.convert(..., "normal_map"), demo_interpolation.py).

Two references:
  * the UNFUSED composition of the project's own ops in the same process (convert, an exact 3x3 median from F.unfold +
    sort, / max_depth, convert to a normal map, (n + 1) / 2): dgv2_frame_points must equal it BIT FOR BIT -- the median
    is a selection and both sides inline the same device functions (coords_dev.h, normal_dev.h).  torch.equal compares
    values: two zeros of opposite sign, which a selection may pick either of, are equal;
  * tests/golden/interpolation.npz: the reference's own code on CPU in float64 and float32
    (tests/golden/make_interpolation_golden.py).  Tolerance, the rule of tests/test_gpu_inversion.py: 1e-6 absolute
    (points and colours live in [-1, 1]) plus twice the reference's OWN float32-vs-float64 deviation of that case,
    outside the fragile pixels the fixture stores (selections a rounding error can flip), at most 2 % of a case.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
BORDERS = ("zeros", "ring")
CASES = ("2x8x32", "1x5x7", "3x3x5", "1x16x40")
MIN_DEPTH, MAX_DEPTH = 1.45, 80.0


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "interpolation.npz"))
    g = {k: d[k] for k in d.files}
    assert tuple(g["chain.cases"]) == CASES and tuple(g["depth_range"]) == (MIN_DEPTH, MAX_DEPTH)
    return g


def t(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


def bridge(H, W, angle_file, angle=None):
    from gans.coords import CoordBridge
    c = CoordBridge(H, W, MIN_DEPTH, MAX_DEPTH, angle_array=angle_file).to(DEV)
    if angle is not None:   # the very grid the reference resampled, so both sides convert the same angles
        assert float((c.angle.cpu() - torch.from_numpy(angle)).abs().max()) < 1e-5
        c.angle.copy_(torch.from_numpy(angle))
    return c


def case_bridge(gold, case):
    H, W = (int(v) for v in case.split("x")[1:])
    return bridge(H, W, gold["angle_file"], gold[f"chain.{case}.angle"])


def flat(x):
    return x.flatten(2).permute(0, 2, 1).contiguous()


def median3x3(pm, border):
    """Exact 3x3 median of every channel: the 5th of the 9 sorted window values."""
    B, C, H, W = pm.shape
    if border == "zeros":
        u = F.unfold(pm, 3, padding=1)
    else:
        p = F.pad(pm, (0, 0, 1, 1), mode="replicate")
        u = F.unfold(F.pad(p, (1, 1, 0, 0), mode="circular"), 3)
    return u.view(B, C, 9, H, W).sort(dim=2).values[:, :, 4]


def unfused(coord, image, border):
    from gans.utils import tanh_to_sigmoid
    pm = coord.convert(tanh_to_sigmoid(image), "inv_depth_norm", "point_map")
    med = median3x3(pm, border)
    points = med / coord.max_depth
    n = coord.convert(med, "point_map", "normal_map")
    return flat(points), flat((n + 1) / 2)


def fused(coord, image, border):
    from gans.models.ops import native
    return native.frame_points(image, coord.angle, coord.min_depth, coord.max_depth, border)


def synthetic_image(B, H, W, seed):
    """A range surface with noise, dropped rays (image = -1) and returns beyond max_depth, as the generator's image."""
    g = torch.Generator().manual_seed(seed)
    hh = torch.linspace(0, 1, H)[None, None, :, None]
    ww = torch.linspace(0, 2 * np.pi, W + 1)[None, None, None, :W]
    depth = 8.0 + 25.0 * hh + 5.0 * torch.sin(2 * ww) * (1 - hh) + torch.rand(B, 1, H, W, generator=g)
    r = torch.rand(B, 1, H, W, generator=g)
    depth = torch.where(r < 0.01, torch.full_like(depth, 100.0), depth)
    x = torch.where((r >= 0.01) & (r < 0.05), torch.zeros_like(depth), MIN_DEPTH / depth)
    return (x * 2 - 1).to(DEV)


# ---------------------------------------------------------------------------------------
# 1. the one launch equals the unfused definition, bit for bit
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("case", CASES)
def test_frame_points_equals_the_unfused_composition(gold, case, border):
    coord = case_bridge(gold, case)
    image = t(gold[f"chain.{case}.image"])
    (p, c), (p0, c0) = fused(coord, image, border), unfused(coord, image, border)
    assert p.shape == p0.shape == c.shape == (image.shape[0], image.shape[2] * image.shape[3], 3)
    dp, dc = float((p - p0).abs().max()), float((c - c0).abs().max())
    print(f"{case} {border}: max |points diff| {dp:.2e}, max |colors diff| {dc:.2e}, "
          f"{int((c != c0).any(dim=-1).sum())} pixels differ")
    assert torch.equal(p, p0)
    assert torch.equal(c, c0)


@pytest.mark.parametrize("border", BORDERS)
def test_frame_points_equals_the_unfused_composition_at_full_size(border):
    """[2,1,64,512]: 8 x 8 tiles per frame, more than one frame."""
    from gans.coords import synthetic_angle_grid
    coord = bridge(64, 512, synthetic_angle_grid(64))
    image = synthetic_image(2, 64, 512, 5)
    (p, c), (p0, c0) = fused(coord, image, border), unfused(coord, image, border)
    print(f"64x512 {border}: max |points diff| {float((p - p0).abs().max()):.2e}, max |colors diff| "
          f"{float((c - c0).abs().max()):.2e}")
    assert bool((p0 == 0).all(dim=-1).any()) and bool(torch.isfinite(c).all())
    assert torch.equal(p, p0)
    assert torch.equal(c, c0)


@pytest.mark.parametrize("shape", [(1, 9, 65), (2, 17, 130), (1, 1, 3), (1, 2, 70)])
def test_frame_points_at_tile_edges(shape):
    """One past a multiple of the 8 x 64 tile in both directions, one row, the narrowest legal width."""
    from gans.coords import synthetic_angle_grid
    B, H, W = shape
    coord = bridge(H, W, synthetic_angle_grid(max(H, 2)))
    image = synthetic_image(B, H, W, 11)
    for border in BORDERS:
        (p, c), (p0, c0) = fused(coord, image, border), unfused(coord, image, border)
        assert torch.equal(p, p0) and torch.equal(c, c0), (shape, border)


# ---------------------------------------------------------------------------------------
# 2. the reference's own chain
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("case", CASES)
def test_frame_points_matches_the_reference(gold, case, border):
    coord = case_bridge(gold, case)
    p, c = fused(coord, t(gold[f"chain.{case}.image"]), border)
    k = f"chain.{case}.{border}"
    fragile = torch.from_numpy(gold[f"{k}.fragile"])
    share = float(fragile.float().mean())
    keep = (~fragile).flatten(1).to(DEV)
    # zero normals (a zero vector or two identical vectors in the chosen pair: colour 0.5) are checked apart, to the
    # 1e-6 floor alone: the reference's float32 leaves an FMA residue there, so its deviation is measured without them
    zero = t(gold[f"{k}.zero_normal"]).flatten(1)
    dev_p, dev_c = gold[f"{k}.dev"]
    err_p = float(((p.double() - t(gold[f"{k}.points"])).abs().amax(dim=-1) * keep).max())
    diff_c = (c.double() - t(gold[f"{k}.colors"])).abs().amax(dim=-1)
    err_c, err_z = float((diff_c * (keep & ~zero)).max()), float((diff_c * zero).max())
    print(f"{case} {border}: excluded {share:.2%}; points err {err_p:.2e} (bound {1e-6 + 2 * dev_p:.2e}), colors err "
          f"{err_c:.2e} (bound {1e-6 + 2 * dev_c:.2e}), at the {int(zero.sum())} zero normals {err_z:.2e} (bound 1e-6)")
    assert share <= 0.02 and not bool((zero & ~keep).any())
    assert err_p <= 1e-6 + 2 * dev_p
    assert err_c <= 1e-6 + 2 * dev_c
    assert err_z <= 1e-6


# ---------------------------------------------------------------------------------------
# 3. the border: the normal's neighbour at a clamped row / wrapped column is the median AT that pixel
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", BORDERS)
def test_border_neighbour_is_the_median_at_the_mapped_pixel(border):
    """Far returns planted in row 0 and column W-1.  Reading A (right): medians of the H x W map under the border rule,
    then the normal clamps rows / wraps columns INTO that map.  Reading B (wrong): pad the raw point map by the
    normal's reach (replicate rows, circular columns), take medians of the padded copy, read the normal's neighbours
    from it.  They differ along the edges; the kernel must be A."""
    from gans.coords import synthetic_angle_grid
    from gans.geometry import estimate_surface_normal
    from gans.utils import tanh_to_sigmoid
    H, W = 7, 9
    coord = bridge(H, W, synthetic_angle_grid(H))
    g = torch.Generator().manual_seed(2)
    depth = 10.0 + 2.0 * torch.rand(1, 1, H, W, generator=g)
    depth[:, :, 0, :] = 60.0 + 5.0 * torch.rand(1, 1, W, generator=g)
    depth[:, :, :, W - 1] = 60.0 + 5.0 * torch.rand(1, 1, H, generator=g)
    image = ((MIN_DEPTH / depth) * 2 - 1).to(DEV)
    p, c = fused(coord, image, border)
    pa, ca = unfused(coord, image, border)
    # reading B
    pm = coord.convert(tanh_to_sigmoid(image), "inv_depth_norm", "point_map")
    ext = F.pad(F.pad(pm, (0, 0, 2, 2), mode="replicate"), (2, 2, 0, 0), mode="circular")
    med_b = median3x3(ext, border)
    med_b[:, :, 2:-2, 2:-2] = median3x3(pm, border)     # inside the image both readings agree; the halo is B's own
    n_b = -estimate_surface_normal(med_b / coord.max_depth, d=2)[:, :, 2:-2, 2:-2]
    n_b[n_b != n_b] = 0.0
    cb = flat((n_b + 1) / 2)
    differs = (ca - cb).abs().amax(dim=-1).view(H, W) > 1e-3
    print(f"{border}: readings differ at {int(differs.sum())} of {H * W} pixels; rows {differs.any(dim=1).tolist()}")
    assert bool(differs[:2].any()) and bool(differs[:, -2:].any())      # the case tells the readings apart at both edges
    assert not bool(differs[2:-2, 2:-2].any())                          # and only there
    assert torch.equal(p, pa) and torch.equal(c, ca)
    assert float((c - cb).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------
# 4. argument checks: the status word, no launch
# ---------------------------------------------------------------------------------------
def test_frame_points_rejects_bad_arguments():
    import dgv2_native as N
    from gans.coords import synthetic_angle_grid
    H, W = 4, 8
    coord = bridge(H, W, synthetic_angle_grid(H))
    image = synthetic_image(1, H, W, 3)
    pts = torch.full((1, H * W, 3), 7.0, device=DEV)
    col = torch.full((1, H * W, 3), 7.0, device=DEV)
    f = N.lib.dgv2_frame_points
    a = coord.angle.contiguous()
    ok = (N.ptr(pts), N.ptr(col), N.ptr(image), N.ptr(a), 1, H, W, MIN_DEPTH, MAX_DEPTH, 0, N.stream())

    def with_(i, v):
        return ok[:i] + (v,) + ok[i + 1:]
    bad = {"d >= W (W = 2)": with_(6, 2), "W = 1": with_(6, 1), "B = 0": with_(4, 0), "H = 0": with_(5, 0),
           "points null": with_(0, None), "colors null": with_(1, None), "image null": with_(2, None),
           "angle null": with_(3, None), "border 2": with_(9, 2), "border -1": with_(9, -1)}
    for what, args in bad.items():
        assert f(*args) == -1, what     # DGV2_EINVAL, as dgv2_surface_normal for the same shapes
    assert N.lib.dgv2_surface_normal(N.ptr(pts), N.ptr(col), 1, H, 2, 2, 0, N.stream()) == -1
    torch.cuda.synchronize()
    assert bool((pts == 7.0).all()) and bool((col == 7.0).all())        # nothing was launched
    assert f(*ok) == 0
    torch.cuda.synchronize()
    assert not bool((pts == 7.0).any()) and not bool((col == 7.0).any())
    assert N.lib.dgv2_colorize(None, N.ptr(image), N.ptr(a), 1, H, W, 256, N.stream()) == -1
    assert N.lib.dgv2_colorize(N.ptr(pts), N.ptr(image), N.ptr(a), 1, H, W, 0, N.stream()) == -1


# ---------------------------------------------------------------------------------------
# 5. colorize
# ---------------------------------------------------------------------------------------
def test_colorize_equals_the_reference_and_embedding(gold):
    from gans.utils import colorize
    lut, x = gold["colorize.lut"], t(gold["colorize.x"])
    assert isinstance(lut, np.ndarray) and lut.dtype == np.float64
    y = colorize(x, cmap=lut)
    assert y.dtype == torch.float32 and tuple(y.shape) == (2, 3, 4, 16)
    assert torch.equal(y, t(gold["colorize.y"]))
    assert torch.equal(colorize(x[:, 0], cmap=lut), y)                  # (B,H,W) input
    index = (x[:, 0] * 256).clamp(0, 255).long()
    assert int(index.min()) == 0 and int(index.max()) == 255
    assert torch.equal(y, F.embedding(index, torch.tensor(lut, device=DEV).float()).permute(0, 3, 1, 2))
    small = np.random.RandomState(1).rand(7, 3)                          # an ndarray of another length
    index = (x[:, 0] * 7).clamp(0, 6).long()
    assert torch.equal(colorize(x, cmap=small), F.embedding(index, torch.tensor(small, device=DEV).float()).permute(0, 3, 1, 2))
    with pytest.raises(AssertionError):
        colorize(torch.zeros(1, 2, 4, 4, device=DEV), cmap=lut)


def test_colorize_by_name(gold):
    matplotlib = pytest.importorskip("matplotlib")
    import gans.utils as U
    x = t(gold["colorize.x"])
    want = U.colorize(x, cmap=matplotlib.colormaps["turbo"](np.linspace(0, 1, 256))[:, :3])
    assert torch.equal(U.colorize(x), want)
    lut = U._LUTS[("turbo", x.device)]
    assert torch.equal(U.colorize(x, "turbo"), want) and U._LUTS[("turbo", x.device)] is lut    # cached per device
    with pytest.raises(ValueError):
        U.colorize(x, cmap="no_such_colormap")


# ---------------------------------------------------------------------------------------
# 6. CoordBridge.convert(..., "normal_map")
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_convert_to_normal_map_from_every_source(gold, case):
    coord = case_bridge(gold, case)
    want = t(gold[f"normal.{case}.value"])
    keep = (~t(gold[f"normal.{case}.fragile"]))[:, None]
    assert float((~keep).float().mean()) <= 0.02
    for src, dev in zip(gold["normal.sources"], gold[f"normal.{case}.dev"]):
        got = coord.convert(t(gold[f"normal.{case}.src.{src}"]), str(src), "normal_map")
        assert got.shape == want.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        err = float(((got.double() - want).abs() * keep).max())
        print(f"{case} {src}: err {err:.2e} (bound {1e-6 + 2 * dev:.2e})")
        assert err <= 1e-6 + 2 * dev, (case, src)


def test_points_to_normal_2d_is_the_clamped_colour_of_the_normal_map(gold):
    from gans.utils import points_to_normal_2d
    case = "2x8x32"
    coord = case_bridge(gold, case)
    pm = t(gold[f"normal.{case}.src.point_map"])
    got = points_to_normal_2d(pm / coord.max_depth, mode="closest")
    want = ((coord.convert(pm, "point_map", "normal_map") + 1) / 2).clamp(0, 1)
    assert torch.equal(got, want) and float(got.min()) >= 0 and float(got.max()) <= 1


# ---------------------------------------------------------------------------------------
# 7. the walk, end to end
# ---------------------------------------------------------------------------------------
CKPT = os.path.join(GOLDEN, "checkpoint_small.pth")


@pytest.fixture(scope="module")
def small():
    from gans.coords import synthetic_angle_grid
    from gans.models.builder import build_generator
    from gans.pretrained import autoload_ckpt
    ck = autoload_ckpt(CKPT)
    G = build_generator(ck["cfg"].model.generator)
    G.load_state_dict(ck["G_ema"])
    G.eval().to(DEV)
    return G, bridge(16, 64, synthetic_angle_grid(16))


def test_interpolate_end_to_end(small):
    from gans.interpolation import LatentPath, interpolate, sample_anchors
    from gans.models.ops import native
    G, coord = small
    anchors = sample_anchors(G, 3, generator=torch.Generator(device=DEV).manual_seed(4))
    assert tuple(anchors.shape) == (3, G.synthesis_network.num_styles, 32)
    path = LatentPath(anchors)
    assert path.coef.is_cuda
    steps = path.steps(4)
    u = native.gumbel_uniform((1, 1, 16, 64), DEV)
    runs = [list(interpolate(G, coord, path, steps, truncation_psi=0.7, mode="3d", batch=5, u=u)) for _ in range(2)]
    assert len(runs[0]) == 12
    for (p, c), (p2, c2) in zip(*runs):
        assert tuple(p.shape) == tuple(c.shape) == (16 * 64, 3) and p.dtype == c.dtype == torch.float32
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(c).all())
        assert torch.equal(p, p2) and torch.equal(c, c2)                 # run to run
    # frame k = a direct generator call at path(t_k) + the unfused composition (in the walk's batches of 5, 5, 2: the
    # generator is only bit-reproducible at equal batch size)
    with torch.no_grad():
        for i in range(0, 12, 5):
            w = path(steps[i:i + 5]).float()
            o = G(z=w, angle=coord.angle, truncation_psi=0.7, input_w=True, noise={"gumbel_u": u.expand(len(w), 1, 16, 64)})
            p0, c0 = unfused(coord, o["image"], "zeros")
            for j in range(len(w)):
                assert torch.equal(runs[0][i + j][0], p0[j]) and torch.equal(runs[0][i + j][1], c0[j]), i + j
    assert float((runs[0][0][0] - runs[0][6][0]).abs().max()) > 1e-4     # the walk moves
    frames = list(interpolate(G, coord, path, steps[:3], mode="2d", batch=2, u=u))
    assert len(frames) == 3 and tuple(frames[0].shape) == (3, 3 * 16, 64)
    with pytest.raises(ValueError):
        next(interpolate(G, coord, path, steps, mode="4d"))


@pytest.mark.parametrize("mode", ["3d", "2d"])
def test_cli_writes_the_frames(tmp_path, mode):
    import demo_interpolation
    argv = ["--ckpt_path", CKPT, "--mode", mode, "--num_anchors", "2", "--frames_per_anchor", "3", "--batch", "4",
            "--out_dir", str(tmp_path)]
    demo_interpolation.main(argv + (["--num_frames", "7"] if mode == "2d" else []))
    if mode == "3d":
        pts, col = np.load(tmp_path / "points.npy"), np.load(tmp_path / "colors.npy")
        assert pts.shape == col.shape == (6, 16 * 64, 3) and pts.dtype == col.dtype == np.float32
        assert np.isfinite(pts).all() and np.isfinite(col).all()
    else:
        fr = np.load(tmp_path / "frames.npy")
        assert fr.shape == (7, 3, 3 * 16, 64) and fr.dtype == np.uint8
        assert not np.array_equal(fr[0], fr[3])                         # the walk moves
