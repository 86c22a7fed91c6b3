"""Host side of the latent walk (gans/interpolation.py, gans/utils.py, demo_interpolation.py): no GPU.

LatentPath keeps the reference's scipy spline as polynomial pieces; here they are evaluated in float64 on the CPU
against scipy.interpolate.interp1d itself and against what the reference recorded (tests/golden/interpolation.npz,
written by tests/golden/make_interpolation_golden.py).  `rel` is the project's: max |got - want| / max |want|."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.interpolate
import torch

from conftest import GOLDEN, PKG, ROOT


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "interpolation.npz"))
    return {k: d[k] for k in d.files}


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def reference_interp(zs):
    n = len(zs)
    return scipy.interpolate.interp1d(x=np.arange(-n * 2, n * 3), y=np.tile(zs, [5] + [1] * (zs.ndim - 1)), kind="cubic",
                                      axis=0)


def test_exports():
    import gans.interpolation as I
    for name in ("sample_anchors", "LatentPath", "interpolate"):
        assert name in I.__all__ and callable(getattr(I, name))


@pytest.mark.parametrize("n", [2, 3, 10])
def test_path_matches_the_recorded_reference(gold, n):
    from gans.interpolation import LatentPath
    path = LatentPath(torch.from_numpy(gold[f"interp.{n}.anchors"]))
    assert path.coef.dtype == torch.float64 and tuple(path.coef.shape) == (n, 4, 6)
    got = path(torch.from_numpy(gold[f"interp.{n}.pos"]))
    assert tuple(got.shape) == (17, 6)
    assert rel(got, gold[f"interp.{n}.value"]) < 1e-12


@pytest.mark.parametrize("n", [1, 2, 3, 10])
def test_path_matches_scipy_directly(n):
    """Anchors shaped like a generator's w ([N, styles, D]), dense positions over the whole lap."""
    from gans.interpolation import LatentPath
    zs = np.random.RandomState(n).randn(n, 3, 8)
    path = LatentPath(torch.from_numpy(zs))
    t = np.linspace(0, n, 257, endpoint=False)
    got = path(torch.from_numpy(t))
    assert tuple(got.shape) == (257, 3, 8)
    assert rel(got, reference_interp(zs)(t)) < 1e-12


def test_path_is_closed_and_interpolates_the_anchors():
    from gans.interpolation import LatentPath
    n = 5
    zs = np.random.RandomState(0).randn(n, 2, 16)
    path = LatentPath(torch.from_numpy(zs))
    assert rel(path(torch.arange(n, dtype=torch.float64)), zs) < 1e-12          # the knots
    end = path(torch.tensor([n - 1e-9]))
    assert float((end - path(torch.tensor([0.0]))).abs().max()) < 1e-5          # t -> N- meets t = 0
    # and smoothly.  The tiled not-a-knot spline is periodic only up to what its end conditions, two laps away, leak
    # into the middle lap: a factor (2 - sqrt 3) ~ 0.27 per knot, 2N = 10 knots: ~2e-6 of the data's scale
    c = path.coef
    d_end = c[-1, 1] + 2 * c[-1, 2] + 3 * c[-1, 3]
    assert float((d_end - c[0, 1]).abs().max()) < 1e-3 * float(c[:, 1].abs().max())


def test_path_keeps_the_anchors_dtype_and_takes_float32_positions():
    from gans.interpolation import LatentPath
    zs = torch.randn(3, 2, 4, generator=torch.Generator().manual_seed(1))
    path = LatentPath(zs)
    assert path.coef.dtype == torch.float32
    t = np.array([0.0, 0.25, 1.5, 2.999])
    got = path(torch.from_numpy(t))               # float64 positions are cast to the pieces' dtype
    assert got.dtype == torch.float32
    assert rel(got, reference_interp(zs.double().numpy())(t)) < 1e-5


def test_steps_equal_the_reference_linspace():
    from gans.interpolation import LatentPath
    for n, per in ((10, 90), (3, 4)):
        path = LatentPath(torch.zeros(n, 2))
        steps = path.steps() if per == 90 else path.steps(per)
        want = np.linspace(0, n, int(per * n), endpoint=False)     # demo_interpolation.py:153,160
        assert steps.dtype == torch.float64 and np.array_equal(steps.numpy(), want)


def test_cycle():
    from gans.utils import cycle
    it = cycle([1, 2, 3])
    assert list(itertools.islice(it, 7)) == [1, 2, 3, 1, 2, 3, 1]


def test_cli_defaults_equal_the_reference():
    import demo_interpolation
    args = demo_interpolation.parse(["--ckpt_path", "x.pth"])
    # demo_interpolation.py:103-110
    assert (args.ckpt_path, args.mode, args.num_anchors, args.truncation_psi, args.seed, args.device) == \
        ("x.pth", "2d", 10, 0.7, 0, "cuda")
    assert (args.frames_per_anchor, args.num_frames, args.batch, args.border, args.out_dir) == (90, None, 8, "zeros", ".")
    with pytest.raises(SystemExit):
        demo_interpolation.parse([])                                  # --ckpt_path is required
    with pytest.raises(SystemExit):
        demo_interpolation.parse(["--ckpt_path", "x", "--mode", "4d"])


def test_cli_imports_no_display_packages():
    for f in ("demo_interpolation.py", os.path.join("dusty-gan-v2_amd", "gans", "interpolation.py")):
        src = open(os.path.join(ROOT, f)).read()
        for mod in ("cv2", "polyscope", "kornia", "einops"):
            assert f"import {mod}" not in src and f"from {mod}" not in src, (f, mod)


def test_utils_does_not_import_matplotlib_at_import_time():
    """In a fresh interpreter: importing gans.utils (and the walk) leaves matplotlib unloaded."""
    code = "import sys, gans.utils, gans.interpolation; assert hasattr(gans.utils, 'colorize'); " \
           "sys.exit(int('matplotlib' in sys.modules))"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])


def test_frame_ops_fail_loudly_on_cpu_tensors():
    from gans.coords import CoordBridge, synthetic_angle_grid
    from gans.models.ops import native
    from gans.utils import colorize
    coord = CoordBridge(8, 32, 1.45, 80.0, angle_array=synthetic_angle_grid(8, 64))
    with pytest.raises(RuntimeError):
        native.frame_points(torch.zeros(1, 1, 8, 32), coord.angle, 1.45, 80.0)
    with pytest.raises(RuntimeError):
        colorize(torch.zeros(1, 1, 8, 32), cmap=np.zeros((256, 3)))
    with pytest.raises(RuntimeError):
        coord.convert(torch.zeros(1, 3, 8, 32), "point_map", "normal_map")
    with pytest.raises(ValueError):
        native.frame_points(torch.zeros(1, 1, 8, 32), coord.angle, 1.45, 80.0, border="reflect")
