"""CPU checks of the bird's-eye-view feature: the two new C entries in the header and the
binding, their argument validation (nothing is launched for an invalid request, so no GPU is needed), make_Rt, the
argument logic of train_gan.py, and the float64 restatement of tests/bev_ref.py against splats worked out by hand.
Needs the built library, no GPU."""
import ctypes
import math
import os
import re

import pytest
import torch

import bev_ref
from conftest import ROOT
from test_abi import HEADER, parse_header

ENTRIES = {"dgv2_bev_render": ["ptr"] * 6 + ["int"] * 4 + ["f32", "ptr"],
           "dgv2_bilinear_splat": ["ptr"] * 4 + ["int"] * 5 + ["ptr"]}
P = 1 << 20   # a non-null address: an invalid request returns before anything could read it


def test_header_and_binding_declare_the_entries():
    import dgv2_native as N
    protos = parse_header()
    names = {ctypes.c_void_p: "ptr", ctypes.c_int64: "i64", ctypes.c_float: "f32", ctypes.c_int: "int"}
    for entry, kinds in ENTRIES.items():
        assert protos[entry] == kinds
        assert [names[t] for t in N.SIGNATURES[entry]] == kinds
        assert hasattr(N.lib, entry)
    src = open(HEADER).read()
    assert "render.py:21-127" in src
    assert not [n for n in protos if n.startswith(("dgv2_bev", "dgv2_bilinear")) and n.endswith("_scratch")]


def test_abi_version_did_not_move():
    import dgv2_native as N
    assert N.ABI_VERSION == 60 and N.lib.dgv2_abi_version() == 60
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 37\.", design, flags=re.M)


RENDER_OK = dict(out=P, acc=P, points=P, colors=P, R=None, t=None, B=1, N=8, C=3, size=16, focal=1.0)


@pytest.mark.parametrize("change", [dict(out=None), dict(acc=None), dict(points=None), dict(colors=None), dict(C=0),
                                    dict(C=5), dict(size=0), dict(N=1 << 22), dict(N=0), dict(B=0)],
                         ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_render_refuses_invalid_requests(change):
    import dgv2_native as N
    a = {**RENDER_OK, **change}
    rc = N.lib.dgv2_bev_render(a["out"], a["acc"], a["points"], a["colors"], a["R"], a["t"], a["B"], a["N"], a["C"],
                               a["size"], a["focal"], None)
    assert rc == N.EINVAL


SPLAT_OK = dict(out=P, acc=P, coords=P, values=P, B=1, N=8, C=1, H=4, W=6)


@pytest.mark.parametrize("change", [dict(out=None), dict(acc=None), dict(coords=None), dict(values=None), dict(C=0),
                                    dict(C=5), dict(H=0), dict(W=0), dict(N=1 << 22)],
                         ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_splat_refuses_invalid_requests(change):
    import dgv2_native as N
    a = {**SPLAT_OK, **change}
    rc = N.lib.dgv2_bilinear_splat(a["out"], a["acc"], a["coords"], a["values"], a["B"], a["N"], a["C"], a["H"], a["W"], None)
    assert rc == N.EINVAL


def test_wrappers_refuse_before_the_library():
    from gans.models.ops import native
    from gans.render import render_point_clouds
    pts, col = torch.zeros(2, 5, 3), torch.zeros(2, 5, 5)
    with pytest.raises(ValueError, match="C <= 4"):
        render_point_clouds(pts, col)
    with pytest.raises(ValueError, match="one for the whole batch"):
        render_point_clouds(pts, col[..., :3], R=torch.eye(3).repeat(2, 1, 1))
    with pytest.raises(ValueError, match="one for the whole batch"):
        render_point_clouds(pts, col[..., :3], t=torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.bev_render(pts, col[..., :3], 8)
    with pytest.raises(ValueError, match="points per sample"):
        native.bev_render(torch.zeros(1, 1, 3).expand(1, 1 << 22, 3), torch.zeros(1, 1, 1).expand(1, 1 << 22, 1), 8)


def test_value_scaling_bound_is_the_smallest_power_of_two():
    from gans.render import _pow2_bound, bilinear_rasterizer, render_point_clouds
    for peak, want in ((0.0, 1.0), (1.0, 1.0), (0.5, 0.5), (0.50001, 1.0), (0.9, 1.0), (3.5, 4.0), (4.0, 4.0), (2.0 ** -20, 2.0 ** -20)):
        assert float(_pow2_bound(torch.tensor([[peak, -peak / 2]]))) == want, peak
    with pytest.raises(ValueError, match="non-empty"):
        render_point_clouds(torch.zeros(1, 5, 3), torch.zeros(1, 5, 0))
    with pytest.raises(ValueError, match="non-empty"):
        bilinear_rasterizer(torch.zeros(1, 5, 2), torch.zeros(1, 5, 0), (4, 4))


def test_make_rt_quarter_turns():
    from gans.render import make_Rt
    h = math.pi / 2
    want = {
        "yaw": [[0, -1, 0], [1, 0, 0], [0, 0, 1]],      # x -> y
        "pitch": [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],    # z -> x
        "roll": [[1, 0, 0], [0, 0, -1], [0, 1, 0]],     # y -> z
    }
    for name, m in want.items():
        R, t = make_Rt(**{name: h}, x=1, y=2, z=3)
        assert R.shape == (1, 3, 3) and t.shape == (1, 3) and R.dtype == t.dtype == torch.float32
        assert torch.allclose(R[0], torch.tensor(m, dtype=torch.float32), atol=1e-7), name
        assert torch.allclose(R[0].double(), bev_ref.make_Rt(**{name: h})[0][0], atol=1e-7), name
        assert t.tolist() == [[1.0, 2.0, 3.0]]
    # the composition order: yaw . pitch . roll
    R, _ = make_Rt(roll=h, pitch=h, yaw=h)
    Rz, Ry, Rx = (torch.tensor(want[k], dtype=torch.float64) for k in ("yaw", "pitch", "roll"))
    assert torch.allclose(R[0].double(), Rz @ Ry @ Rx, atol=1e-6)
    assert torch.allclose(R[0].double(), bev_ref.make_Rt(h, h, h)[0][0], atol=1e-6)
    assert torch.equal(make_Rt()[0][0], torch.eye(3))


# ---------------------------------------------------------------------------- the restatement, by hand
def _point_at(row, col, size, depth=1.0):
    """The point that projects to raster position (row, col) at distance `depth` along z, no extrinsics, focal 1 (up to
    the 1e-8 in the projection's 1 / (p_z + 1e-8): the hand-made expectations below hold to about 1e-7)."""
    ux, uy = size - row, size - col
    return [(ux / size - 0.5) * depth, (uy / size - 0.5) * depth, -depth]


def test_restatement_one_point_with_fractions():
    size = 8
    pts = torch.tensor([[_point_at(3.25, 4.5, size)]], dtype=torch.float64)
    col = torch.tensor([[[0.5, 1.0]]], dtype=torch.float64)
    d = bev_ref.render(pts, col, size, details=True)
    e = math.exp(-3 * float(pts[0, 0].norm()))
    want_den = {(3, 4): 0.75 * 0.5, (3, 5): 0.75 * 0.5, (4, 4): 0.25 * 0.5, (4, 5): 0.25 * 0.5}
    den = torch.zeros(size, size, dtype=torch.float64)
    for (r, c), b in want_den.items():
        den[r, c] = e * b
    assert torch.allclose(d["den"][0], den, rtol=1e-6, atol=0)
    assert torch.allclose(d["esum"][0], (den > 0).double() * e, rtol=1e-6, atol=0)
    for (r, c), b in want_den.items():   # one contributor: its colour, up to the 1e-8 in the denominator
        assert torch.allclose(d["out"][0, :, r, c], col[0, 0] * (e * b / (e * b + 1e-8)), rtol=1e-6)
    assert float(d["out"][0].sum(dim=0)[den == 0].abs().max()) == 0
    assert not bool(d["fragile"].any()) and not bool(d["exclude"].any())
    # the same four weights from the rasterizer alone
    r = bev_ref.splat(torch.tensor([[3.25]], dtype=torch.float64), torch.tensor([[4.5]], dtype=torch.float64),
                      torch.ones(1, 1, 1, dtype=torch.float64), size, size)
    assert torch.allclose(r[0, 0], den / e, rtol=1e-6)


def test_restatement_point_across_the_border():
    """Raster row 7.5 at size 8: row 7 is in the image, row 8 is not.  u_x = 0.5 is inside (0, size - 1), so the colour
    stays; the lost corner's weight is simply gone (no renormalisation of the splat)."""
    size = 8
    pts = torch.tensor([[_point_at(7.5, 2.5, size)]], dtype=torch.float64)
    col = torch.ones(1, 1, 1, dtype=torch.float64)
    d = bev_ref.render(pts, col, size, details=True)
    e = math.exp(-3 * float(pts[0, 0].norm()))
    den = torch.zeros(size, size, dtype=torch.float64)
    den[7, 2] = den[7, 3] = e * 0.25
    assert torch.allclose(d["den"][0], den, rtol=1e-6, atol=0)
    assert torch.allclose(d["out"][0, 0][den > 0], torch.full((2,), e * 0.25 / (e * 0.25 + 1e-8), dtype=torch.float64))
    # row 0.5: u_x = 7.5 > size - 1, the point is not kept: weight, no colour
    pts = torch.tensor([[_point_at(0.5, 2.5, size)]], dtype=torch.float64)
    d = bev_ref.render(pts, col, size, details=True)
    assert float(d["den"][0, 0, 2]) > 0 and float(d["den"][0, 1, 2]) > 0 and float(d["out"].abs().max()) == 0


def test_restatement_unkept_point_dilutes_its_neighbour():
    size = 8
    a = _point_at(0.75, 3.5, size)        # u_x = 7.25 > size - 1 = 7: not kept; corners rows 0 (b .25) and 1 (b .75)
    b = _point_at(1.5, 3.5, size)         # kept; corners rows 1 and 2, b .5 each
    pts = torch.tensor([[a, b]], dtype=torch.float64)
    col = torch.ones(1, 2, 1, dtype=torch.float64)
    d = bev_ref.render(pts, col, size, details=True)
    ea, eb = (math.exp(-3 * float(p.norm())) for p in pts[0])
    # pixel (1, 3): a's 0.75 * 0.5 in the denominator only, b's 0.5 * 0.5 in both
    want = eb * 0.25 / (ea * 0.375 + eb * 0.25 + 1e-8)
    assert abs(float(d["out"][0, 0, 1, 3]) - want) < 1e-7 and want < 0.5
    assert float(d["out"][0, 0, 0, 3]) == 0 and float(d["den"][0, 0, 3]) > 0
    assert abs(float(d["out"][0, 0, 2, 3]) - eb * 0.25 / (eb * 0.25 + 1e-8)) < 1e-7


def test_restatement_drops_small_weights_and_flags_edges():
    size = 8
    # row fraction 0.0005: the far row's corners weigh 0.0005 * 0.5 < 1e-3 and are dropped
    d = bev_ref.render(torch.tensor([[_point_at(3.0005, 4.5, size)]], dtype=torch.float64),
                       torch.ones(1, 1, 1, dtype=torch.float64), size, details=True)
    assert float(d["den"][0, 4].abs().max()) == 0 and float(d["den"][0, 3, 4]) > 0
    # a coordinate on an integer is fragile and excludes its 3 x 3 block; a dropped ray (x = y = 0) never is
    d = bev_ref.render(torch.tensor([[_point_at(3.0, 4.5, size), [0.0, 0.0, 0.3]]], dtype=torch.float64),
                       torch.ones(1, 2, 1, dtype=torch.float64), size, details=True)
    assert d["fragile"].tolist() == [[True, False]]
    assert int(d["exclude"].sum()) == 9


def test_power_spectrum_restatement_of_a_plane_wave():
    H, W = 4, 8
    x = torch.cos(2 * math.pi * torch.arange(W, dtype=torch.float64) * 2 / W)[None].repeat(H, 1)
    s = bev_ref.power_spectrum_2d(x)
    # cos = two lines of amplitude 1/2 at columns W/2 +- 2 of the centred spectrum's row H/2
    assert abs(float(s[H // 2, W // 2 + 2]) - 10 * math.log10(0.25)) < 1e-9
    assert abs(float(s[H // 2, W // 2 - 2]) - 10 * math.log10(0.25)) < 1e-9
    from gans.utils import power_spectrum_2d
    got = power_spectrum_2d(x)
    big = s > -100
    assert int(big.sum()) == 2 and torch.allclose(got[big], s[big], rtol=1e-9)


# ---------------------------------------------------------------------------- train_gan.py without a GPU
def _train_gan():
    import train_gan
    return train_gan


CONFIG = os.path.join(ROOT, "configs", "gans", "dusty_v2.yaml")


def test_train_gan_dry_run_prints_the_derived_config(capsys):
    import yaml
    assert _train_gan().main(["--config", CONFIG, "--num_gpus", "4", "--dry_run", "--synthetic"]) == 0
    cfg = yaml.safe_load(capsys.readouterr().out)
    assert cfg["training"]["num_gpus"] == 4 and cfg["training"]["batch_size_per_gpu"] == 8
    assert cfg["training"]["rank"] == 0 and cfg["training"]["resume"] is None
    assert cfg["dataset"]["name"] == "synthetic"
    assert cfg["model"]["generator"]["arch"] == "dusty_v2"


def test_train_gan_argument_derivations(tmp_path):
    tg = _train_gan()
    args = tg.parse(["--config", CONFIG])
    assert (args.num_gpus, args.resume, args.dry_run, args.out_dir, args.max_iters, args.synthetic) == \
        (1, None, False, None, None, False)
    cfg = tg.derive_config(args)
    assert cfg.training.batch_size_per_gpu == cfg.training.batch_size == 32 and cfg.dataset.name == "kitti_raw"
    assert tg.total_iterations(args, cfg) == 25_000_000 // 32
    assert tg.total_iterations(tg.parse(["--config", CONFIG, "--max_iters", "7"]), cfg) == 7
    import datetime
    d = tg.log_dir_for(args, cfg, now=datetime.datetime(2024, 1, 2, 3, 4, 5))
    assert d.as_posix() == "logs/gans/kitti_raw/dusty_v2+dusty_v2/20240102T030405"
    assert tg.log_dir_for(tg.parse(["--config", CONFIG, "--out_dir", str(tmp_path)]), cfg) == tmp_path
    # --resume: the log directory is two levels above the checkpoint, whatever --out_dir says
    ck = tmp_path / "run" / "models" / "checkpoint_0000000016.pth"
    args = tg.parse(["--config", CONFIG, "--resume", str(ck), "--out_dir", "elsewhere"])
    assert tg.log_dir_for(args, cfg) == tmp_path / "run" and tg.derive_config(args).training.resume == str(ck)
    with pytest.raises(ValueError, match="divisible"):
        tg.derive_config(tg.parse(["--config", CONFIG, "--num_gpus", "3"]))
    for bad in ("0", "17"):
        with pytest.raises(SystemExit):
            tg.parse(["--config", CONFIG, "--num_gpus", bad])
    assert tg.parse(["--config", CONFIG, "--num_gpus", "16"]).num_gpus == 16


def test_train_gan_seeds_a_single_process_from_the_config():
    """One rank joins no process group, but the seed must still come from cfg.random_seed (+ rank): the weights, z_fixed
    and the device's random stream follow torch's seed at the moment Trainer(cfg) is built."""
    import random
    import numpy as np
    from gans.config import to_config
    tg = _train_gan()
    draws = {}
    saved = (torch.get_rng_state(), np.random.get_state(), random.getstate(), os.environ.get("PYTHONHASHSEED"))
    try:
        _check_seeding(tg, to_config, draws, random, np)
    finally:   # the generators of the tests that follow stay as they were
        torch.set_rng_state(saved[0])
        np.random.set_state(saved[1])
        random.setstate(saved[2])
        os.environ.pop("PYTHONHASHSEED", None)
        if saved[3] is not None:
            os.environ["PYTHONHASHSEED"] = saved[3]
    src = open(os.path.join(ROOT, "train_gan.py")).read()
    assert src.index("seed_and_connect(rank, cfg, temp_dir)") < src.index("trainer = Trainer(cfg")


def _check_seeding(tg, to_config, draws, random, np):
    for seed in (3, 11):
        cfg = to_config({"random_seed": seed, "training": {"num_gpus": 1}})
        tg.seed_and_connect(0, cfg, None)
        assert torch.initial_seed() == seed and not torch.distributed.is_initialized()
        draws[seed] = (torch.randn(4), np.random.rand(), random.random())
    assert not torch.equal(draws[3][0], draws[11][0]) and draws[3][1:] != draws[11][1:]
    tg.seed_and_connect(0, to_config({"random_seed": 3, "training": {"num_gpus": 1}}), None)
    assert torch.equal(torch.randn(4), draws[3][0])
    tg.seed_and_connect(2, to_config({"random_seed": 3, "training": {"num_gpus": 1}}), None)
    assert torch.initial_seed() == 5


def test_train_gan_names_no_runtime_knobs_and_never_replaces_its_process():
    src = open(os.path.join(ROOT, "train_gan.py")).read()
    assert "os.exec" not in src and "execv" not in src and "os.environ[" not in src and "putenv" not in src
    assert 'get_context("spawn")' in src
    assert tuple(_train_gan().REAL_TAGS + _train_gan().FAKE_TAGS).count("pointcloud") == 2


def test_json_line_writes_non_finite_as_null():
    line = _train_gan().json_line({"iteration": 3, "a": float("nan"), "b": 1.5})
    assert line == '{"iteration": 3, "a": null, "b": 1.5}'
