"""train_gan.py end to end on the GPU: four iterations of the reduced 16 x 64 configuration on
synthetic scans, then a resumed run to iteration six.  The command line is what is under test, so each run is the script
in a child process under a time limit of its own; the second run starts only if the first one ended well."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from helpers import small_cfg

pytestmark = pytest.mark.gpu
B, H, W, BEV = 4, 16, 64, 512
RGB, ONE = (B, 3, H, W), (B, 1, H, W)
SHAPES = {"image": RGB, "image/spectrum": RGB, "normal": RGB, "pointcloud": (B, 3, BEV, BEV), "image/orig": RGB,
          "image/aug": RGB, "raydrop_prob": RGB, "raydrop_mask": ONE}
LIMIT = 240   # seconds for one run: interpreter start, library load, a handful of 16 x 64 iterations, image panels


def run_cli(tmp, *argv):
    import train_gan
    env = {k: v for k, v in os.environ.items() if k != "DGV2_POINTNET"}
    env["TORCH_HOME"] = str(tmp / "torch_home")   # an empty checkpoint cache: the PointNet weights are not on disk
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, train_gan.__file__, *argv]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp), env=env)
    assert r.returncode == 0, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    return r.stdout


def read_log(run_dir):
    with open(run_dir / "train_log.jsonl") as f:
        return [json.loads(line) for line in f]


@pytest.fixture(scope="module")
def first_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("train_gan")
    cfg = small_cfg()
    cfg.training.batch_size = B
    cfg.training.checkpoint.update(validation=2, save_model=2, save_image=2, save_stats=2)
    import train_gan
    config = tmp / "small.yaml"
    with open(config, "w") as f:
        yaml.safe_dump(train_gan.plain(cfg), f)
    run_dir = tmp / "run"
    out = run_cli(tmp, "--config", str(config), "--synthetic", "--out_dir", str(run_dir), "--max_iters", "4")
    return dict(tmp=tmp, config=config, run_dir=run_dir, stdout=out)


def test_log_lines(first_run):
    rows = read_log(first_run["run_dir"])
    assert [r["iteration"] for r in rows] == [2, 4] and [r["num_imgs"] for r in rows] == [2 * B, 4 * B]
    for r in rows:
        assert math.isfinite(r["loss/G/adversarial"]) and math.isfinite(r["loss/D/adversarial"])
        assert r["stats/ema_decay"] is not None
    printed = [json.loads(line) for line in first_run["stdout"].splitlines() if line.startswith("{")]
    assert printed == rows
    assert "iterations 1 .. 4" in first_run["stdout"]
    with open(first_run["run_dir"] / "training_config.yaml") as f:
        saved = yaml.safe_load(f)
    assert saved["training"]["batch_size_per_gpu"] == B and saved["training"]["num_gpus"] == 1
    assert saved["dataset"]["name"] == "synthetic"


def test_a_missing_pointnet_file_is_said_once_and_stops_nothing(first_run):
    assert first_run["stdout"].count("validation skipped") == 1
    assert not [r for r in read_log(first_run["run_dir"]) if any(k.startswith("score/") for k in r)]


def test_image_files(first_run):
    import train_gan
    for num_imgs in (2 * B, 4 * B):
        for tag, keys in (("real", train_gan.REAL_TAGS), ("fake", train_gan.FAKE_TAGS)):
            with np.load(first_run["run_dir"] / "images" / f"{tag}_{num_imgs:010d}.npz") as d:
                assert sorted(d.files) == sorted(keys), (tag, d.files)
                for k in keys:
                    assert d[k].dtype == np.uint8 and d[k].shape == SHAPES[k], (tag, k, d[k].dtype, d[k].shape)
                bev = d["pointcloud"]
                assert int(bev.max()) > int(bev.min()), tag
                assert int(d["image"].max()) > int(d["image"].min())
    assert set(train_gan.REAL_TAGS) | set(train_gan.FAKE_TAGS) == set(SHAPES)


def test_random_seed_of_the_config_reaches_the_run(first_run):
    """Two iterations of the same configuration under random_seed 1: another initial network and other draws than the
    first run's seed 0, so its first log line carries other losses."""
    import train_gan
    with open(first_run["config"]) as f:
        cfg = yaml.safe_load(f)
    assert cfg["random_seed"] == 0
    cfg["random_seed"] = 1
    cfg["training"]["checkpoint"].update(validation=100, save_model=100, save_image=100)
    config = first_run["tmp"] / "seed1.yaml"
    with open(config, "w") as f:
        yaml.safe_dump(cfg, f)
    run_dir = first_run["tmp"] / "run_seed1"
    run_cli(first_run["tmp"], "--config", str(config), "--synthetic", "--out_dir", str(run_dir), "--max_iters", "2")
    a, b = read_log(first_run["run_dir"])[0], read_log(run_dir)[0]
    assert a["iteration"] == b["iteration"] == 2
    assert a["loss/G/adversarial"] != b["loss/G/adversarial"] and a["loss/D/adversarial"] != b["loss/D/adversarial"]


def test_checkpoints_and_resume(first_run):
    from gans.pretrained import load_checkpoint
    models = first_run["run_dir"] / "models"
    assert sorted(p.name for p in models.iterdir()) == [f"checkpoint_{n:010d}.pth" for n in (2 * B, 4 * B)]
    for n in (2 * B, 4 * B):
        sd = load_checkpoint(str(models / f"checkpoint_{n:010d}.pth"))
        assert sd["step"] == n and {"G", "D", "G_ema", "A", "optim_G", "optim_D", "cfg"} <= set(sd)
        assert sd["cfg"].training.batch_size == B
    config_written = os.path.getmtime(first_run["run_dir"] / "training_config.yaml")
    out = run_cli(first_run["tmp"], "--config", str(first_run["config"]), "--synthetic", "--max_iters", "6",
                  "--resume", str(models / f"checkpoint_{4 * B:010d}.pth"))
    assert "iterations 5 .. 6" in out
    rows = read_log(first_run["run_dir"])
    assert [r["iteration"] for r in rows] == [2, 4, 6] and math.isfinite(rows[-1]["loss/G/adversarial"])
    assert load_checkpoint(str(models / f"checkpoint_{6 * B:010d}.pth"))["step"] == 6 * B
    assert os.path.getmtime(first_run["run_dir"] / "training_config.yaml") == config_written
    assert (first_run["run_dir"] / "images" / f"fake_{6 * B:010d}.npz").exists()
