"""The GAN evaluation driver on the small reference-written checkpoint: gans.evaluation.collect_sets / score_sets and
the test_gan.py command line, on synthetic scans (12 per set in batches of 5: the last batch is ragged)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
CKPT = os.path.join(GOLDEN, "checkpoint_small.pth")
N, BS, SEED = 12, 5, 3
H, W = 16, 64


def seeded_pointnet():
    from gans.metrics.pointnet import PointNet1
    torch.manual_seed(11)
    return PointNet1(k=16).eval().requires_grad_(False)


def loaders(cfg):
    from gans.evaluation import synthetic_loader
    kw = dict(num_scans=N, batch_size=BS, shape=(H, W), min_depth=cfg.dataset.min_depth, max_depth=cfg.dataset.max_depth,
              device=DEV)
    return synthetic_loader(seed=SEED, **kw), synthetic_loader(seed=SEED + 1, **kw)


@pytest.fixture(scope="module")
def run():
    from gans.evaluation import collect_sets
    from gans.pretrained import autoload_ckpt
    ckpt = autoload_ckpt(CKPT)
    record = {}
    train, test = loaders(ckpt["cfg"])
    summary = collect_sets(ckpt, train, test, N, BS, SEED, DEV, pointnet=seeded_pointnet(), record=record)
    return ckpt, summary, record


def test_collect_sets_returns_nine_tensors(run):
    _, summary, _ = run
    assert set(summary) == {f"{s}-{k}" for s in ("train", "test", "gen") for k in ("imgs", "points", "feats")}
    for s in ("train", "test", "gen"):
        assert tuple(summary[f"{s}-imgs"].shape) == (N, 1, H, W)
        assert tuple(summary[f"{s}-points"].shape) == (N, H * W, 3)     # min(cfg.validation.num_points = 2048, H * W)
        assert tuple(summary[f"{s}-feats"].shape) == (N, 1024 + 512 + 256 + 16)
        for k in ("imgs", "points", "feats"):
            t = summary[f"{s}-{k}"]
            assert t.device.type == "cpu" and t.dtype == torch.float32 and bool(torch.isfinite(t).all())
        assert float(summary[f"{s}-imgs"].min()) >= 0 and float(summary[f"{s}-imgs"].max()) <= 1
    assert not torch.equal(summary["train-imgs"], summary["test-imgs"])
    assert not torch.equal(summary["gen-imgs"][0], summary["gen-imgs"][1])


def test_without_features_no_pointnet_is_built(run, monkeypatch):
    import gans.metrics.pointnet as P
    from gans.evaluation import collect_sets
    ckpt, summary, _ = run
    monkeypatch.setattr(P, "pretrained_pointnet", lambda *a, **k: pytest.fail("a PointNet was built"))
    train, test = loaders(ckpt["cfg"])
    got = collect_sets(ckpt, train, test, N, BS, SEED, DEV, features=False)
    assert set(got) == {f"{s}-{k}" for s in ("train", "test", "gen") for k in ("imgs", "points")}
    for k, v in got.items():                                              # and the run is repeatable
        assert torch.equal(v, summary[k]), k


def test_real_images_follow_transform_reals(run):
    """test-imgs against the image lines of transform_reals (test_gan.py:106-114) written out in torch ops."""
    ckpt, summary, _ = run
    cfg = ckpt["cfg"]
    _, test = loaders(cfg)
    const = cfg.model.generator.measurement_kwargs.raydrop_const
    want = []
    for item in test:
        depth, mask = item["depth"].double(), item["mask"].double()
        valid = ((depth >= cfg.dataset.min_depth) & (depth <= cfg.dataset.max_depth) & (depth > 0)).double()
        imgs = 1 / (depth + 1e-11) * valid * cfg.dataset.min_depth        # depth -> inv_depth -> inv_depth_norm
        imgs = imgs * 2 - 1
        imgs = mask * imgs + (1 - mask) * const
        want.append(((imgs + 1) / 2).clamp(0, 1))
    want = torch.cat(want).cpu()
    assert tuple(want.shape) == (N, 1, H, W)
    assert float((summary["test-imgs"].double() - want).abs().max()) <= 1e-6
    assert float((want == 0).double().mean()) > 0.05                      # dropped rays are in the set


def test_every_sample_shares_the_one_uniform_map(run):
    _, _, record = run
    u, logit, mask = record["uniform"].double(), record["raydrop_logit"].double(), record["raydrop_mask"]
    assert tuple(u.shape) == (1, H, W) and tuple(logit.shape) == tuple(mask.shape) == (N, 1, H, W)
    eps = torch.finfo(torch.float32).eps
    assert float(u.min()) >= eps and float(u.max()) <= 1 - eps
    s = logit + (u.log() - (-u).log1p())[None]
    clear = s.abs() > 1e-5                                                # fp32 rounding may flip a sum this close to 0
    assert float(clear.double().mean()) > 0.99
    assert torch.equal((s > 0)[clear], mask[clear] > 0.5)
    assert mask.unique().tolist() == [0.0, 1.0]                           # rays are dropped and kept


def direct(summary, name):
    """The reference's metric blocks (test_gan.py:215-249) called one by one."""
    from gans.evaluation import subsample
    from gans.metrics.cov_mmd_1nna import compute_cov_mmd_1nna
    from gans.metrics.fpd_kpd import compute_frechet_distance, compute_squared_mmd
    from gans.metrics.jsd import compute_jsd
    from gans.metrics.swd import compute_swd
    g = {k: subsample(summary[f"gen-{k}"], 2048).to(DEV) for k in ("imgs", "points")}
    t = {k: subsample(summary[f"test-{k}"], 2048).to(DEV) for k in ("imgs", "points")}
    if name == "swd":
        return compute_swd(img1=g["imgs"], img2=t["imgs"])
    if name == "jsd":
        return {"jsd": compute_jsd(pcs_gen=g["points"] / 2, pcs_ref=t["points"] / 2)}
    if name == "1nna":
        return compute_cov_mmd_1nna(pcs_gen=g["points"], pcs_ref=t["points"], batch_size=256, metrics=("emd",),
                                    engine="pairwise")
    f1, f2 = summary["gen-feats"].numpy(), summary["train-feats"].numpy()
    return {name: compute_frechet_distance(f1, f2) if name == "fpd" else compute_squared_mmd(f1, f2)}


KEYS = {"swd": {"swd-16", "swd-mean"}, "jsd": {"jsd"}, "fpd": {"fpd"}, "kpd": {"kpd"},
        "1nna": {f"{k}-emd" for k in ("mmd", "mmd-sample", "cov")}
        | {f"1-nn-{k}-emd" for k in ("tp", "fp", "fn", "tn", "precision", "recall", "accuracy_t", "accuracy_f", "accuracy")}}


@pytest.mark.parametrize("name", ["swd", "jsd", "1nna", "fpd", "kpd"])
def test_score_sets_is_the_metric_on_the_returned_sets(run, name):
    from gans.evaluation import score_sets
    from gans.utils import init_random_seed
    _, summary, _ = run
    init_random_seed(5)
    got = score_sets(summary, [name])
    init_random_seed(5)
    want = direct(summary, name)
    assert set(got) == KEYS[name]
    assert got == want
    assert all(np.isfinite(v) for v in got.values())


def test_score_sets_all_five_keys(run):
    from gans.evaluation import score_sets
    _, summary, _ = run
    got = score_sets(summary, ["swd", "jsd", "1nna", "kpd"])
    assert set(got) == KEYS["swd"] | KEYS["jsd"] | KEYS["1nna"] | KEYS["kpd"]


@pytest.fixture(scope="module")
def pointnet_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("pointnet") / "cls_model_39.pth"
    torch.save(seeded_pointnet().state_dict(), path)
    return str(path)


def cli(capsys, pointnet_file, *extra):
    import test_gan
    argv = ["--ckpt_path", CKPT, "--synthetic", str(N), "--num_samples", str(N), "--batch_size_per_gpu", str(BS),
            "--random_seed", str(SEED), "--metrics", "swd,jsd,1nna,kpd", "--pointnet", pointnet_file]
    capsys.readouterr()
    assert test_gan.main(argv + list(extra)) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines[0].startswith("sets: ") and [ln.split(":")[0] for ln in lines[1:-1]] == ["swd", "jsd", "1nna", "kpd"]
    return lines[-1]


def test_cli_prints_the_same_json_line_twice(run, capsys, pointnet_file, tmp_path):
    from gans.evaluation import score_sets
    _, summary, _ = run
    out = tmp_path / "scores.json"
    first = cli(capsys, pointnet_file, "--out", str(out))
    second = cli(capsys, pointnet_file)
    assert first == second
    scores = json.loads(first, parse_constant=lambda c: pytest.fail(f"{c} in the JSON line"))
    assert set(scores) == KEYS["swd"] | KEYS["jsd"] | KEYS["1nna"] | KEYS["kpd"]
    assert json.loads(out.read_text()) == scores
    # the command line builds the sets the fixture built: the RNG-free scores are those of the fixture's summary
    want = score_sets(summary, ["jsd", "1nna"])
    assert {k: scores[k] for k in want} == want


def test_cli_batched_engine_agrees(run, capsys, pointnet_file):
    from gans.evaluation import score_sets
    pairwise = score_sets(run[1], ["1nna"], engine="pairwise")
    batched = json.loads(cli(capsys, pointnet_file, "--emd_engine", "batched"))
    assert set(k for k in batched if k.endswith("-emd")) == KEYS["1nna"] <= set(pairwise)
    assert abs(pairwise["mmd-emd"] - batched["mmd-emd"]) <= 2e-3 * batched["mmd-emd"]
