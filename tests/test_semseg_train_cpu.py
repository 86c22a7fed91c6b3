"""CPU checks of the segmentation training step: the index stream of InfiniteSampler, the
file-backed datasets against a numpy restatement, the builders on the two fixture configurations, the three ABI 60
entries of csrc/sgd.hip (declared, bound, argument checks that launch nothing) and the lr schedule.  Needs the built
library, no GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_abi import HEADER, parse_header

CFG_DIR = os.path.join(GOLDEN, "semseg_cfg")
SGD_ENTRIES = ("dgv2_sumsq_list", "dgv2_clip_prep", "dgv2_sgd_step")


# ---------------------------------------------------------------------------------------------------------------------
# 1. InfiniteSampler
# ---------------------------------------------------------------------------------------------------------------------
def _index_stream(n, rank, num_replicas, seed, window_size=0.5):
    """Restatement: shuffle once; visit positions cyclically; after each visit swap the entry with the one
    randint(window) places behind it; a replica sees every num_replicas-th visit."""
    rng = np.random.RandomState(seed)
    order = np.arange(n)
    rng.shuffle(order)
    window = int(np.rint(n * window_size))
    visit = 0
    while True:
        i = visit % n
        if visit % num_replicas == rank:
            yield int(order[i])
        if window >= 2:
            j = (i - rng.randint(window)) % n
            order[i], order[j] = order[j], order[i]
        visit += 1


def test_infinite_sampler_order():
    from semseg.utils import InfiniteSampler

    got = [int(i) for i in itertools.islice(iter(InfiniteSampler(range(7), rank=1, num_replicas=2, seed=3)), 50)]
    want = list(itertools.islice(_index_stream(7, 1, 2, 3), 50))
    assert got == want
    assert set(got) <= set(range(7)) and len(set(got)) > 1
    plain = [int(i) for i in itertools.islice(iter(InfiniteSampler(range(3), shuffle=False)), 7)]
    assert plain == [0, 1, 2, 0, 1, 2, 0]


# ---------------------------------------------------------------------------------------------------------------------
# 2. datasets
# ---------------------------------------------------------------------------------------------------------------------
K_MEAN = np.array([10.88, 0.23, -1.04, 0.21, 12.12, 0.0], dtype=np.float32)
K_STD = np.array([11.47, 6.91, 0.86, 0.16, 12.32, 1.0], dtype=np.float32)
G_MEAN, G_STD = K_MEAN[[0, 1, 2, 4, 5]], K_STD[[0, 1, 2, 4, 5]]
H, W = 4, 8


def _scan(seed, channels):
    """[H, W, channels] float32: geometry channels in (-5, 20), depth 0 on a quarter of the rays, labels 0..3 last."""
    rng = np.random.RandomState(seed)
    pts = rng.uniform(-5, 20, size=(H, W, channels)).astype(np.float32)
    pts[..., channels - 2] = np.where(rng.rand(H, W) < 0.25, 0.0, rng.uniform(2, 60, size=(H, W))).astype(np.float32)
    pts[..., channels - 1] = rng.randint(0, 4, size=(H, W)).astype(np.float32)
    pts[0, 0, channels - 1] = 3.0     # at least one cyclist ...
    pts[0, 0, channels - 2] = 0.0     # ... on a missing ray: the label must survive the mask
    return pts


@pytest.fixture
def kitti_root(tmp_path):
    (tmp_path / "lidar_2d").mkdir()
    (tmp_path / "ImageSet").mkdir()
    names = [f"scan_{i}" for i in range(3)]
    for i, name in enumerate(names):
        np.save(tmp_path / "lidar_2d" / (name + ".npy"), _scan(10 + i, 6))
    (tmp_path / "ImageSet" / "train.txt").write_text("\n".join(names) + "\n")
    return tmp_path, names


def _expected(scan, mean, std, depth_ch):
    chw = scan.transpose(2, 0, 1).copy()
    mask = (chw[depth_ch] > 0).astype(np.float32)
    chw[:-1] *= mask[None]                                   # masked first ...
    chw = (chw - mean[:, None, None]) / std[:, None, None]   # ... then normalised; the label row passes (0, 1)
    return chw, mask


def test_kitti_items_match_restatement(kitti_root):
    from semseg.datasets import KITTIRawFrontal

    root, names = kitti_root
    ds = KITTIRawFrontal(root=root, split="train", shape=(H, W))
    assert len(ds) == 3 and ds.class_list == ["unknown", "car", "pedestrian", "cyclist"]
    for i, name in enumerate(names):
        scan = np.load(root / "lidar_2d" / (name + ".npy"))
        chw, mask = _expected(scan, K_MEAN, K_STD, 4)
        item = ds[i]
        assert set(item) == {"xyz", "reflectance", "depth", "label", "mask"}
        assert item["xyz"].dtype == item["depth"].dtype == item["mask"].dtype == torch.float32
        assert item["label"].dtype == torch.int64
        assert item["xyz"].shape == (3, H, W) and item["reflectance"].shape == (1, H, W) and item["depth"].shape == (1, H, W)
        assert item["label"].shape == (H, W) and item["mask"].shape == (H, W)
        np.testing.assert_array_equal(item["mask"].numpy(), mask)
        np.testing.assert_allclose(item["xyz"].numpy(), chw[:3], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(item["reflectance"].numpy(), chw[3:4], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(item["depth"].numpy(), chw[4:5], rtol=1e-6, atol=1e-7)
        np.testing.assert_array_equal(item["label"].numpy(), scan[..., 5].astype(np.int64))   # untouched by the mask
        # a missing ray holds the normalised ZERO, not zero
        miss = mask == 0
        np.testing.assert_allclose(item["depth"].numpy()[0][miss], -K_MEAN[4] / K_STD[4], rtol=1e-6)
    assert int(ds[0]["label"][0, 0]) == 3 and float(ds[0]["mask"][0, 0]) == 0


def test_kitti_flip_and_omit_cyclist(kitti_root, monkeypatch):
    from semseg.datasets import KITTIRawFrontal

    root, _ = kitti_root
    plain = KITTIRawFrontal(root=root, split="train", shape=(H, W))[1]
    ds = KITTIRawFrontal(root=root, split="train", shape=(H, W), flip=True)
    monkeypatch.setattr(np.random, "rand", lambda *a: 0.75)
    item = ds[1]
    np.testing.assert_array_equal(item["mask"].numpy(), plain["mask"].numpy()[:, ::-1])
    np.testing.assert_array_equal(item["label"].numpy(), plain["label"].numpy()[:, ::-1])
    np.testing.assert_array_equal(item["depth"].numpy(), plain["depth"].numpy()[..., ::-1])
    np.testing.assert_array_equal(item["xyz"].numpy()[[0, 2]], plain["xyz"].numpy()[[0, 2]][..., ::-1])
    np.testing.assert_array_equal(item["xyz"].numpy()[1], -plain["xyz"].numpy()[1][:, ::-1])   # the NORMALISED y is negated
    monkeypatch.setattr(np.random, "rand", lambda *a: 0.25)
    np.testing.assert_array_equal(ds[1]["xyz"].numpy(), plain["xyz"].numpy())

    omit = KITTIRawFrontal(root=root, split="train", shape=(H, W), omit_cyclist=True)
    assert omit.class_list == ["unknown", "car", "pedestrian"]
    want = plain["label"].numpy().copy()
    assert (want == 3).any()
    want[want == 3] = 0
    np.testing.assert_array_equal(omit[1]["label"].numpy(), want)


def test_gta_raydrop_maps(tmp_path):
    from semseg.datasets import GTALiDAR, GTALiDAR_GAN

    (tmp_path / "GTAV" / "seq").mkdir(parents=True)
    (tmp_path / "GTAV_noise_v2" / "seq").mkdir(parents=True)
    scans = [_scan(20 + i, 5) for i in range(2)]
    for i, scan in enumerate(scans):
        np.save(tmp_path / "GTAV" / "seq" / f"{i:04d}.npy", scan)
        np.save(tmp_path / "GTAV_noise_v2" / "seq" / f"{i:04d}.npy", np.full((H, W), float(i), dtype=np.float32))
    chw, mask = _expected(scans[0], G_MEAN, G_STD, 3)
    for raydrop in (None, np.ones((H, W), dtype=np.float32)):
        ds = GTALiDAR(root=tmp_path, shape=(H, W), raydrop_p=raydrop)
        assert len(ds) == 2 and ds.class_list == ["unknown", "car", "pedestrian"]
        item = ds[0]
        assert set(item) == {"xyz", "depth", "label", "mask"}
        np.testing.assert_array_equal(item["mask"].numpy(), mask)          # all-ones map: the mask is unchanged
        np.testing.assert_allclose(item["xyz"].numpy(), chw[:3], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(item["depth"].numpy(), chw[3:4], rtol=1e-6, atol=1e-7)
        np.testing.assert_array_equal(item["label"].numpy(), scans[0][..., 4].astype(np.int64))
    item = GTALiDAR(root=tmp_path, shape=(H, W), raydrop_p=np.zeros((H, W), dtype=np.float32))[0]
    assert float(item["mask"].sum()) == 0                                  # all-zeros map: the mask is cleared
    np.testing.assert_allclose(item["depth"].numpy(), np.full((1, H, W), -G_MEAN[3] / G_STD[3]), rtol=1e-6)
    gan = GTALiDAR_GAN(root=tmp_path, shape=(H, W), gan_dir="GTAV_noise_v2")
    assert float(gan[0]["mask"].sum()) == 0                                # scan 0's map is all zeros,
    np.testing.assert_array_equal(gan[1]["mask"].numpy(), (scans[1][..., 3] > 0).astype(np.float32))   # scan 1's all ones
    assert "GTAV_noise_v2" in repr(gan)


def test_synthetic_frontal_is_deterministic():
    from semseg.datasets import SyntheticFrontal

    a, b = SyntheticFrontal(4, (3, 48), 3, seed=5), SyntheticFrontal(4, (3, 48), 3, seed=5)
    for k, v in a[2].items():
        assert torch.equal(v, b[2][k]), k
    item = a[1]
    assert item["xyz"].shape == (3, 3, 48) and item["depth"].shape == (1, 3, 48) and item["label"].dtype == torch.int64
    assert 0 <= int(item["label"].min()) and int(item["label"].max()) <= 2 and len(a.class_list) == 3
    assert not torch.equal(a[1]["depth"], a[2]["depth"])
    assert not torch.equal(a[1]["depth"], SyntheticFrontal(4, (3, 48), 3, seed=6)[1]["depth"])
    assert 0 < float(item["mask"].mean()) < 1


# ---------------------------------------------------------------------------------------------------------------------
# 3. configurations and builders
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, classes", [("real2real.yaml", 4), ("sim2real_w_gan_noise_dustyv2.yaml", 3)])
def test_fixture_configs_build(name, classes):
    from semseg.config import default_config, load_config
    from semseg.models import MaskedSegLoss, SqueezeSegV2
    from semseg.trainer import build_criterion, build_model

    cfg = load_config(os.path.join(CFG_DIR, name))
    assert cfg.dataset.num_classes == classes and cfg.training.lr == 0.05 and cfg.use_amp is True
    assert set(default_config()) == set(cfg) and set(default_config().training) == set(cfg.training)
    model = build_model(cfg, pretrained_weights=False)
    assert isinstance(model, SqueezeSegV2)
    prior = torch.tensor(cfg.dataset.logit_bias)
    assert torch.allclose(model.decoder.head[1].bias.detach(), -torch.log((1 - prior) / prior))
    assert torch.allclose(torch.sigmoid(model.decoder.head[1].bias.detach()), prior, atol=1e-6)
    assert model.decoder.head[1].bias.requires_grad
    for key in ("theta_gamma", "theta_alpha", "theta_beta"):
        assert isinstance(cfg.arch.crf[key], list) and len(cfg.arch.crf[key]) == classes
        assert torch.equal(getattr(model.crf, key), torch.tensor(cfg.arch.crf[key], dtype=torch.float32)), key
    assert model.crf.num_iters == 3 and model.crf.kernel_size == (3, 5)
    crit = build_criterion(cfg)
    assert isinstance(crit, MaskedSegLoss) and crit.gamma == 2.0
    assert torch.equal(crit.alpha, torch.tensor(cfg.loss.cls_weight))
    cfg.loss.name = "cross_entropy"
    assert build_criterion(cfg).gamma == 0.0
    cfg.loss.name = "dice"
    with pytest.raises(ValueError):
        build_criterion(cfg)


# ---------------------------------------------------------------------------------------------------------------------
# 4. ABI 60
# ---------------------------------------------------------------------------------------------------------------------
def test_sgd_entries_declared_and_bound():
    import dgv2_native as N

    protos = parse_header()
    for name in SGD_ENTRIES:
        assert name in protos and name in N.SIGNATURES, name
    assert N.ABI_VERSION == 60 and N.lib.dgv2_abi_version() == 60
    src = open(HEADER).read()
    assert re.search(r"#define\s+DGV2_SUMSQ_PARTS\s+64\b", src) and N.SUMSQ_PARTS == 64
    assert re.search(r"#define\s+DGV2_SGD_N_MAX\s+\(2147483647 - \(1 << 17\)\)", src)
    for needle in ("train_semseg.py:201-212", "278-283", "360-362", "d = sc[1]*g + weight_decay*p"):
        assert needle in src, needle
    # the workspace is the caller's: no _scratch sibling, no _needed parameter
    scratch = {n for n in protos if n.endswith("_scratch")}
    assert len(scratch) == 15 and not [n for n in scratch if "sgd" in n or "sumsq" in n or "clip" in n]
    decl = re.search(r"int\s+dgv2_sumsq_list\s*\(([^;]*?)\)\s*;", src, flags=re.S).group(1)
    assert "needed" not in decl


def test_sgd_step_rejects_bad_arguments():
    """Every refusal returns DGV2_EINVAL before anything is launched: the pointers below are never dereferenced (no
    GPU is present where this runs)."""
    import dgv2_native as N

    fake = 0x1000
    ptrs = lambda n: (ctypes.c_void_p * n)(*([fake] * n))   # noqa: E731
    ints = lambda n, v=4: (ctypes.c_int * n)(*([v] * n))   # noqa: E731
    step = N.lib.dgv2_sgd_step

    def call(p, g, m, n, L, sc, momentum=0.9):
        return step(p, g, m, n, L, sc, 0.1, momentum, 0.0, None)

    assert call(ptrs(1), ptrs(1), ptrs(1), ints(1), 0, fake) == N.EINVAL
    assert call(ptrs(73), ptrs(73), ptrs(73), ints(73), 73, fake) == N.EINVAL
    assert call(ptrs(2), ptrs(2), ptrs(2), ints(2), 2, None) == N.EINVAL
    assert call(ptrs(2), ptrs(2), ptrs(2), (ctypes.c_int * 2)(4, -1), 2, fake) == N.EINVAL
    assert call(None, ptrs(2), ptrs(2), ints(2), 2, fake) == N.EINVAL
    assert call(ptrs(2), None, ptrs(2), ints(2), 2, fake) == N.EINVAL
    assert call(ptrs(2), ptrs(2), None, ints(2), 2, fake) == N.EINVAL
    assert call(ptrs(2), (ctypes.c_void_p * 2)(fake, None), ptrs(2), ints(2), 2, fake) == N.EINVAL
    assert call(ptrs(2), ptrs(2), (ctypes.c_void_p * 2)(fake, None), ints(2), 2, fake) == N.EINVAL
    assert call(ptrs(2), ptrs(2), ptrs(2), None, 2, fake) == N.EINVAL
    # lengths the kernels' int indices cannot step through: refused, just below they pass the check (not run here)
    assert N.SGD_N_MAX == 2 ** 31 - 1 - 2 ** 17
    assert call(ptrs(1), ptrs(1), ptrs(1), ints(1, N.SGD_N_MAX + 1), 1, fake) == N.EINVAL
    assert call(ptrs(1), ptrs(1), ptrs(1), ints(1, 2 ** 31 - 1), 1, fake) == N.EINVAL
    assert N.lib.dgv2_sumsq_list(ptrs(1), ints(1, N.SGD_N_MAX + 1), 1, fake, None) == N.EINVAL
    assert N.lib.dgv2_sumsq_list(ptrs(1), ints(1), 0, fake, None) == N.EINVAL
    assert N.lib.dgv2_sumsq_list(ptrs(73), ints(73), 73, fake, None) == N.EINVAL
    assert N.lib.dgv2_sumsq_list(ptrs(1), ints(1, -1), 1, fake, None) == N.EINVAL
    assert N.lib.dgv2_sumsq_list(ptrs(1), ints(1), 1, None, None) == N.EINVAL
    assert N.lib.dgv2_clip_prep(None, 64, 1.0, None, 2.0, 0.5, 2000, fake, None) == N.EINVAL
    assert N.lib.dgv2_clip_prep(fake, 64, 1.0, None, 2.0, 0.5, 2000, None, None) == N.EINVAL
    assert N.lib.dgv2_clip_prep(fake, 0, 1.0, None, 2.0, 0.5, 2000, fake, None) == N.EINVAL


def test_fused_step_rejects_unsupported_options():
    from gans.models.ops.native import fused_clip_sgd_step

    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.zeros(4)
    for kw in ({"dampening": 0.1, "momentum": 0.9}, {"nesterov": True, "momentum": 0.9}, {"maximize": True}):
        with pytest.raises(RuntimeError, match="unsupported optimizer options"):
            fused_clip_sgd_step(torch.optim.SGD([p], lr=0.1, **kw), 1.0)
    with pytest.raises(RuntimeError):     # CPU tensors: no fallback
        fused_clip_sgd_step(torch.optim.SGD([p], lr=0.1), 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the schedule
# ---------------------------------------------------------------------------------------------------------------------
def test_lr_schedule():
    """lr during steps 1, 2 and 3 with lr_decay_steps = 2: the decay lands after every second step."""
    lr, decay, every = 0.05, 0.5, 2
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=lr, momentum=0.9)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=decay)
    seen = []
    for step in range(1, 4):
        seen.append(opt.param_groups[0]["lr"])
        opt.step()
        if step % every == 0:
            sched.step()
    assert seen == [lr, lr, lr * decay]
    assert opt.param_groups[0]["lr"] == lr * decay and sched.get_last_lr() == [lr * decay]
