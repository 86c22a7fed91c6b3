"""Host side of the GAN evaluation driver (test_gan.py, gans/evaluation.py): argument parsing, the subsampling rule,
the new entry's prototype, and the order in which a run fails.  No GPU."""
import os
import re

import pytest
import torch

from conftest import GOLDEN, ROOT


def test_parse_carries_the_reference_defaults():
    import test_gan
    args = test_gan.parse(["--ckpt_path", "x.pth"])
    assert args.ckpt_path == "x.pth"
    assert args.batch_size_per_gpu == 32 and args.random_seed == 0 and args.num_samples == 50_000
    assert args.metrics == ["swd", "jsd", "1nna", "fpd", "kpd"]
    assert args.synthetic is None and args.pointnet is None and args.out is None and args.data_root is None
    assert args.emd_engine in ("pairwise", "batched")
    args = test_gan.parse(["--ckpt_path", "x.pth", "--metrics", "jsd, 1nna", "--synthetic", "12", "--emd_engine", "batched"])
    assert args.metrics == ["jsd", "1nna"] and args.synthetic == 12 and args.emd_engine == "batched"


def test_unknown_metric_raises_at_parse_time():
    import test_gan
    with pytest.raises(ValueError, match="fid"):
        test_gan.parse(["--ckpt_path", "x.pth", "--metrics", "swd,fid"])
    from gans.evaluation import score_sets
    with pytest.raises(ValueError):
        score_sets({}, ["fid"])


@pytest.mark.parametrize("length", [5, 2048, 2049, 5000])
def test_subsample_is_the_reference_index_rule(length):
    from gans.evaluation import subsample
    n = 2048
    batch = torch.arange(length * 2).reshape(length, 2)
    got = subsample(batch, n)
    if length <= n:
        assert got is batch
    else:
        assert torch.equal(got, batch[torch.linspace(0, len(batch), n + 1)[:-1].long()])
        assert len(got) == n


def test_header_and_binding_hold_the_pairwise_entry():
    import dgv2_native as N
    from test_abi import parse_header
    want = ["ptr", "ptr", "ptr", "int", "int", "int", "int", "ptr"]
    assert parse_header()["dgv2_emd_pairwise_cost"] == want
    names = {N._c_ptr: "ptr", N._c_int: "int"}
    assert [names[t] for t in N.SIGNATURES["dgv2_emd_pairwise_cost"]] == want
    assert N.ABI_VERSION == 60 and N.lib.dgv2_abi_version() == 60
    src = open(os.path.join(ROOT, "include", "dgv2.h")).read()
    cap = int(re.search(r"#define DGV2_EMD_PAIR_MAX_POINTS (\d+)", src).group(1))
    from gans.metrics.distance.emd.earth_mover_distance import PAIR_MAX_POINTS
    assert cap == PAIR_MAX_POINTS >= 4096
    assert (2 * cap + 4 * 1024) * 4 <= 64 * 1024           # state + the 16 KB tile fit the LDS a workgroup may declare
    for needle in ("earth_mover_distance.cu:3-226", "cov_mmd_1nna.py:16-40"):
        assert needle in src, needle


def test_missing_pointnet_fails_before_anything_is_built(monkeypatch, tmp_path):
    import gans.models.builder as builder
    import test_gan

    def reached(*a, **k):
        pytest.fail("the generator was built although the PointNet file is missing")
    monkeypatch.setattr(builder, "build_generator", reached)
    monkeypatch.delenv("DGV2_POINTNET", raising=False)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path))
    ckpt = os.path.join(GOLDEN, "checkpoint_small.pth")
    with pytest.raises(FileNotFoundError, match="cls_model_39.pth"):
        test_gan.main(["--ckpt_path", ckpt, "--metrics", "fpd", "--synthetic", "4", "--num_samples", "4",
                       "--pointnet", str(tmp_path / "absent.pth")])
    from gans.evaluation import collect_sets
    with pytest.raises(FileNotFoundError, match="cls_model_39.pth"):
        collect_sets(ckpt, [], [], 4, 4, 0, "cpu")
