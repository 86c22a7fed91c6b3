"""CPU checks of the multi-GPU segmentation training: the command line's argument errors, the
sample stream's shards, the four dgv2_bn_* entries (declared, bound, argument checks that launch nothing), a numpy
restatement of the fold, and the module swap on the CPU.  Needs the built library, no GPU."""
import ctypes
import importlib
import itertools

import numpy as np
import pytest
import torch

from test_abi import parse_header
from test_semseg_train_cpu import _index_stream

BN_ENTRIES = {"dgv2_bn_partials": ["ptr", "ptr"] + ["int"] * 5 + ["ptr"],
              "dgv2_bn_apply": ["ptr"] * 10 + ["int"] * 5 + ["f32", "f32", "int", "ptr"],
              "dgv2_bn_bwd_partials": ["ptr"] * 5 + ["int"] * 5 + ["ptr"],
              "dgv2_bn_bwd_apply": ["ptr"] * 9 + ["int"] * 7 + ["ptr"]}


# ---- the command line -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    return importlib.import_module("train_semseg")


@pytest.mark.parametrize("n", [0, 9])
def test_cli_refuses_num_gpus_out_of_range(cli, n, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["--synthetic", "--num_gpus", str(n)])
    assert e.value.code == 2
    assert f"--num_gpus must be in 1 .. 8, got {n}" in capsys.readouterr().err
    assert not torch.cuda.is_initialized()


def test_cli_refuses_an_indivisible_batch(cli, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match=r"training.batch_size \(5\) must be divisible by --num_gpus \(2\)"):
        cli.main(["--synthetic", "--batch_size", "5", "--num_gpus", "2"])
    assert not torch.cuda.is_initialized()
    assert not list(tmp_path.iterdir())        # checked before anything is built: no log directory either


def test_cli_split_and_worker_bound(cli):
    args, cfg = cli.parse(["--synthetic", "--batch_size", "40", "--num_gpus", "8", "--sync_bn"])
    assert args.sync_bn and cfg.training.num_gpus == 8 and cfg.training.batch_size_per_gpu == 5
    args, cfg = cli.parse(["--synthetic"])
    assert not args.sync_bn and cfg.training.num_gpus == 1 and cfg.training.batch_size_per_gpu == cfg.training.batch_size
    for n in range(1, 9):
        _, cfg = cli.parse(["--synthetic", "--batch_size", str(8 * n), "--num_gpus", str(n)])
        cfg.training.num_workers = 64
        w = cli.workers_per_rank(cfg)
        assert w >= 0 and n * (w + 1) <= cli.CPU_BUDGET, (n, w)
        cfg.training.num_workers = 0
        assert cli.workers_per_rank(cfg) == 0


# ---- the sample stream ------------------------------------------------------------------------------------------------
def test_sampler_shards_are_disjoint_and_the_reference_stream():
    from semseg.utils import InfiniteSampler

    n, seed, take = 11, 5, 60
    shards = [[int(i) for i in itertools.islice(iter(InfiniteSampler(range(n), rank=r, num_replicas=2, seed=seed)), take)]
              for r in range(2)]
    whole = [int(i) for i in itertools.islice(iter(InfiniteSampler(range(n), seed=seed)), 2 * take)]
    # one stream, dealt out visit by visit: the two shards interleave to it, so no visit goes to both
    assert [v for pair in zip(*shards) for v in pair] == whole
    for r in range(2):
        assert shards[r] == list(itertools.islice(_index_stream(n, r, 2, seed), take))
    # the trainer seeds rank r with random_seed + r, as the reference does: two streams of their own
    mine = [int(i) for i in itertools.islice(iter(InfiniteSampler(range(n), rank=1, num_replicas=2, seed=seed + 1)), take)]
    assert mine == list(itertools.islice(_index_stream(n, 1, 2, seed + 1), take)) and mine != shards[1]


# ---- the ABI -----------------------------------------------------------------------------------------------------------
def test_entries_declared_and_bound():
    import dgv2_native as N

    protos = parse_header()
    names = {ctypes.c_void_p: "ptr", ctypes.c_int64: "i64", ctypes.c_float: "f32", ctypes.c_int: "int"}
    for entry, kinds in BN_ENTRIES.items():
        assert protos[entry] == kinds, entry
        assert [names[t] for t in N.SIGNATURES[entry]] == kinds, entry
        assert hasattr(N.lib, entry)
    assert N.ABI_VERSION == 60 and not [n for n in protos if n.startswith("dgv2_bn_") and n.endswith("_scratch")]


def test_entries_refuse_bad_arguments_without_a_launch():
    """Every refusal below is decided on the host before any launch, so fake non-null addresses are never read."""
    import dgv2_native as N

    p = 4096
    L = N.lib
    assert L.dgv2_bn_partials(None, p, 2, 3, 4, 5, N.F32, None) == N.EINVAL
    assert L.dgv2_bn_partials(p, p, 0, 3, 4, 5, N.F32, None) == N.EINVAL
    assert L.dgv2_bn_partials(p, p, 2, 3, 4, 5, 2, None) == N.EINVAL                      # fp8 is not a dtype here
    assert L.dgv2_bn_partials(p, p, 1 << 16, 1 << 16, 1, 1, N.F32, None) == N.EINVAL      # more planes than blocks
    ok = [p, p, p, None, None, None, p, p, None, None]
    assert L.dgv2_bn_apply(*ok, 1, 1, 3, 1, 1, 1e-5, 0.1, N.F32, None) == N.EINVAL        # one value per channel
    assert L.dgv2_bn_apply(*ok, 2, 1, 3, 4, 5, 1e-5, 0.1, N.F32, None) == N.EINVAL        # Btot < B
    assert L.dgv2_bn_apply(*ok, 2, 2, 3, 4, 5, -1.0, 0.1, N.F32, None) == N.EINVAL        # eps < 0
    assert L.dgv2_bn_apply(*ok, 2, 2, 3, 4, 5, 1e-5, float("nan"), N.F32, None) == N.EINVAL
    half = [p, p, p, p, None, None, p, p, None, None]
    assert L.dgv2_bn_apply(*half, 2, 2, 3, 4, 5, 1e-5, 0.1, N.F32, None) == N.EINVAL      # one running buffer alone
    cum = [p, p, p, p, p, None, p, p, None, None]
    assert L.dgv2_bn_apply(*cum, 2, 2, 3, 4, 5, 1e-5, -1.0, N.F32, None) == N.EINVAL      # cumulative without a count
    assert L.dgv2_bn_bwd_partials(p, p, p, None, p, 2, 3, 4, 5, N.F32, None) == N.EINVAL
    assert L.dgv2_bn_bwd_partials(p, p, p, p, p, 2, 3, 4, 5, 9, None) == N.EINVAL
    okb = [p, None, None, p, p, p, p, p, None]
    assert L.dgv2_bn_bwd_apply(*okb, 2, 4, 3, 3, 4, 5, N.F32, None) == N.EINVAL           # b_off + B > Btot
    assert L.dgv2_bn_bwd_apply(*okb, 2, 4, -1, 3, 4, 5, N.F32, None) == N.EINVAL
    assert L.dgv2_bn_bwd_apply(*okb, 1, 1, 0, 3, 1, 1, N.F32, None) == N.EINVAL           # one value per channel


def test_wrapper_has_no_cpu_path():
    from gans.models.ops import native

    x = torch.randn(2, 3, 4, 5)
    w = torch.ones(3)
    with pytest.raises(RuntimeError, match="must be a CUDA/HIP tensor"):
        native.sync_batch_norm(x, w, w, None, None, None, 1e-5, 0.1)
    with pytest.raises(RuntimeError, match="must be a CUDA/HIP tensor"):
        native.bn_partials(x)
    assert native.sync_batch_norm is native.syncbn.sync_batch_norm


# ---- the fold, restated ---------------------------------------------------------------------------------------------
def fold(x, pieces):
    """Per-sample float64 partials of each piece of the batch (any order INSIDE a plane, here numpy's), concatenated in
    sample order and folded one after the other: what dgv2_bn_partials / dgv2_bn_apply do across ranks."""
    parts = []
    for a, z in pieces:
        xs = x[a:z].astype(np.float64)
        parts.append(np.stack([xs.sum(axis=(2, 3)), (xs * xs).sum(axis=(2, 3))], axis=-1))
    part = np.concatenate(parts)
    s = np.zeros(x.shape[1])
    q = np.zeros(x.shape[1])
    for b in range(part.shape[0]):
        s = s + part[b, :, 0]
        q = q + part[b, :, 1]
    n = x.shape[0] * x.shape[2] * x.shape[3]
    mean = s / n
    return mean, np.maximum(q / n - mean * mean, 0.0)


@pytest.mark.parametrize("shape", [(4, 5, 7, 9), (4, 16, 3, 67), (8, 3, 1, 1), (6, 130, 2, 33)])
def test_numpy_fold_is_split_invariant_and_the_variance(shape):
    x = np.random.RandomState(sum(shape)).standard_normal(shape).astype(np.float32)
    B = shape[0]
    whole = fold(x, [(0, B)])
    for pieces in ([(0, B // 2), (B // 2, B)], [(b, b + 1) for b in range(B)], [(0, 1), (1, B)]):
        got = fold(x, pieces)
        assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    ref_var = x.astype(np.float64).var(axis=(0, 2, 3))
    ref_mean = x.astype(np.float64).mean(axis=(0, 2, 3))
    assert np.abs(whole[1] - ref_var).max() <= 1e-12 * np.abs(ref_var).max()
    assert np.abs(whole[0] - ref_mean).max() <= 1e-12 * max(1.0, np.abs(ref_mean).max())


# ---- the module on the CPU ------------------------------------------------------------------------------------------
def test_convert_on_the_cpu_is_batchnorm():
    """Away from the GPU the converted module is nn.BatchNorm2d.forward in both modes: same bits, same buffers."""
    from semseg.models import SyncBatchNorm2d, convert_sync_batchnorm
    from semseg.models.common import ConvNormReLU

    torch.manual_seed(0)
    a = ConvNormReLU(3, 8, 3, 1, 1, 0.1)
    b = ConvNormReLU(3, 8, 3, 1, 1, 0.1)
    b.load_state_dict(a.state_dict())
    keys = list(b.state_dict().keys())
    weight = b[1].weight
    assert convert_sync_batchnorm(b) is b and type(b[1]) is SyncBatchNorm2d and b[1].weight is weight
    assert list(b.state_dict().keys()) == keys and b[1].momentum == 0.1 and b[1].training
    assert type(convert_sync_batchnorm(torch.nn.BatchNorm2d(4).eval())) is SyncBatchNorm2d
    x = torch.randn(2, 3, 5, 6)
    for mode in (True, False):
        a.train(mode), b.train(mode)
        assert torch.equal(a(x), b(x))
    assert torch.equal(a[1].running_var, b[1].running_var) and int(b[1].num_batches_tracked) == 1
    a.load_state_dict(b.state_dict(), strict=True)
