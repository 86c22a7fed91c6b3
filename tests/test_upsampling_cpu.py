"""CPU checks around beam upsampling: the two C entries' declarations and refusals, the wrappers'
argument checks (the library is never reached), depth_summary, the restatements the GPU tests lean on against the
fixture of the reference's own depth.py, the command line's parser and its checks before any generator exists.  Needs the
built library, no GPU."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import upsampling_ref as R
from conftest import GOLDEN
from test_abi import HEADER, parse_header


def test_header_and_binding_declare_the_entries():
    import dgv2_native as N
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    protos = parse_header()
    assert protos["dgv2_beam_split"] == ["ptr"] * 6 + ["int"] * 6 + ["ptr"]
    assert protos["dgv2_depth_score"] == ["ptr"] * 4 + ["int", "i64", "ptr"]
    assert N.SIGNATURES["dgv2_beam_split"] == [P] * 6 + [I] * 6 + [P]
    assert N.SIGNATURES["dgv2_depth_score"] == [P] * 4 + [I, L, P]
    assert "dgv2_beam_split_scratch" not in N.SIGNATURES and "dgv2_depth_score_scratch" not in N.SIGNATURES
    assert "dgv2_beam_split_scratch" not in protos and "dgv2_depth_score_scratch" not in protos
    assert N.ABI_VERSION == 60 and N.lib.dgv2_abi_version() == 60
    assert "gans/metrics/depth.py:4-45" in open(HEADER).read()


def test_refusals_launch_nothing():
    """Every refusal is decided on the host before a launch: the entries never look behind the pointers, so small
    16-byte-aligned integers stand in for them."""
    import dgv2_native as N
    ok = [64 * (i + 1) for i in range(6)]          # recon, recon_mask, obs, held, depth, valid

    def split(ptrs=ok, B=2, H=8, W=5, factor=4, offset=1, mode=2):
        return N.lib.dgv2_beam_split(*ptrs, B, H, W, factor, offset, mode, None)
    for i in (2, 3, 4):
        assert split(ok[:i] + [None] + ok[i + 1:]) == N.EINVAL, i
    for i in (0, 1):                               # the reconstruction pointers are needed where something is reconstructed
        assert split(ok[:i] + [None] + ok[i + 1:], mode=1) == N.EINVAL and split(ok[:i] + [None] + ok[i + 1:], mode=2) == N.EINVAL
    assert split(B=0) == N.EINVAL and split(H=0) == N.EINVAL and split(W=0) == N.EINVAL
    assert split(factor=0) == N.EINVAL and split(factor=9) == N.EINVAL and split(factor=-1) == N.EINVAL
    assert split(offset=4) == N.EINVAL and split(offset=-1) == N.EINVAL
    assert split(mode=3) == N.EINVAL and split(mode=-1) == N.EINVAL
    assert split(B=1 << 20, H=1 << 10, W=1 << 10) == N.EINVAL      # more than 2^31 - 1 blocks

    def score(ptrs=ok[:4], B=2, n=100):
        return N.lib.dgv2_depth_score(*ptrs, B, n, None)
    for i in (0, 1, 2):
        assert score(ok[:i] + [None] + ok[i + 1:4]) == N.EINVAL, i
    assert score(B=0) == N.EINVAL and score(B=-3) == N.EINVAL
    assert score(n=0) == N.EINVAL and score(n=-1) == N.EINVAL and score(n=2 ** 31) == N.EINVAL


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the device: lets the wrappers' checks AFTER the device check run without one."""
    is_cuda = True


def _fake(t):
    return t.as_subclass(_FakeCuda)


@pytest.fixture
def unreachable(monkeypatch):
    import dgv2_native as N
    for name in ("dgv2_beam_split", "dgv2_depth_score"):
        monkeypatch.setattr(N.lib, name, lambda *a, _n=name: pytest.fail(f"{_n} was reached"))


def test_wrappers_check_their_arguments(unreachable):
    from gans.models.ops import native
    depth, valid = R.make_scan(1, 2, 8, 6, 4, 0)
    with pytest.raises(RuntimeError):                           # CPU tensors: no fallback
        native.beam_split(depth, valid, 4)
    with pytest.raises(RuntimeError):
        native.beam_split(_fake(depth), valid, 4)
    with pytest.raises(RuntimeError):
        native.depth_score(depth, depth, valid)
    with pytest.raises(RuntimeError):
        native.depth_score(_fake(depth), depth)
    d, v = _fake(depth), _fake(valid)
    bad_split = [
        lambda: native.beam_split(_fake(depth.double()), v, 4),                         # float64
        lambda: native.beam_split(d, _fake(valid.double()), 4),
        lambda: native.beam_split(_fake(depth.transpose(2, 3)), _fake(valid.transpose(2, 3)), 4),     # non-contiguous
        lambda: native.beam_split(d, _fake(valid[:, :, :, :5]), 4),                     # mismatched shapes
        lambda: native.beam_split(_fake(depth[:, 0]), _fake(valid[:, 0]), 4),           # not [B,1,H,W]
        lambda: native.beam_split(_fake(depth.repeat(1, 2, 1, 1)), None, 4),
        lambda: native.beam_split(d, v, 0),                                             # factor
        lambda: native.beam_split(d, v, 9),
        lambda: native.beam_split(d, v, 4, offset=4),                                   # offset >= factor
        lambda: native.beam_split(d, v, 4, offset=-1),
        lambda: native.beam_split(d, v, 4, mode="cubic"),                               # unknown mode
        lambda: native.beam_split(d, v, 4, mode=2),
    ]
    bad_score = [
        lambda: native.depth_score(_fake(depth.double()), d),
        lambda: native.depth_score(d, _fake(depth.double())),
        lambda: native.depth_score(d, d, _fake(valid.bool())),
        lambda: native.depth_score(_fake(depth.transpose(2, 3)), _fake(depth.transpose(2, 3))),
        lambda: native.depth_score(d, _fake(depth[:1])),
        lambda: native.depth_score(d, d, _fake(valid[:, :, :4])),
        lambda: native.depth_score(_fake(depth[:0]), _fake(depth[:0])),
    ]
    for i, f in enumerate(bad_split + bad_score):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} was accepted")


def test_depth_summary_by_hand():
    from gans.models.ops import native
    sums = torch.tensor([[2.0, 8.0, 64.0, 1.0, 3.0, 4.0, 4.0, 4.0],
                         [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    got = native.depth_summary(sums)
    assert tuple(got) == R.KEYS == native.DEPTH_KEYS
    want = {"abs_rel": 0.5, "sq_rel": 2.0, "rmse": 4.0, "rmse_log": 0.5, "accuracy_1": 0.75, "accuracy_2": 1.0, "accuracy_3": 1.0}
    for k, v in got.items():
        assert v.dtype == torch.float64 and tuple(v.shape) == (2,)
        assert float(v[0]) == want[k], k
        assert math.isnan(float(v[1])), k                      # 0 / 0, as the reference's masked mean
    assert float(native.depth_summary(sums[0])["rmse"]) == 4.0         # a single [8] row (a pooled total)
    with pytest.raises(ValueError):
        native.depth_summary(sums[:, :7])


def test_restatements_agree_with_the_reference_fixture():
    """The float32 restatement and the float64 oracle the GPU tests compare the kernel with, against the values the
    reference's own depth.py gave (tests/golden/make_golden.py), and against this package's tensor-op port of it."""
    from gans.metrics import depth as D
    from gans.models.ops import native
    d = np.load(os.path.join(GOLDEN, "metrics.npz"))
    ref, gen, mask = (torch.from_numpy(d[k]) for k in ("depth_ref", "depth_gen", "depth_mask"))
    got = native.depth_summary(R.score_sums_f32(ref, gen, mask))
    oracle = R.summary_f64(ref, gen, mask)
    port = {**D.compute_depth_error(ref, gen, mask), **D.compute_depth_accuracy(ref, gen, mask)}
    for k in R.KEYS:
        np.testing.assert_allclose(got[k].numpy(), d["depth_" + k], rtol=1e-5, err_msg=k)
        np.testing.assert_allclose(oracle[k].numpy(), d["depth_" + k], rtol=1e-5, err_msg=k)
        np.testing.assert_allclose(port[k].numpy(), d["depth_" + k], rtol=1e-5, err_msg=k)


@pytest.mark.parametrize("seed,shape", list(zip(R.SEEDS, R.SHAPES)))
def test_seeded_inputs_keep_clear_of_the_thresholds(seed, shape):
    """What the GPU tests assume of their inputs, for the reference alone: no pixel's float64 delta within 1e-6 relative
    of a threshold, at least 22 unmasked pixels per image, and the reference's float32 result within 1e-5 of float64."""
    from gans.metrics import depth as D
    ref, gen, mask = R.make_inputs(seed, shape)
    assert R.threshold_margin(ref, gen) > 1e-6
    assert int(mask.flatten(1).sum(dim=1).min()) >= 22
    oracle = R.summary_f64(ref, gen, mask)
    port = {**D.compute_depth_error(ref, gen, mask), **D.compute_depth_accuracy(ref, gen, mask)}
    for k in R.KEYS:
        np.testing.assert_allclose(port[k].double().numpy(), oracle[k].numpy(), rtol=1e-5, err_msg=k)


def test_beam_split_restatement_by_hand():
    """H = 7, factor 3, offset 1: rows 1 and 4 are observed; rows 0 and 5, 6 have one neighbour only."""
    depth = torch.arange(1.0, 8.0).reshape(1, 1, 7, 1).repeat(1, 1, 1, 2).contiguous()      # row h holds h + 1
    valid = torch.ones(1, 1, 7, 2)
    valid[0, 0, 4, 1] = 0.0                                     # column 1 loses its lower observed row
    lin = R.beam_split_ref(depth, valid, 3, 1, "linear")
    near = R.beam_split_ref(depth, valid, 3, 1, "nearest")
    t1, t2 = torch.tensor(1.0) / torch.tensor(3.0), torch.tensor(2.0) / torch.tensor(3.0)      # float32, as the contract's t
    assert lin["obs"][0, 0, :, 0].tolist() == [0, 1, 0, 0, 1, 0, 0] and lin["held"][0, 0, :, 0].tolist() == [1, 0, 1, 1, 0, 1, 1]
    assert lin["obs"][0, 0, :, 1].tolist() == [0, 1, 0, 0, 0, 0, 0] and lin["held"][0, 0, :, 1].tolist() == [1, 0, 1, 1, 0, 1, 1]
    assert lin["recon"][0, 0, :, 0].tolist() == [2.0, 2.0, float(2 + t1 * 3), float(2 + t2 * 3), 5.0, 5.0, 5.0]
    assert near["recon"][0, 0, :, 0].tolist() == [2.0, 2.0, 2.0, 5.0, 5.0, 5.0, 5.0]
    assert lin["recon"][0, 0, :, 1].tolist() == [2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0]
    assert near["recon"][0, 0, :, 1].tolist() == [2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0]
    assert lin["recon_mask"][0, 0, :, 1].tolist() == [1, 1, 1, 1, 0, 0, 0] and torch.equal(lin["recon_mask"], near["recon_mask"])
    none = R.beam_split_ref(depth, None, 3, 1, "none")
    assert set(none) == {"obs", "held"} and float(none["obs"].sum()) == 4 and float(none["held"].sum()) == 10


def test_parser_defaults_and_checks_before_any_generator(tmp_path, monkeypatch, capsys):
    import eval_upsampling as E
    import gans.models.builder as builder
    monkeypatch.setattr(builder, "build_generator", lambda *a, **k: pytest.fail("a generator was built"))
    ckpt = tmp_path / "ckpt.pth"
    ckpt.write_bytes(b"")
    a = E.parse(["--ckpt_path", str(ckpt)])
    assert (a.factor, a.offset, a.methods, a.num_steps, a.batch_size, a.latent_type) == (4, 0, ("nearest", "linear", "gan"), 500, 32, "w+")
    assert (a.no_graph, a.limit, a.out, a.random_seed, a.data_root, a.synthetic) == (False, None, None, 0, None, None)
    assert tuple(E.METHODS) == tuple(__import__("gans.upsampling", fromlist=["METHODS"]).METHODS)
    # a missing checkpoint with gan requested ends the run in the parser
    for argv in (["--synthetic", "4"], ["--synthetic", "4", "--ckpt_path", str(tmp_path / "missing.pth")],
                 ["--ckpt_path", str(tmp_path / "missing.pth"), "--methods", "linear,gan"]):
        with pytest.raises(SystemExit):
            E.main(argv)
    assert "ckpt_path" in capsys.readouterr().err
    # without gan no checkpoint is needed
    b = E.parse(["--synthetic", "4", "--methods", "nearest"])
    assert b.methods == ("nearest",) and b.ckpt_path is None and b.synthetic == 4
    for argv in (["--methods", "cubic"], ["--methods", "nearest,nearest"], ["--methods", ""],
                 ["--methods", "nearest", "--factor", "0"], ["--methods", "nearest", "--offset", "4"],
                 ["--methods", "nearest", "--synthetic", "0"], ["--methods", "nearest", "--latent_type", "q"]):
        with pytest.raises(SystemExit):
            E.parse(argv)


def test_gan_without_a_fitter_raises(unreachable):
    from gans.upsampling import UpsamplingBenchmark, upsample_scans
    depth, valid = R.make_scan(2, 1, 8, 6, 4, 0)
    with pytest.raises(ValueError, match="fitter"):
        upsample_scans(depth, valid, factor=4, method="gan")
    with pytest.raises(ValueError):
        upsample_scans(depth, valid, factor=4, method="cubic")
    with pytest.raises(ValueError, match="fitter"):
        UpsamplingBenchmark(("linear", "gan")).update(depth, valid)
    with pytest.raises(ValueError):
        UpsamplingBenchmark(("linear", "linear"))
    with pytest.raises(ValueError):
        UpsamplingBenchmark(("nearest",), factor=4, offset=4)
