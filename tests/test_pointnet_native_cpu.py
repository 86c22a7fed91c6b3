"""CPU checks around the native PointNet trunk: the C entry's declaration and refusals, the
float64 restatement the GPU tests lean on against the fixture of the reference's own module (tests/golden/
make_pointnet_golden.py), and the untouched library path of gans.metrics.pointnet.  Needs the built library, no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import pointnet_ref as R
from test_abi import HEADER, parse_header


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


@pytest.fixture(scope="module")
def net():
    from gans.metrics.pointnet import PointNet1
    m = PointNet1(k=16)
    m.load_state_dict(R.state_dict(), strict=True)
    return m.eval().requires_grad_(False)


def test_header_and_binding_declare_the_entry():
    import dgv2_native as N
    want = ["ptr"] * 9 + ["int"] * 3 + ["ptr"]
    assert parse_header()["dgv2_pointnet_trunk"] == want
    assert N.SIGNATURES["dgv2_pointnet_trunk"] == [ctypes.c_void_p] * 9 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    assert "dgv2_pointnet_trunk_scratch" not in N.SIGNATURES       # no workspace: nothing for the library to size
    src = open(HEADER).read()
    assert "gans/metrics/pointnet.py:22-26" in src and ":46-55" in src


def test_wrapper_constants_mirror_the_header():
    from gans.models.ops.native import pointnet as W
    src = open(HEADER).read()
    assert f"#define DGV2_POINTNET_TILE {W.P}\n" in src and f"#define DGV2_POINTNET_FEATURES {W.FEATURES}\n" in src
    assert "#define DGV2_POINTNET_MAX_TILES (1 << 28)\n" in src and W.MAX_TILES == 1 << 28
    assert W.S >= W.P and W.S % W.P == 0
    assert W.pointnet_supported(1, 1) and W.pointnet_supported(32, 32768)
    assert not W.pointnet_supported(0, 5) and not W.pointnet_supported(5, 0)
    assert W.pointnet_supported(1 << 28, W.P) and not W.pointnet_supported(1 << 28, W.P + 1)


def test_refusals_launch_nothing():
    """Every refusal is decided on the host before a launch: the entry never looks behind the pointers, so small
    16-byte-aligned integers stand in for them here."""
    import dgv2_native as N
    f = N.lib.dgv2_pointnet_trunk
    ok = [64 * (i + 1) for i in range(9)]        # feat, pts, trans, w1, b1, w2, b2, w3, b3

    def rc(ptrs=ok, B=2, n=100, relu=0):
        return f(*ptrs, B, n, relu, None)
    for i in (0, 1, 3, 4, 5, 6, 7, 8):           # every pointer but trans is required
        assert rc(ok[:i] + [None] + ok[i + 1:]) == N.EINVAL, i
    assert rc(B=0) == N.EINVAL and rc(B=-1) == N.EINVAL
    assert rc(n=0) == N.EINVAL and rc(n=-7) == N.EINVAL
    assert rc(relu=2) == N.EINVAL
    assert rc(ok[:5] + [ok[5] + 4] + ok[6:]) == N.EINVAL and rc(ok[:7] + [ok[7] + 8] + ok[8:]) == N.EINVAL   # misaligned w2 / w3
    assert rc(B=1 << 24, n=2 ** 31 - 1) == N.ENOTSUP
    assert rc(B=(1 << 28) + 1, n=1) == N.ENOTSUP
    assert rc(B=1 << 28, n=129) == N.ENOTSUP


@pytest.mark.parametrize("n", R.CASES)
def test_restatement_equals_the_reference_in_float64(fx, n):
    sd = R.state_dict()
    pts = R.case_points(n)
    top = float(fx[f"{n}/max64"])
    assert top == float(np.abs(fx[f"{n}/ref64"]).max())
    assert float(fx[f"{n}/e_ref"]) == float(np.abs(fx[f"{n}/ref32"].astype(np.float64) - fx[f"{n}/ref64"]).max())
    trans, stn = R.stn(sd, pts)
    for got, key in ((R.pointnet1(sd, pts), "ref64"), (trans, "trans64"), (stn, "stn64")):
        assert got.dtype == torch.float64
        assert np.abs(got.numpy() - fx[f"{n}/{key}"]).max() <= 1e-12 * top, key


@pytest.mark.parametrize("n", R.CASES)
def test_cpu_inputs_take_the_library_path_unchanged(fx, net, n, monkeypatch):
    """CPU tensors never reach the kernel, whatever the switch says: the results are the library composition's, within
    the existing 1e-4 of the reference's float32 output, and the same bits with the switch on, off, and twice."""
    import dgv2_native as N
    from gans.metrics import pointnet as M
    monkeypatch.setattr(N.lib, "dgv2_pointnet_trunk", lambda *a: pytest.fail("the kernel was called for a CPU tensor"))
    x = R.case_points(n).transpose(1, 2)
    assert M.POINTNET_NATIVE in (True, False)
    outs = []
    for flag in (False, True, False):
        monkeypatch.setattr(M, "POINTNET_NATIVE", flag)
        assert not M.uses_native(x.transpose(1, 2))
        outs.append(net(x))
    want = fx[f"{n}/ref32"]
    assert outs[0].shape == (2, 1808)
    assert np.abs(outs[0].numpy() - want).max() <= 1e-4 * np.abs(want).max()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_wrapper_checks_its_arguments():
    from gans.models.ops.native import pointnet as W
    sd = R.state_dict()
    layers = R.trunk_layers(sd, "feat.", torch.float32)
    pts = R.case_points(5)
    with pytest.raises(RuntimeError):                       # no CPU fallback inside the wrapper
        W.pointnet_trunk(pts, None, *layers, False)
    with pytest.raises(ValueError):
        W.pointnet_trunk(pts.transpose(1, 2), None, *layers, False)
    with pytest.raises(ValueError):
        W.pointnet_trunk(pts[:, :0], None, *layers, False)
    with pytest.raises(ValueError):
        W.pointnet_trunk(pts.double(), None, *layers, False)
    with pytest.raises(ValueError):
        W.pointnet_trunk(pts, torch.zeros(2, 3, 4), *layers, False)
    with pytest.raises(ValueError):
        W.pointnet_trunk(pts, None, layers[0], layers[2], layers[1], False)
