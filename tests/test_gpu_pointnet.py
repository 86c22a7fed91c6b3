"""GPU checks of the native PointNet trunk (csrc/pointnet.hip) against the float64 fixture of the
reference's own module (tests/golden/pointnet.npz) and the float64 restatement tests/pointnet_ref.py.

The bound everywhere is the float32 bound of DESIGN.md 31.3: max|gpu - ref64| <= 4 E_ref + 2^-22 max|ref64|, E_ref being
the deviation of a float32 library evaluation (the reference's module for the fixture cases) from the same float64
values.  Every figure is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import pointnet_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


@pytest.fixture(scope="module")
def sd():
    return R.state_dict()


@pytest.fixture(scope="module")
def W():
    from gans.models.ops.native import pointnet
    return pointnet


@pytest.fixture(scope="module")
def nets(sd):
    """(the module on the device, the same module on the CPU)"""
    from gans.metrics.pointnet import PointNet1
    out = []
    for dev in (DEV, "cpu"):
        m = PointNet1(k=16)
        m.load_state_dict(sd, strict=True)
        out.append(m.eval().requires_grad_(False).to(dev))
    return out


def dev_layers(sd, prefix, b3_shift=0.0):
    """The float32 folded layers of a trunk on the device (what gans.metrics.pointnet._fold hands the kernel)."""
    layers = [(w.contiguous().to(DEV), b.contiguous().to(DEV)) for w, b in R.trunk_layers(sd, prefix, torch.float32)]
    layers[2] = (layers[2][0], layers[2][1] + b3_shift)
    return layers


def ref_layers(sd, prefix, dtype, b3_shift=0.0):
    layers = R.trunk_layers(sd, prefix, dtype)
    layers[2] = (layers[2][0], layers[2][1] + b3_shift)
    return layers


def edge_points(seed, B, n):
    import recipe
    return recipe.point_clouds(seed, B, n) + torch.tensor(R.SHIFT)


def check(tag, got, ref64, e_ref, factor=1.0):
    top = float(ref64.abs().max())
    err = float((got.double().cpu() - ref64).abs().max())
    lim = factor * R.bound(e_ref, top)
    print(f"{tag}: err {err:.3e}  E_ref {float(e_ref):.3e}  max|ref64| {top:.3f}  bound {lim:.3e}  err/bound {err / lim:.3f}")
    assert err <= lim, (tag, err, lim)
    return err / lim


# ---- 1. trunk parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.CASES)
def test_trunk_parity(fx, sd, W, n):
    """Both trunks' weights x relu_last 0 / 1 x trans NULL / given, on the float32 rounding of the fixture's float64
    transform (the trunk apart from the transformer's own error).  The two combinations the model uses are held to the
    fixture itself, the others to the restatement (which the CPU tests hold to the fixture within 1e-12)."""
    pts = R.case_points(n)
    trans64 = torch.from_numpy(fx[f"{n}/trans64"])
    e_ref = float(fx[f"{n}/e_ref"])
    pts_d, trans_d = pts.to(DEV), trans64.float().contiguous().to(DEV)
    for prefix in ("feat.stn.", "feat."):
        layers_d, layers64 = dev_layers(sd, prefix), R.trunk_layers(sd, prefix)
        for relu_last in (0, 1):
            for with_trans in (False, True):
                got = W.pointnet_trunk(pts_d, trans_d if with_trans else None, *layers_d, relu_last)
                assert got.shape == (2, 1024) and got.dtype == torch.float32
                ref64 = R.trunk(pts.double(), trans64 if with_trans else None, layers64, relu_last)
                if (prefix, relu_last, with_trans) == ("feat.stn.", 1, False):
                    ref64 = torch.from_numpy(fx[f"{n}/stn64"])
                if (prefix, relu_last, with_trans) == ("feat.", 0, True):
                    ref64 = torch.from_numpy(fx[f"{n}/ref64"][:, :1024].copy())
                check(f"n={n} {prefix} relu_last={relu_last} trans={'given' if with_trans else 'NULL'}", got, ref64, e_ref)


# ---- 2. the whole module ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.CASES)
def test_whole_pointnet1_parity(fx, nets, n, monkeypatch):
    from gans.metrics import pointnet as M
    monkeypatch.setattr(M, "POINTNET_NATIVE", True)
    x = R.case_points(n).transpose(1, 2).to(DEV)
    assert M.uses_native(x.transpose(1, 2))
    got = nets[0](x)
    assert got.shape == (2, 1808)
    check(f"PointNet1 n={n}", got, torch.from_numpy(fx[f"{n}/ref64"]), float(fx[f"{n}/e_ref"]))


@pytest.mark.parametrize("tag,B,n", [("a", 3, 500), ("b", 2, 2048)])
def test_validation_fixture_through_the_kernel(nets, tag, B, n, monkeypatch):
    import recipe
    from gans.metrics import pointnet as M
    monkeypatch.setattr(M, "POINTNET_NATIVE", True)
    want = np.load(f"{GOLDEN}/validation.npz")[f"feats_{tag}"]
    got = nets[0](recipe.point_clouds(11 + n, B, n).to(DEV).transpose(1, 2)).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"validation.npz feats_{tag}: err {err:.3e}  limit {2e-4 * np.abs(want).max():.3e}")
    assert err <= 2e-4 * np.abs(want).max()


# ---- 3. the kernel's own edges --------------------------------------------------------------------------------------------
def test_tile_and_span_edges(sd, nets, W, monkeypatch):
    from gans.metrics import pointnet as M
    monkeypatch.setattr(M, "POINTNET_NATIVE", True)
    P, S = W.P, W.S
    assert P >= 2 and S >= P
    for n in sorted({P - 1, P, P + 1, S, S + 1, 3 * S + 1}):
        pts = edge_points(700 + n, 3, n)
        ref64 = R.pointnet1(sd, pts)
        e_ref = float((nets[1](pts.transpose(1, 2)).double() - ref64).abs().max())
        check(f"edge n={n}", nets[0](pts.to(DEV).transpose(1, 2)), ref64, e_ref)


# ---- 4. same bits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 385, 2048])
def test_same_bits(fx, sd, W, n):
    pts = edge_points(900 + n, 3, n).to(DEV)
    g = torch.Generator().manual_seed(n)
    trans = (torch.eye(3) + 0.2 * torch.randn(3, 3, 3, generator=g)).to(DEV)
    perm = torch.randperm(n, generator=g).to(DEV)
    for prefix, relu_last, tr in (("feat.stn.", 1, None), ("feat.", 0, trans)):
        layers = dev_layers(sd, prefix)
        whole = W.pointnet_trunk(pts, tr, *layers, relu_last)
        again = W.pointnet_trunk(pts, tr, *layers, relu_last)
        assert torch.equal(whole, again), "two consecutive calls"
        alone = W.pointnet_trunk(pts[2:3].contiguous(), None if tr is None else tr[2:3].contiguous(), *layers, relu_last)
        assert torch.equal(whole[2], alone[0]), "alone and as row 2 of a batch of 3"
        shuffled = W.pointnet_trunk(pts[:, perm].contiguous(), tr, *layers, relu_last)
        assert torch.equal(whole, shuffled), "a permutation of the points"
        longer = W.pointnet_trunk(torch.cat([pts, pts[:, :17]], dim=1).contiguous(), tr, *layers, relu_last)
        assert torch.equal(whole, longer), "17 of its own points appended"
        assert torch.isfinite(whole).all()


# ---- 5. ragged maximum of negative values ---------------------------------------------------------------------------------
def test_ragged_max_with_negative_values(fx, sd, W):
    """relu_last = 0 and b3 shifted by -50: every true h3 is far below zero, so the image of anything that is not a point
    of the cloud -- a zero row, the origin -- would win the maximum."""
    for n in (1, W.P + 1):
        pts = R.case_points(n) if n == 1 else edge_points(40 + n, 2, n)
        trans64 = torch.from_numpy(fx["1/trans64"])
        got = W.pointnet_trunk(pts.to(DEV), trans64.float().to(DEV), *dev_layers(sd, "feat.", -50.0), 0)
        ref64 = R.trunk(pts.double(), trans64, ref_layers(sd, "feat.", torch.float64, -50.0), 0)
        ref32 = R.trunk(pts, trans64.float(), ref_layers(sd, "feat.", torch.float32, -50.0), 0)
        assert float(ref64.max()) < -1.0
        check(f"negative n={n}", got, ref64, float((ref32.double() - ref64).abs().max()))
        print(f"negative n={n}: largest output {float(got.max()):.3f}")
        assert float(got.max()) <= -1.0


# ---- 6. memory and launches -------------------------------------------------------------------------------------------------
def test_memory_and_call_count(sd, nets, monkeypatch):
    import dgv2_native as N
    from gans.metrics import pointnet as M
    B, n = 4, 32768
    net = nets[0]
    x = edge_points(5, B, n).to(DEV).transpose(1, 2)
    calls = []
    real = N.lib.dgv2_pointnet_trunk
    monkeypatch.setattr(N.lib, "dgv2_pointnet_trunk", lambda *a: (calls.append(a[9:11]), real(*a))[1])

    monkeypatch.setattr(M, "POINTNET_NATIVE", True)
    net(x[:1, :, :64])                                     # nothing of the first call (the LDS attribute) is measured
    torch.cuda.synchronize()
    del calls[:]
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    native = net(x)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print(f"native PointNet1.forward at B={B}, N={n}: max_memory_allocated grew by {grew} bytes "
          f"(limit {B * n * 1024 * 4 // 64}); the [B,N,1024] activation is {B * n * 1024 * 4} bytes")
    assert grew < B * n * 1024 * 4 // 64
    assert calls == [(B, n), (B, n)], calls                # one call per trunk

    del calls[:]
    big = edge_points(6, 40, n).to(DEV).transpose(1, 2)    # three chunks of the library path's 2 GB budget
    assert 40 * n * 1024 * 4 > 2 * M.PointNet1.ACT_BYTES
    out = net(big)
    assert out.shape == (40, 1808) and calls == [(40, n), (40, n)], calls
    del big, out

    # the library path on the same device, and float64 on the same device as the judge of both
    monkeypatch.setattr(M, "POINTNET_NATIVE", False)
    del calls[:]
    library = net(x)
    assert calls == []
    pts64 = x.transpose(1, 2).double()
    sd64 = {k: v.to(DEV) for k, v in sd.items()}
    ref64 = torch.cat([R.pointnet1(sd64, pts64[i:i + 1]) for i in range(B)])   # a cloud at a time: 268 MB
    e_ref = float((library.double() - ref64).abs().max())
    check("B=4 N=32768 native vs float64", native, ref64.cpu(), e_ref)
    top = float(ref64.abs().max())
    diff = float((native - library).abs().max())
    print(f"native vs library on the device: {diff:.3e}  (twice the bound: {2 * R.bound(e_ref, top):.3e})")
    assert diff <= 2 * R.bound(e_ref, top)


# ---- 7. bad arguments -------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_feat_untouched(sd):
    import dgv2_native as N
    layers = dev_layers(sd, "feat.")
    flat = [t for pair in layers for t in pair]
    pts = R.case_points(65).to(DEV)
    feat = torch.full((2, 1024), 7.0, device=DEV)

    def rc(feat_=feat, B=2, n=65):
        return N.lib.dgv2_pointnet_trunk(N.ptr(feat_), N.ptr(pts), None, *[N.ptr(t) for t in flat], B, n, 0, N.stream())
    assert rc(feat_=None) == N.EINVAL
    assert rc(n=0) == N.EINVAL
    assert rc(B=0) == N.EINVAL
    assert rc(B=1 << 24, n=2 ** 31 - 1) == N.ENOTSUP       # above DGV2_POINTNET_MAX_TILES: refused before any launch
    torch.cuda.synchronize()
    assert bool((feat == 7.0).all())
    assert rc() == 0                                       # the same arguments, in range, are taken
    torch.cuda.synchronize()
    assert bool((feat != 7.0).all())
