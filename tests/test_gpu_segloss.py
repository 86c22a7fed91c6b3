"""The segmentation training objective on the GPU (csrc/segloss.hip, gans/models/ops/native/segloss.py,
semseg/models/loss.py) against tests/golden/segloss.npz, which the reference wrote on CPU in float32 and in float64
(tests/golden/make_segloss_golden.py).

Comparison rule.  The yardstick is the reference itself: per tensor E_ref = max |ref32 - ref64| from the fixture, and
the GPU result must satisfy  max |gpu - ref64| <= 4 E_ref + 2^-22 max |ref64|  (the factor 4 covers another exp / log
and another summation order than the CPU's, the floor the cases where the reference happens to be exact).  It holds
for the per-pixel loss, the gradient of the masked scalar (through both backward modes) and the scalar itself.  Shapes
outside the fixture go against tests/segloss_ref.py in float64 under the same rule, E_ref coming from its float32 run
(test_segloss_cpu.py pins both to the fixture).  Predictions and confusion counts are integers: exact.

Measured on an MI355X (`ratio` = max |gpu - ref64| / E_ref, printed per case): on the fixture the largest ratio is
1.23 for the per-pixel loss (c7), 1.85 for the gradient (c7, the same through both backward modes) and 1.64 for the
scalar (c7); c6 (C = 1) is exactly 0 throughout.  Outside the fixture: 1.00 / 1.00 / 24.3 at (2,4,64,512), where the
float32 reference's scalar happens to be within 2.0e-8 of float64 (the GPU's is within 5.0e-7 of a loss of 7.13, 0.28
of its bound), and 1.16 / 1.07 / 0.02 at (2,5,11,70).  The largest error over bound anywhere is 0.34 (c7, gradient).
The file runs in under two seconds."""
import os

import numpy as np
import pytest
import torch

import segloss_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ["c0", "c1", "c2", "c3", "c4", "c5", "c6", "c7"]
FLOOR = 2.0 ** -22


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "segloss.npz"))
    return {k: d[k] for k in d.files}


def t(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


def within(tag, got, ref32, ref64):
    """The rule above for one tensor; prints the measured ratio before it asserts."""
    got, ref32, ref64 = (torch.as_tensor(v).detach().cpu().double() for v in (got, ref32, ref64))
    assert got.shape == ref64.shape, (tag, got.shape, ref64.shape)
    e_ref, top = float((ref32 - ref64).abs().max()), float(ref64.abs().max())
    err = float((got - ref64).abs().max())
    bound = 4 * e_ref + FLOOR * top
    print(f"{tag}: max |gpu - ref64| {err:.3e}, E_ref {e_ref:.3e}, ratio {err / e_ref if e_ref else float('nan'):.3f}, "
          f"bound {bound:.3e} (max |ref64| {top:.3e})")
    assert err <= bound, (tag, err, bound)


def run(logit, label, mask, alpha, gamma, conf=None):
    """-> loss, pred, grad of the masked scalar, loss_map, the same grad through the per-pixel backward."""
    from semseg.models import FocalLoss, MaskedSegLoss
    z = logit.detach().requires_grad_(True)          # no copy: the kernels see the caller's pointer and strides
    loss, pred = MaskedSegLoss(gamma, alpha=alpha)(z, label, mask, conf=conf)
    assert loss.dtype == torch.float32 and loss.ndim == 0 and pred.dtype == torch.int64 and not pred.requires_grad
    loss.backward()
    z2 = logit.detach().requires_grad_(True)
    loss_map = FocalLoss(gamma, alpha=alpha)(z2, label)
    assert loss_map.dtype == torch.float32 and tuple(loss_map.shape) == tuple(label.shape)
    m = mask.float()
    ((loss_map * m).sum() / m.sum()).backward()
    assert z.grad.dtype == logit.dtype and z2.grad.dtype == logit.dtype
    return loss.detach(), pred, z.grad, loss_map.detach(), z2.grad


@pytest.mark.parametrize("name", CASES)
def test_matches_the_reference(gold, name):
    g = {k: gold[f"{name}.{k}"] for k in ("logit", "label", "mask", "alpha", "loss_map32", "loss32", "grad32", "loss_map64",
                                          "loss64", "grad64")}
    gamma = float(gold[f"{name}.gamma_scale"][0])
    loss, pred, grad, loss_map, grad_px = run(t(g["logit"]), t(g["label"]), t(g["mask"]), t(g["alpha"]), gamma)
    within(f"{name} loss_map", loss_map, g["loss_map32"], g["loss_map64"])
    within(f"{name} grad", grad, g["grad32"], g["grad64"])
    within(f"{name} grad (per-pixel backward)", grad_px, g["grad32"], g["grad64"])
    within(f"{name} loss", loss, g["loss32"], g["loss64"])
    if gamma == 0:
        within(f"{name} loss_map vs F.cross_entropy", loss_map, gold[f"{name}.xent32"], gold[f"{name}.xent64"])
    want = torch.from_numpy(g["logit"]).argmax(dim=1) * (torch.from_numpy(g["mask"]) != 0)
    assert torch.equal(pred.cpu(), want)


def make_inputs(shape, seed, scale=3.0, stray=False):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    logit = scale * torch.randn(B, C, H, W, generator=g)
    label = torch.randint(0, C, (B, H, W), generator=g)
    if stray:   # labels outside [0, C) on both sides
        u = torch.rand(B, H, W, generator=g)
        label = torch.where(u < 0.04, torch.full_like(label, C), torch.where(u < 0.08, torch.full_like(label, -3), label))
    mask = (torch.rand(B, H, W, generator=g) < 0.8).float() * (0.5 + torch.rand(B, H, W, generator=g))
    alpha = 0.25 + 3.5 * torch.rand(C, generator=g)
    return logit, label, mask, alpha


@pytest.mark.parametrize("shape", [(2, 4, 64, 512), (2, 5, 11, 70)])
def test_shapes_outside_the_fixture(shape):
    logit, label, mask, alpha = make_inputs(shape, seed=sum(shape), stray=True)
    gamma = 2.0
    ref = {}
    for tag, z, a in (("32", logit, alpha), ("64", logit.double(), alpha.double())):
        ref["map" + tag] = R.loss_map(z, label, a, gamma)
        ref["loss" + tag] = R.masked_loss(z, label, mask, a, gamma)
        ref["grad" + tag] = R.masked_grad(z, label, mask, a, gamma)
    loss, pred, grad, loss_map, grad_px = run(logit.to(DEV), label.to(DEV), mask.to(DEV), alpha.to(DEV), gamma)
    within(f"{shape} loss_map", loss_map, ref["map32"], ref["map64"])
    within(f"{shape} grad", grad, ref["grad32"], ref["grad64"])
    within(f"{shape} grad (per-pixel backward)", grad_px, ref["grad32"], ref["grad64"])
    within(f"{shape} loss", loss, ref["loss32"], ref["loss64"])
    assert torch.equal(pred.cpu(), R.pred(logit, mask))
    # labels outside [0, C): no loss, no gradient
    off = (label < 0) | (label >= shape[1])
    assert int(off.sum()) > 0 and float(loss_map.cpu()[off].abs().max()) == 0
    assert float(grad.cpu().permute(0, 2, 3, 1)[off].abs().max()) == 0
    assert float(grad_px.cpu().permute(0, 2, 3, 1)[off].abs().max()) == 0


@pytest.fixture(scope="module")
def small():
    """(2,4,9,72): 648 pixels per sample, a multiple of 4 (vector path), more than one block; scale-1 logits."""
    logit, label, mask, alpha = make_inputs((2, 4, 9, 72), seed=21, scale=1.0, stray=True)
    return logit.to(DEV), label.to(DEV), mask.to(DEV), alpha.to(DEV)


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_bit_identical_run_to_run(small):
    logit, label, mask, alpha = small
    assert same_bits(run(logit, label, mask, alpha, 2.0), run(logit, label, mask, alpha, 2.0))
    big = [v.to(DEV) for v in make_inputs((2, 4, 64, 512), seed=5)]
    assert same_bits(run(*big, 2.0), run(*big, 2.0))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(2, 4, 9, 72), (1, 20, 5, 33)])
def test_half_logits_equal_their_float_cast(dtype, shape):
    logit, label, mask, alpha = (v.to(DEV) for v in make_inputs(shape, seed=31, scale=1.0))
    half = logit.to(dtype)
    loss_h, pred_h, grad_h, map_h, gpx_h = run(half, label, mask, alpha, 2.0)
    loss_f, pred_f, grad_f, map_f, gpx_f = run(half.float(), label, mask, alpha, 2.0)
    assert torch.equal(loss_h, loss_f) and torch.equal(map_h, map_f) and torch.equal(pred_h, pred_f)
    assert grad_h.dtype == dtype and torch.equal(grad_h, grad_f.to(dtype)) and torch.equal(gpx_h, gpx_f.to(dtype))
    assert float(grad_h.float().abs().max()) > 0


def test_ties_go_to_the_lowest_index():
    # bf16 logits of scale 1 have 8 bits of significand: among 20 classes the largest value is often attained twice
    logit, label, mask, alpha = make_inputs((2, 20, 16, 64), seed=41, scale=1.0)
    half = logit.bfloat16()
    top = half.float().max(dim=1, keepdim=True).values
    tied = (half.float() == top).sum(dim=1) > 1
    assert int(tied.sum()) >= 10
    from gans.models.ops import native
    for z in (half, half.float(), half.half()):
        _, pred = native.seg_masked_loss(z.to(DEV), label.to(DEV), None, None, 2.0)
        assert torch.equal(pred.cpu(), R.pred(half.float()))
    _, pred = native.seg_masked_loss(half.to(DEV), label.to(DEV), mask.to(DEV), None, 2.0)
    assert torch.equal(pred.cpu(), R.pred(half.float(), mask))


def test_unaligned_and_non_contiguous_inputs(small):
    logit, label, mask, alpha = small
    want = run(logit, label, mask, alpha, 2.0)
    # the same values one element into a buffer: the pointers are only 4-byte (logits, mask) / 8-byte (labels) aligned
    def shifted(v):
        buf = torch.zeros(v.numel() + 1, device=DEV, dtype=v.dtype)
        buf[1:] = v.flatten()
        out = buf[1:].view(v.shape)
        assert out.data_ptr() % 16 != 0 and out.is_contiguous()
        return out
    assert same_bits(run(shifted(logit), label, mask, alpha, 2.0), want)
    assert same_bits(run(shifted(logit), shifted(label), shifted(mask), alpha, 2.0), want)
    # channels-last storage, a W-slice of a wider tensor, int32 labels, a bool-like mask dtype
    assert same_bits(run(logit.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), label, mask, alpha, 2.0), want)
    wide = torch.zeros(2, 4, 9, 80, device=DEV)
    wide[..., :72] = logit
    assert same_bits(run(wide[..., :72], label.int(), mask.double(), alpha, 2.0), want)
    # a pixel count that is no multiple of 4 takes the element-wise path throughout: against the reference rule
    odd = [v.to(DEV) for v in make_inputs((2, 3, 7, 37), seed=43)]
    a, b = run(*odd, 2.0), run(shifted(odd[0]), *odd[1:], 2.0)
    assert same_bits(a, b)


def test_alpha_none_equals_ones(small):
    logit, label, mask, _ = small
    for gamma in (0.0, 2.0):
        assert same_bits(run(logit, label, mask, None, gamma), run(logit, label, mask, torch.ones(4, device=DEV), gamma))


@pytest.mark.parametrize("shape", [(2, 4, 9, 72), (2, 20, 5, 33), (2, 4, 64, 512)])
def test_fused_counts_equal_seg_confusion(shape):
    from gans.models.ops import native
    C = shape[1]
    logit, label, mask, alpha = (v.to(DEV) for v in make_inputs(shape, seed=51, stray=True))
    conf = torch.zeros(C + 1, C + 1, device=DEV, dtype=torch.int64)
    loss, pred = native.seg_masked_loss(logit, label, mask, alpha, 2.0, conf=conf)
    want = native.seg_confusion(label, logit.argmax(1), C, mask=mask)
    assert torch.equal(conf, want) and int(conf.sum()) == label.numel() and int(conf[C].sum()) > 0
    assert torch.equal(pred, logit.argmax(1) * (mask != 0))
    # the second call adds; without conf the loss is the same bits
    loss2, _ = native.seg_masked_loss(logit, label, mask, alpha, 2.0, conf=conf, want_pred=False)
    assert torch.equal(conf, 2 * want) and torch.equal(loss, loss2)
    assert torch.equal(loss, native.seg_masked_loss(logit, label, mask, alpha, 2.0)[0])
    # no mask: every pixel counts with its own label
    conf_all = torch.zeros_like(conf)
    native.seg_masked_loss(logit, label, None, alpha, 2.0, conf=conf_all)
    assert torch.equal(conf_all, native.seg_confusion(label, logit.argmax(1), C))


def test_module_api(small):
    from semseg.models import FocalLoss, MaskedSegLoss
    logit, label, mask, alpha = small
    assert torch.equal(FocalLoss(2.0, alpha=alpha, reduction="mean")(logit, label), FocalLoss(2.0, alpha=alpha)(logit, label).mean())
    crit = MaskedSegLoss(2.0, alpha=alpha)
    loss, pred = crit(logit, label, torch.zeros_like(mask))
    assert bool(torch.isnan(loss)) and int(pred.abs().max()) == 0
    # the upstream scalar is read on the device: half the loss, exactly half the gradient
    z1, z2 = (logit.clone().requires_grad_(True) for _ in range(2))
    crit(z1, label, mask)[0].backward()
    (crit(z2, label, mask)[0] * 0.5).backward()
    assert float(z1.grad.abs().max()) > 0 and torch.equal(z2.grad, z1.grad * 0.5)
    # first order only
    for first in (lambda z: crit(z, label, mask)[0], lambda z: FocalLoss(2.0)(z, label).sum()):
        z = logit.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(first(z), z, create_graph=True)
        with pytest.raises(RuntimeError):
            g.sum().backward()


def test_step_is_capturable():
    """Forward + backward with conf in one graph on one stream: nothing reads a value on the host."""
    from semseg.models import MaskedSegLoss
    shape = (2, 4, 9, 70)
    crit = MaskedSegLoss(2.0, alpha=torch.tensor([0.33, 1.0, 3.5, 2.0])).to(DEV)
    batches = [[v.to(DEV) for v in make_inputs(shape, seed=s, stray=True)[:3]] for s in (61, 62, 63)]

    def eager(logit, label, mask):
        z = logit.clone().requires_grad_(True)
        conf = torch.zeros(5, 5, device=DEV, dtype=torch.int64)
        loss, pred = crit(z, label, mask, conf=conf)
        loss.backward()
        return loss.detach().clone(), pred.clone(), z.grad.clone(), conf
    want = [eager(*b) for b in batches]

    z = batches[0][0].clone().requires_grad_(True)
    label, mask = batches[0][1].clone(), batches[0][2].clone()
    conf = torch.zeros(5, 5, device=DEV, dtype=torch.int64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm-up
        crit(z, label, mask, conf=conf)[0].backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    z.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, pred = crit(z, label, mask, conf=conf)
        loss.backward()
    grad = z.grad
    for (zb, lb, mb), w in zip(batches[1:], want[1:]):
        with torch.no_grad():
            z.copy_(zb)
            label.copy_(lb)
            mask.copy_(mb)
            conf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits((loss.detach(), pred, grad, conf), w)


def test_unsupported_arguments_are_rejected(small):
    import ctypes
    import dgv2_native as N
    from gans.models.ops import native
    logit, label, mask, alpha = small
    B, C, H, W = logit.shape
    for gamma in (0.5, -2.0, float("nan")):
        with pytest.raises(ValueError):
            native.seg_masked_loss(logit, label, mask, alpha, gamma)
        with pytest.raises(ValueError):
            native.seg_focal_loss_map(logit, label, alpha, gamma)
    with pytest.raises(ValueError):
        native.seg_masked_loss(torch.zeros(1, 33, 2, 4, device=DEV), label[:1, :2, :4], None, None, 2.0)
    with pytest.raises(ValueError):
        native.seg_masked_loss(logit, label, mask, alpha, 2.0, conf=torch.zeros(C, C, device=DEV, dtype=torch.int64))
    with pytest.raises(ValueError):
        native.seg_masked_loss(logit, label, mask, alpha, 2.0, conf=torch.zeros(C + 1, C + 1, device=DEV, dtype=torch.int32))

    # the C entry points themselves: DGV2_EINVAL, nothing launched
    need = ctypes.c_int64(0)
    assert N.lib.dgv2_seg_loss_scratch(ctypes.addressof(need), B, H, W) == 0
    loss_map = torch.full((B, H, W), -7.0, device=DEV)
    pred = torch.full((B, H, W), -7, device=DEV, dtype=torch.int64)
    conf = torch.full((C + 1, C + 1), -7, device=DEV, dtype=torch.int64)
    sums = torch.full((3,), -7.0, device=DEV)
    scratch = torch.full((need.value,), -7.0, device=DEV)
    g_logit = torch.full_like(logit, -7.0)
    gout = torch.ones((), device=DEV)

    def fwd(lm=N.ptr(loss_map), p=N.ptr(pred), cf=N.ptr(conf), s=N.ptr(sums), sc=N.ptr(scratch), n=need.value, z=N.ptr(logit),
            y=N.ptr(label), dims=(B, C, H, W), gamma=2.0, dtype=0):
        return N.lib.dgv2_seg_loss_forward(lm, p, cf, s, sc, n, z, y, N.ptr(mask), N.ptr(alpha), *dims, gamma, dtype, N.stream())

    def bwd(g=N.ptr(g_logit), z=N.ptr(logit), y=N.ptr(label), go=N.ptr(gout), s=N.ptr(sums), dims=(B, C, H, W), gamma=2.0, dtype=0,
            per_pixel=0):
        return N.lib.dgv2_seg_loss_backward(g, z, y, N.ptr(mask), N.ptr(alpha), go, s, *dims, gamma, dtype, per_pixel, N.stream())
    bad_dims = ((0, C, H, W), (B, 0, H, W), (B, 33, H, W), (B, C, 0, W), (B, C, H, 0), (-1, C, H, W), (1 << 20, C, 1 << 10, 1 << 10))
    assert fwd(z=None) == -1 and fwd(y=None) == -1 and fwd(lm=None, p=None, cf=None, s=None) == -1
    assert fwd(sc=None) == -1 and fwd(n=need.value - 1) == -1
    assert all(fwd(dims=d) == -1 for d in bad_dims)
    assert all(fwd(gamma=v) == -1 for v in (0.5, -1.0, float("nan"))) and fwd(dtype=2) == -1 and fwd(dtype=4) == -1 and fwd(dtype=-1) == -1
    assert bwd(g=None) == -1 and bwd(z=None) == -1 and bwd(y=None) == -1 and bwd(go=None) == -1 and bwd(s=None) == -1
    assert all(bwd(dims=d) == -1 for d in bad_dims)
    assert all(bwd(gamma=v) == -1 for v in (0.5, -1.0, float("nan"))) and bwd(dtype=2) == -1 and bwd(per_pixel=2) == -1
    torch.cuda.synchronize()
    for canary in (loss_map, pred, conf, sums, scratch, g_logit):
        assert int((canary != -7).sum()) == 0
    # and the same calls with good arguments run
    conf.zero_()
    assert fwd() == 0 and bwd() == 0 and fwd(lm=None, p=None, cf=None) == 0 and fwd(s=None, sc=None, n=0) == 0
    torch.cuda.synchronize()
    assert int(conf.sum()) == 2 * B * H * W and float(sums[2]) == pytest.approx(float(mask.sum()), rel=1e-6)
    assert bool(torch.isfinite(g_logit).all()) and int((pred == -7).sum()) == 0
