"""CPU checks of the segmentation training objective (semseg/models/loss.py, gans/models/ops/native/segloss.py): the
closed form of tests/segloss_ref.py against the reference's own float64 results in tests/golden/segloss.npz
(tests/golden/make_segloss_golden.py) on every element, its rule for labels outside [0, C), the modules' buffers and
argument checks, and the exported C entry points.  No kernel runs here.

Pinning rule: per tensor, max |ref(float64) - fixture float64| <= 64 eps64 max |fixture| -- a few dozen roundings at
the tensor's scale; the two differ only in how 1 - p_y is formed (the closed form takes the other classes' share of
the softmax sum, the reference subtracts).  Measured on the fixture: at most 1.13 eps64 max|fixture| (loss map, c0),
2.91 (gradient, c2) and 0.74 (scalar, c1)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import segloss_ref as R
from conftest import GOLDEN

EPS64 = 2.0 ** -52
CASES = [(2, 3, 9, 37, 2.0, 1.0), (1, 4, 7, 130, 2.0, 4.0), (1, 20, 5, 33, 2.0, 8.0), (2, 32, 3, 5, 1.0, 4.0),
         (1, 4, 7, 40, 0.0, 4.0), (1, 4, 7, 40, 2.0, 30.0), (1, 1, 1, 9, 2.0, 1.0), (1, 3, 6, 50, 1.5, 4.0)]


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "segloss.npz"))
    return {k: d[k] for k in d.files}


def case_of(gold, name):
    c = {k: torch.from_numpy(np.asarray(gold[f"{name}.{k}"])) for k in
         ("logit", "label", "mask", "alpha", "loss_map32", "loss32", "grad32", "loss_map64", "loss64", "grad64")}
    c["gamma"] = float(gold[f"{name}.gamma_scale"][0])
    return c


def test_fixture_holds_the_eight_cases(gold):
    got = [tuple(int(v) for v in gold[f"{n}.config"]) + tuple(float(v) for v in gold[f"{n}.gamma_scale"]) for n in gold["cases"]]
    assert got == CASES
    assert not bool(np.isin(gold["c1.mask"], (0.0, 1.0)).all())          # the non-binary mask
    for n in gold["cases"]:
        assert gold[f"{n}.logit"].dtype == np.float32 and gold[f"{n}.label"].dtype == np.int64
        assert gold[f"{n}.loss_map32"].dtype == np.float32 and gold[f"{n}.grad64"].dtype == np.float64
        assert 0.7 < float(gold[f"{n}.mask"].astype(bool).mean()) <= 1.0
    # the saturated case: float32 p_y is exactly 1 somewhere and the loss is large somewhere else
    py = torch.softmax(torch.from_numpy(gold["c5.logit"]), 1).gather(1, torch.from_numpy(gold["c5.label"])[:, None])
    assert bool((py == 1).any()) and float(gold["c5.loss_map64"].max()) > 50
    assert np.array_equal(gold["c4.xent64"], gold["c4.loss_map64"]) and np.array_equal(gold["c4.xent32"], gold["c4.loss_map32"])
    assert float(np.abs(gold["c6.loss_map64"]).max()) == 0


@pytest.mark.parametrize("name", [f"c{i}" for i in range(len(CASES))])
def test_closed_form_equals_the_reference_in_float64(gold, name):
    c = case_of(gold, name)
    z, a = c["logit"].double(), c["alpha"].double()
    got = {"loss_map64": R.loss_map(z, c["label"], a, c["gamma"]),
           "loss64": R.masked_loss(z, c["label"], c["mask"], a, c["gamma"]),
           "grad64": R.masked_grad(z, c["label"], c["mask"], a, c["gamma"])}
    for key, v in got.items():
        want = c[key]
        assert v.dtype == torch.float64 and v.shape == want.shape
        err, top = float((v - want).abs().max()), float(want.abs().max())
        print(f"{name} {key}: max |ref - fixture| {err:.3e} = {err / (EPS64 * top) if top else 0:.2f} eps64 max|fixture|")
        assert err <= 64 * EPS64 * top, (name, key, err, top)
    assert torch.equal(R.pred(c["logit"]), c["logit"].argmax(dim=1))
    assert torch.equal(R.pred(c["logit"], c["mask"]), c["logit"].argmax(dim=1) * (c["mask"] != 0))


def test_closed_form_float32_is_as_good_as_the_reference(gold):
    """The float32 run of the closed form serves as the error estimate for shapes outside the fixture: on the fixture
    its error against float64 must be of the reference's own size (not above 4 E_ref + the floor of the GPU rule)."""
    for name in gold["cases"]:
        c = case_of(gold, name)
        for key32, key64, v in (("loss_map32", "loss_map64", R.loss_map(c["logit"], c["label"], c["alpha"], c["gamma"])),
                                ("grad32", "grad64", R.masked_grad(c["logit"], c["label"], c["mask"], c["alpha"], c["gamma"]))):
            assert v.dtype == torch.float32
            e_ref = float((c[key32].double() - c[key64]).abs().max())
            err = float((v.double() - c[key64]).abs().max())
            assert err <= 4 * e_ref + 2.0 ** -22 * float(c[key64].abs().max()), (name, key32, err, e_ref)


def test_labels_outside_the_range_and_ties():
    g = torch.Generator().manual_seed(7)
    z = torch.randn(1, 3, 4, 10, generator=g).double()
    label = torch.randint(0, 3, (1, 4, 10), generator=g)
    mask = torch.ones(1, 4, 10)
    stray = label.clone()
    stray[0, 1, ::3] = 3
    stray[0, 2, ::4] = -1
    off = (stray != label)
    L, Ls = R.loss_map(z, label, None, 2.0), R.loss_map(z, stray, None, 2.0)
    assert float(Ls[off].abs().max()) == 0 and torch.equal(Ls[~off], L[~off])
    gs = R.masked_grad(z, stray, mask, None, 2.0)
    assert float(gs.permute(0, 2, 3, 1)[off].abs().max()) == 0
    # the stray pixels' mask weights stay in the denominator
    assert float(R.masked_loss(z, stray, mask, None, 2.0)) == pytest.approx(float(Ls.sum()) / 40, rel=1e-14)
    # the gradient formula is autograd's, away from the fixture too (alpha = None, gamma = 0 and 3)
    for gamma in (0.0, 3.0):
        zz = z.clone().requires_grad_(True)
        R.masked_loss(zz, stray, mask, None, gamma).backward()
        assert float((zz.grad - R.masked_grad(z, stray, mask, None, gamma)).abs().max()) < 1e-15
    tie = torch.tensor([1.0, 2.0, 2.0, 2.0]).view(1, 4, 1, 1)
    assert R.pred(tie).item() == 1 and R.pred(tie, torch.zeros(1, 1, 1)).item() == 0


def test_modules_buffers_and_argument_checks():
    from gans.models.ops import native
    from semseg.models import FocalLoss, MaskedSegLoss
    alpha = torch.tensor([0.33, 1.0, 3.5])
    for mod in (FocalLoss(2.0, alpha=alpha), MaskedSegLoss(2.0, alpha=alpha)):
        assert list(mod.state_dict()) == ["alpha"] and not list(mod.parameters()) and mod.gamma == 2.0
        assert torch.equal(mod.alpha, alpha)
    for mod in (FocalLoss(2), MaskedSegLoss(0)):
        assert list(mod.state_dict()) == [] and mod.alpha is None
    assert FocalLoss(2).reduction == "none" and FocalLoss(2, reduction="mean").reduction == "mean"
    with pytest.raises(AssertionError):
        FocalLoss(2, reduction="sum")
    for gamma in (0.5, -1.0, float("nan"), 0.999):
        with pytest.raises(ValueError):
            FocalLoss(gamma)
        with pytest.raises(ValueError):
            MaskedSegLoss(gamma)
        with pytest.raises(ValueError):
            native.seg_masked_loss(torch.zeros(1, 3, 2, 4), torch.zeros(1, 2, 4, dtype=torch.int64), None, None, gamma)
    z, label, mask = torch.zeros(1, 3, 2, 4), torch.zeros(1, 2, 4, dtype=torch.int64), torch.ones(1, 2, 4)
    with pytest.raises(RuntimeError):       # CPU tensors: there is no CPU path
        FocalLoss(2.0)(z, label)
    with pytest.raises(RuntimeError):
        MaskedSegLoss(2.0, alpha=alpha)(z, label, mask)
    with pytest.raises(ValueError):         # C outside 1 .. 32
        native.seg_focal_loss_map(torch.zeros(1, 33, 2, 4), label, None, 2.0)
    with pytest.raises(ValueError):
        native.seg_masked_loss(torch.zeros(1, 0, 2, 4), label, mask, None, 2.0)
    with pytest.raises(ValueError):
        native.seg_masked_loss(z[0], label, mask, None, 2.0)
    with pytest.raises(ValueError):
        native.seg_masked_loss(z, label[:, :1], mask, None, 2.0)
    with pytest.raises(ValueError):
        native.seg_masked_loss(z, label, mask[:, :, :2], None, 2.0)
    with pytest.raises(ValueError):
        native.seg_masked_loss(z, label, mask, alpha[:2], 2.0)
    with pytest.raises(ValueError):
        native.seg_masked_loss(z, label, mask, None, 2.0, conf=torch.zeros(3, 3, dtype=torch.int64))
    assert native.SEG_LOSS_C_MAX == native.knn.CONFUSION_C_MAX == 32


def test_entry_points_are_exported_and_reject_on_the_host():
    import dgv2_native as N
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ("dgv2_seg_loss_scratch", "dgv2_seg_loss_forward", "dgv2_seg_loss_backward"):
        assert hasattr(lib, name) and name in N.SIGNATURES
    assert N.ABI_VERSION >= 55 and N.F16 == 3
    # the scratch query and the argument checks run on the host: no device is touched
    need = ctypes.c_int64(-1)
    assert N.lib.dgv2_seg_loss_scratch(ctypes.addressof(need), 2, 9, 37) == 0 and need.value >= 2 and need.value % 2 == 0
    small = need.value
    assert N.lib.dgv2_seg_loss_scratch(ctypes.addressof(need), 8, 64, 2048) == 0 and small <= need.value <= 1 << 16
    assert N.lib.dgv2_seg_loss_scratch(None, 2, 9, 37) == -1
    assert N.lib.dgv2_seg_loss_scratch(ctypes.addressof(need), 0, 9, 37) == -1
    assert N.lib.dgv2_seg_loss_scratch(ctypes.addressof(need), 1 << 20, 1 << 10, 1 << 10) == -1      # 2^40 pixels
    assert N.lib.dgv2_seg_loss_forward(None, None, None, None, None, 0, None, None, None, None, 1, 3, 2, 4, 2.0, 0, None) == -1
    assert N.lib.dgv2_seg_loss_backward(None, None, None, None, None, None, None, 1, 3, 2, 4, 2.0, 0, 0, None) == -1
