"""CPU checks of the kNN label filter and the scoring (semseg/models/knn.py, semseg/metrics.py): the restatement
tests/knn_ref.py against the reference's own labels in tests/golden/knn2d.npz (tests/golden/make_knn_golden.py), the
module's buffer, attributes and argument checks, and evaluate's index arithmetic on a confusion matrix against the
reference's tp / fp / fn.  No kernel runs here.

A pixel is FRAGILE when its float64 decision margin (knn_ref's docstring) is below 1e-6 S + 4 D, S being the case's
largest finite float64 distance and D the largest float32-vs-float64 deviation of the restatement's distances: there
the float32 reference and a float64 evaluation may pick different neighbours.  At most 1 % of a case's pixels may be
fragile, or the fixture is useless and the test fails.  Measured on the fixture: one fragile pixel in c1 (0.36 %) and
one in c6 (0.02 %), none elsewhere, and no float32 / float64 disagreement at all; D / S is 2e-8 .. 3e-7."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from knn_ref import fragile_threshold, knn_ref

FRAGILE_CAP = 0.01


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "knn2d.npz"))
    return {k: d[k] for k in d.files}


def case_of(gold, name):
    B, H, W, C, k, kh, kw = (int(v) for v in gold[f"{name}.config"])
    sigma, cutoff = (float(v) for v in gold[f"{name}.sigma_cutoff"])
    return dict(B=B, H=H, W=W, C=C, k=k, ks=(kh, kw), sigma=sigma, cutoff=cutoff,
                depth=torch.from_numpy(gold[f"{name}.depth"]), label=torch.from_numpy(gold[f"{name}.label"]),
                dist_kernel=torch.from_numpy(gold[f"{name}.dist_kernel"]), refined=torch.from_numpy(gold[f"{name}.refined"]))


def both_precisions(c):
    """-> (labels32, labels64, fragile [B,H,W] bool) of knn_ref on the CPU."""
    l32, d32, _ = knn_ref(c["depth"], c["label"], c["dist_kernel"], c["k"], c["C"], c["cutoff"])
    l64, d64, m64 = knn_ref(c["depth"].double(), c["label"], c["dist_kernel"].double(), c["k"], c["C"], c["cutoff"])
    thr, S, D = fragile_threshold(d64, d32)
    return l32, l64, m64 < thr, (thr, S, D)


def test_fixture_holds_the_seven_cases(gold):
    got = [tuple(int(v) for v in gold[f"{n}.config"]) + tuple(float(v) for v in gold[f"{n}.sigma_cutoff"]) for n in gold["cases"]]
    assert got == [(2, 9, 37, 4, 3, 3, 3, 1.0, 1.0), (1, 7, 40, 20, 5, 5, 5, 1.0, 1.0), (1, 7, 40, 20, 5, 5, 5, 1.0, 0.0),
                   (1, 5, 33, 3, 7, 3, 5, 0.7, 2.0), (1, 1, 9, 2, 1, 3, 3, 1.0, 1.0), (1, 3, 5, 3, 9, 3, 3, 1.0, 1.0),
                   (1, 33, 130, 4, 5, 5, 5, 1.0, 1.0)]
    assert float(gold["c2.depth"].min()) >= 0 and float(gold["c6.depth"].min()) < 0


def test_float32_restatement_equals_the_reference_everywhere(gold):
    bad = []
    for name in gold["cases"]:
        c = case_of(gold, name)
        labels, _, _ = knn_ref(c["depth"], c["label"], c["dist_kernel"], c["k"], c["C"], c["cutoff"])
        assert labels.dtype == torch.int64 and labels.shape == c["refined"].shape
        n = int((labels != c["refined"]).sum())
        print(f"{name}: {n} of {labels.numel()} pixels differ from the reference")
        if n:
            bad.append((name, n))
    assert not bad, bad


def test_float64_restatement_equals_the_reference_outside_fragile_pixels(gold):
    bad = []
    for name in gold["cases"]:
        c = case_of(gold, name)
        l32, l64, fragile, (thr, S, D) = both_precisions(c)
        share = float(fragile.float().mean())
        inside, outside = int(((l64 != c["refined"]) & fragile).sum()), int(((l64 != c["refined"]) & ~fragile).sum())
        print(f"{name}: S {S:.3g}, D {D:.2e}, threshold {thr:.2e}; {int(fragile.sum())} fragile pixels ({share:.2%}), "
              f"{inside} mismatches inside them, {outside} outside")
        if share > FRAGILE_CAP or outside:
            bad.append((name, share, outside))
    assert not bad, bad


def test_module_buffer_and_attributes(gold):
    from semseg.models import kNN2d
    from semseg.models.knn import get_gaussian_kernel
    for name in gold["cases"]:
        c = case_of(gold, name)
        knn = kNN2d(c["C"], k=c["k"], kernel_size=c["ks"], sigma=c["sigma"], cutoff=c["cutoff"])
        assert list(knn.state_dict()) == ["dist_kernel"] and not list(knn.parameters())
        assert knn.dist_kernel.dtype == torch.float32 and tuple(knn.dist_kernel.shape) == (1, 1) + c["ks"]
        assert torch.equal(knn.dist_kernel, c["dist_kernel"]), name
        assert (knn.num_classes, knn.k, knn.kernel_size, knn.sigma, knn.cutoff) == (c["C"], c["k"], c["ks"], c["sigma"], c["cutoff"])
        assert knn.padding == (c["ks"][0] // 2, c["ks"][1] // 2)
    knn = kNN2d(4)
    assert (knn.k, knn.kernel_size, knn.padding, knn.sigma, knn.cutoff) == (3, (3, 3), (1, 1), 1.0, 1.0)
    g = get_gaussian_kernel((3, 5), 0.7)
    assert tuple(g.shape) == (3, 5) and abs(float(g.sum()) - 1) < 1e-6 and torch.equal(g, g.flip(0, 1))


def test_argument_checks():
    from semseg.models import kNN2d
    for kwargs in (dict(kernel_size=4), dict(kernel_size=(3, 2)), dict(kernel_size=7), dict(kernel_size=(3, 7)),
                   dict(kernel_size=1, k=1), dict(kernel_size=3, k=10), dict(kernel_size=(3, 5), k=16), dict(k=0)):
        with pytest.raises(ValueError):
            kNN2d(4, **kwargs)
    with pytest.raises(ValueError):
        kNN2d(0)
    knn = kNN2d(4)
    depth, label = torch.ones(1, 1, 4, 6), torch.zeros(1, 4, 6, dtype=torch.int64)
    with pytest.raises(RuntimeError):       # CPU tensors: there is no CPU path
        knn(depth, label)
    with pytest.raises(ValueError):
        knn(torch.ones(1, 2, 4, 6), label)
    with pytest.raises(ValueError):
        knn(depth[:, 0], label)
    with pytest.raises(ValueError):
        knn(depth, label[:, :, :-1])


def test_evaluate_from_confusion_equals_the_reference(gold):
    from semseg.metrics import counts_from_confusion
    for name in ("e0", "e1"):
        C = int(gold[f"{name}.num_classes"])
        label, pred, mask = (torch.from_numpy(gold[f"{name}.{k}"]) for k in ("label", "pred", "mask"))
        keep = mask != 0
        row = torch.where(keep, label, torch.zeros_like(label))
        col = torch.where(keep, pred, torch.zeros_like(pred))
        row = torch.where((row >= 0) & (row < C), row, torch.full_like(row, C))
        col = torch.where((col >= 0) & (col < C), col, torch.full_like(col, C))
        conf = torch.bincount((row * (C + 1) + col).flatten(), minlength=(C + 1) ** 2).reshape(C + 1, C + 1)
        tp, fp, fn = counts_from_confusion(conf)
        for key, got in (("tp", tp), ("fp", fp), ("fn", fn)):
            assert got.dtype == torch.int64 and got.tolist() == gold[f"{name}.{key}"].tolist(), (name, key)
    assert int((gold["e1.label"] >= 6).sum()) > 0 and int((gold["e1.pred"] < 0).sum()) > 0
