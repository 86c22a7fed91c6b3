"""GPU checks of the segmentation evaluation driver: the whole SqueezeSegV2 eval() forward with the
context-aggregation modules native against composed, semseg.evaluation.evaluate_checkpoint against the reference's
masked-sum counts (test_semseg.py:23-42) in plain torch, and the command line test_semseg.py in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import squeezeseg_ref as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (8, 64)
MODEL_CASE = 3    # squeezeseg_ref.MODEL_CASES[3]: V2, 2 x 5 x 3 x 48, no CRF


def _bound(e_ref, top):
    return 4.0 * e_ref + 2.0 ** -22 * top


def test_whole_model_native_cam_against_composed(monkeypatch):
    """Both routings sit within the float32 bound of the reference's float64 logits, and so does their difference."""
    from gans.models.ops.native import cam as M
    from semseg.models import SqueezeSegV2, common
    assert R.MODEL_CASES[MODEL_CASE] == (2, 2, 3, 48, False)
    d = np.load(os.path.join(GOLDEN, "squeezeseg.npz"))
    name = R.model_case_name(MODEL_CASE)
    model = SqueezeSegV2(R.MODEL_INPUTS, R.MODEL_CLASSES, use_crf=False, pretrained_weights=False)
    model.load_state_dict(R.hash_fill_state_dict(model.state_dict(), salt="v2/"), strict=True)
    model = model.eval().to(DEV)
    img = torch.from_numpy(d[name + "/img"]).to(DEV)
    assert tuple(img.shape) == (2, 5, 3, 48)
    calls = []
    orig = M.cam_forward
    monkeypatch.setattr(M, "cam_forward", lambda *a, **k: calls.append(1) or orig(*a, **k))
    monkeypatch.setattr(common, "CAM_NATIVE", True)
    with torch.no_grad():
        on = model(img).cpu().double()
    assert len(calls) == 3
    monkeypatch.setattr(common, "CAM_NATIVE", False)
    with torch.no_grad():
        off = model(img).cpu().double()
    assert len(calls) == 3
    ref64, ref32 = torch.from_numpy(d[name + "/logit64"]), torch.from_numpy(d[name + "/logit32"])
    e_ref, top = float((ref32.double() - ref64).abs().max()), float(ref64.abs().max())
    err_on, err_off, diff = (float(t.abs().max()) for t in (on - ref64, off - ref64, on - off))
    print(f"MODEL cam on/off: err on {err_on:.3e}  off {err_off:.3e}  on-off {diff:.3e}  E_ref {e_ref:.3e}  "
          f"bound {_bound(e_ref, top):.3e}")
    assert err_on <= _bound(e_ref, top) and err_off <= _bound(e_ref, top)
    assert diff <= _bound(e_ref, top)


# ---- evaluate_checkpoint ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt_path(tmp_path_factory):
    """A randomly initialised V2 checkpoint (with the CRF, the default configuration) as Trainer.state_dict() writes it."""
    from semseg.config import default_config
    from semseg.trainer import Trainer
    cfg = default_config()
    cfg.dataset.shape = list(SHAPE)
    torch.manual_seed(11)
    trainer = Trainer(cfg, DEV, pretrained_weights=False)
    with torch.no_grad():      # spread the classifier so that the predictions are not one class
        trainer.model.decoder.head[1].weight.mul_(4.0)
    path = tmp_path_factory.mktemp("semseg_eval") / "checkpoint.pth"
    torch.save(trainer.state_dict(), path)
    return str(path)


def _loader():
    from semseg.datasets import SyntheticFrontal
    return torch.utils.data.DataLoader(SyntheticFrontal(length=4, shape=SHAPE), batch_size=2)


def _reference_counts(loader, preds, num_classes):
    """test_semseg.py:23-42 and 136-142 on the returned (already masked) predictions: masked sums, summed over batches."""
    tps, fps, fns = (torch.zeros(num_classes, dtype=torch.int64) for _ in range(3))
    for item, pred in zip(loader, preds):
        label = (item["label"].long() * item["mask"].long())
        pred = pred.cpu()
        assert pred.dtype == torch.int64 and pred.shape == label.shape
        assert bool((pred[item["mask"] == 0] == 0).all())
        for c in range(num_classes):
            tps[c] += (pred[label == c] == c).sum()
            fps[c] += (label[pred == c] != c).sum()
            fns[c] += (pred[label == c] != c).sum()
    return tps.numpy(), fps.numpy(), fns.numpy()


_SUMMARIES = {}


def _summary(ckpt_path, with_knn):
    if with_knn not in _SUMMARIES:
        from semseg.evaluation import evaluate_checkpoint
        from semseg.models import kNN2d
        knn = kNN2d(num_classes=4, k=5, kernel_size=5).to(DEV) if with_knn else None
        _SUMMARIES[with_knn] = evaluate_checkpoint(ckpt_path, _loader(), DEV, knn=knn, return_preds=True)
    return _SUMMARIES[with_knn]


@pytest.mark.parametrize("with_knn", [False, True], ids=["plain", "knn"])
def test_evaluate_checkpoint_counts_are_the_reference_sums(ckpt_path, with_knn):
    summary, preds = _summary(ckpt_path, with_knn)
    assert len(preds) == 2 and all(p.is_cuda for p in preds)
    tp, fp, fn = _reference_counts(_loader(), preds, 4)
    for key, want in (("tp", tp), ("fp", fp), ("fn", fn)):
        assert summary[key].dtype == np.int64 and np.array_equal(summary[key], want), (key, summary[key], want)
    pixels = 4 * SHAPE[0] * SHAPE[1]
    assert int((tp + fn).sum()) == pixels and int((tp + fp).sum()) == pixels
    assert not bool(np.any(np.concatenate([p.cpu().numpy().ravel() for p in preds]) == 3))     # the cyclist class is omitted
    seen = sorted({int(v) for p in preds for v in p.unique()})
    print(f"EVAL knn={with_knn}: classes predicted {seen}  tp {tp.tolist()}  fp {fp.tolist()}  fn {fn.tolist()}")
    if not with_knn:   # the filter may vote every pixel of these hashed scans to class 0; the bare predictions may not be one class
        assert len(seen) >= 2
    eps = 1e-12
    assert np.array_equal(summary["iou"], tp / (tp + fn + fp + eps))
    assert summary["mean_iou"] == float((tp / (tp + fn + fp + eps))[1:3].mean())
    assert summary["mean_precision"] == float((tp / (tp + fp + eps))[1:3].mean())
    assert summary["mean_recall"] == float((tp / (tp + fn + eps))[1:3].mean())
    assert summary["classes"] == 4


def test_evaluate_checkpoint_takes_a_loaded_checkpoint_and_repeats(ckpt_path):
    from semseg.evaluation import evaluate_checkpoint
    from semseg.pretrained import load_checkpoint
    summary, _ = _summary(ckpt_path, False)
    again = evaluate_checkpoint(load_checkpoint(ckpt_path), _loader(), DEV)
    assert isinstance(again, dict)
    for key in ("tp", "fp", "fn"):
        assert np.array_equal(again[key], summary[key])


def test_cli_in_a_child_process(ckpt_path):
    """One run of test_semseg.py in a fresh process; its last line is strict JSON with evaluate_checkpoint's numbers."""
    summary, _ = _summary(ckpt_path, False)
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "test_semseg.py"), "--ckpt_path", ckpt_path,
           "--synthetic", "4", "--shape", str(SHAPE[0]), str(SHAPE[1]), "--batch_size", "2"]
    run = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.strip().splitlines()

    def refuse(token):
        raise ValueError(f"not strict JSON: {token}")
    rec = json.loads(lines[-1], parse_constant=refuse)
    table = lines[-7:-1]
    assert table[0].split() == ["class", "iou", "precision", "recall"] and table[-1].split()[0] == "mean"
    assert [row.split()[0] for row in table[1:5]] == rec["classes"] == ["unknown", "car", "pedestrian", "cyclist"]
    assert table[-1].split()[1] == f"{summary['mean_iou']:.1%}"
    for key in ("tp", "fp", "fn"):
        assert rec[key] == [int(v) for v in summary[key]]
    for key in ("iou", "precision", "recall"):
        assert rec[key] == [float(v) for v in summary[key]]
        assert rec["mean_" + key] == summary["mean_" + key]
    assert rec["scans"] == 4 and rec["knn"] is False
