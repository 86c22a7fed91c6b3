"""Scoring of range-image segmentation (reference: test_semseg.py:23-42 and 117-159): per-class tp / fp / fn, IoU,
precision and recall, all derived from one integer confusion matrix that a native kernel accumulates
(gans.models.ops.native.seg_confusion, csrc/segcount.hip).

The matrix is int64 [C+1, C+1]: row = label, column = prediction, the last row / column = "outside [0, C)".
    tp_c = conf[c, c]      fp_c = sum_r conf[r, c] - tp_c      fn_c = sum_r conf[c, r] - tp_c     (r over all C+1)
which is what the reference's masked sums count: its fp includes pixels whose label is out of range, its fn those
whose prediction is.  A mask is applied as the reference does (preds * mask, label * mask): where mask == 0 both count
as class 0; any other mask value counts as 1 (the datasets' masks are binary).
"""
import torch

from gans.models.ops.native.knn import seg_confusion


def confusion(label, pred, num_classes, mask=None, out=None):
    """-> int64 [C+1, C+1] with the counts of (label, pred) ADDED to `out` (zeros when None).  GPU tensors only."""
    return seg_confusion(label, pred, num_classes, mask=mask, out=out)


def counts_from_confusion(conf):
    """conf int64 [C+1, C+1] (any device) -> (tps, fps, fns), int64 [C] each: index arithmetic only."""
    tps = conf.diagonal()[:-1]
    return tps, conf.sum(0)[:-1] - tps, conf.sum(1)[:-1] - tps


def evaluate(label, pred, num_classes, epsilon=1e-12):
    """The reference's evaluate: -> (ious, tps, fps, fns), float32 [num_classes] each, iou = tp / (tp + fn + fp +
    epsilon).  One kernel launch for the counts; the division runs in float64 on the exact integers."""
    tps, fps, fns = counts_from_confusion(confusion(label, pred, num_classes))
    ious = tps.double() / ((tps + fns + fps).double() + epsilon)
    return ious.float(), tps.float(), fps.float(), fns.float()


class Evaluator:
    """Accumulates an evaluation as the reference's loop does (test_semseg.py:128-142) and reports what it prints
    (144-159).  knn: a semseg.models.kNN2d or None; remap: {class: class} applied to the predictions in order (the
    reference omits the cyclist class with {3: 0}).  update() never synchronises with the host."""

    def __init__(self, num_classes, knn=None, remap=None):
        self.num_classes = int(num_classes)
        self.knn = knn
        self.remap = dict(remap or {})
        self.conf = None

    @torch.no_grad()
    def update(self, logit_or_pred, label, mask, depth=None):
        """logit_or_pred: logits [B,C,H,W] (argmax over C is taken) or predictions [B,H,W]; label, mask [B,H,W];
        depth [B,1,H,W], needed when a kNN filter was given."""
        pred = logit_or_pred.argmax(dim=1) if logit_or_pred.ndim == 4 else logit_or_pred
        for src, dst in self.remap.items():
            pred = torch.where(pred == src, dst, pred)
        if self.knn is not None:
            if depth is None:
                raise ValueError("Evaluator.update: the kNN filter needs depth")
            pred = self.knn(depth, pred)
        if self.conf is None:
            self.conf = torch.zeros((self.num_classes + 1, self.num_classes + 1), device=label.device, dtype=torch.int64)
        if mask is not None:
            mask = mask.reshape(label.shape)
        confusion(label, pred, self.num_classes, mask=mask, out=self.conf)

    def summary(self, mean_classes=slice(1, 3), epsilon=1e-12):
        """-> {"iou", "precision", "recall": float64 numpy [num_classes]; "mean_iou", "mean_precision", "mean_recall":
        their means over `mean_classes` (the reference omits 'unknown' and 'cyclist': [1:3]); "tp", "fp", "fn": int64
        numpy}.  Reads the counts back: this is where the host synchronises."""
        if self.conf is None:
            raise RuntimeError("Evaluator.summary: nothing was accumulated")
        tp, fp, fn = (t.cpu().numpy() for t in counts_from_confusion(self.conf))
        out = {"iou": tp / (tp + fn + fp + epsilon), "precision": tp / (tp + fp + epsilon),
               "recall": tp / (tp + fn + epsilon), "tp": tp, "fp": fp, "fn": fn}
        for key in ("iou", "precision", "recall"):
            out["mean_" + key] = float(out[key][mean_classes].mean())
        return out


__all__ = ["confusion", "counts_from_confusion", "evaluate", "Evaluator"]
