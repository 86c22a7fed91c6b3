"""Evaluation of a segmentation checkpoint on one GPU (reference: test_semseg.py:117-159): the model's eval() forward
under inference_mode and float16 autocast -- every Fire module, and every context-aggregation module with
semseg.models.common.CAM_NATIVE on, is one native launch -- scored by semseg.metrics.Evaluator with the reference's
{3: 0} remap (the cyclist class is omitted) and an optional kNN label filter.  The loop never reads anything back:
the only host synchronisation is the summary at the end.

Not here: DataParallel (the reference wraps the model in it), the rich table (the command line test_semseg.py prints
plain text)."""
import os

import torch

from .metrics import Evaluator
from .pretrained import build_from_checkpoint, load_checkpoint
from .trainer import make_inputs

OMIT_REMAP = {3: 0}   # test_semseg.py:130-131


def evaluate_checkpoint(ckpt_or_path, loader, device, knn=None, use_amp=True, return_preds=False):
    """ckpt_or_path: a checkpoint dict as semseg.pretrained.load_checkpoint returns it, or a path to one.  loader yields
    item dicts {"xyz", "depth", "label", "mask"[, "reflectance"]}.  knn: a semseg.models.kNN2d on `device`, or None.
    -> the summary dict of Evaluator (means over classes [1:3]: 'unknown' and 'cyclist' are left out), plus "classes"
    = num_classes.  return_preds=True: -> (summary, preds), preds the list of the per-batch masked predictions
    (int64 [B,H,W] on the device: after the remap and the filter, times the mask -- what the counts were taken of)."""
    ckpt = load_checkpoint(ckpt_or_path) if isinstance(ckpt_or_path, (str, os.PathLike)) else ckpt_or_path
    cfg = ckpt["cfg"]
    device = torch.device(device)
    model = build_from_checkpoint(ckpt, device)
    num_classes = int(cfg.dataset.num_classes)
    evaluator = Evaluator(num_classes, knn=knn, remap=OMIT_REMAP)
    preds = []
    with torch.inference_mode():
        for item in loader:
            item = {k: v.to(device, non_blocking=True) for k, v in item.items()}
            label, mask = item["label"].long(), item["mask"].float()
            inputs = make_inputs(item, cfg.arch.inputs).float()
            with torch.autocast("cuda", dtype=torch.float16, enabled=bool(use_amp)):
                logit = model(inputs, item["xyz"].float(), mask)
            logit = logit[-1] if isinstance(logit, tuple) else logit
            depth = item["depth"].float()
            evaluator.update(logit, label, mask, depth=depth)
            if return_preds:
                # the evaluator's steps again (they are deterministic), for callers that score the predictions themselves
                pred = logit.argmax(dim=1)
                for src, dst in OMIT_REMAP.items():
                    pred = torch.where(pred == src, dst, pred)
                if knn is not None:
                    pred = knn(depth, pred)
                preds.append(pred * (mask != 0).long())
    summary = evaluator.summary(mean_classes=slice(1, 3))
    summary["classes"] = num_classes
    return (summary, preds) if return_preds else summary


__all__ = ["evaluate_checkpoint", "OMIT_REMAP"]
