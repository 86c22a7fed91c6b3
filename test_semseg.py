"""Evaluate a range-image segmentation checkpoint on one GPU (reference: test_semseg.py), headless.

    python test_semseg.py --ckpt_path logs/.../checkpoint_step-0000050000.pth [--data_root data/kitti_raw_frontal]
                          [--batch_size 32] [--knn_enabled] [--knn_k 5] [--knn_kernel_size 5] [--shape 64 512]
    python test_semseg.py --ckpt_path model.pth --synthetic 32        # no data on disk: semseg.datasets.SyntheticFrontal

The checkpoint is one written by train_semseg.py or by the reference (semseg.pretrained.load_checkpoint reads both,
through a restricted unpickler).  The validation set is KITTIRawFrontal(split="val", omit_cyclist=True) under
--data_root.  Prints the per-class IoU / precision / recall table as plain text, then one JSON line with the same
numbers and the integer counts.  Nothing is fetched from anywhere."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "dusty-gan-v2_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ckpt_path", type=str, required=True)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--knn_enabled", action="store_true")
    ap.add_argument("--knn_k", type=int, default=5)
    ap.add_argument("--knn_kernel_size", type=int, default=5)
    ap.add_argument("--data_root", type=str, default="data/kitti_raw_frontal")
    ap.add_argument("--synthetic", type=int, default=None, metavar="N",
                    help="score SyntheticFrontal(length=N) instead of the files under --data_root")
    ap.add_argument("--shape", type=int, nargs=2, default=None, metavar=("H", "W"),
                    help="scan size (default: the checkpoint's cfg.dataset.shape)")
    return ap


def format_table(class_list, summary):
    """The reference's table (test_semseg.py:150-159) as plain text lines."""
    rows = [("class", "iou", "precision", "recall")]
    for i, name in enumerate(class_list):
        rows.append((name, f"{summary['iou'][i]:.1%}", f"{summary['precision'][i]:.1%}", f"{summary['recall'][i]:.1%}"))
    rows.append(("mean", f"{summary['mean_iou']:.1%}", f"{summary['mean_precision']:.1%}", f"{summary['mean_recall']:.1%}"))
    width = max(len(r[0]) for r in rows)
    return [f"{r[0]:<{width}}  {r[1]:>9}  {r[2]:>9}  {r[3]:>9}" for r in rows]


def json_record(args, class_list, summary, num_scans):
    def num(v):
        v = float(v)
        return v if math.isfinite(v) else None
    rec = {"ckpt_path": args.ckpt_path, "scans": int(num_scans), "knn": bool(args.knn_enabled), "classes": list(class_list)}
    for key in ("iou", "precision", "recall"):
        rec[key] = [num(v) for v in summary[key]]
        rec["mean_" + key] = num(summary["mean_" + key])
    for key in ("tp", "fp", "fn"):
        rec[key] = [int(v) for v in summary[key]]
    return rec


def main(argv=None):
    args = build_parser().parse_args(argv)

    import torch
    from semseg.datasets import KITTIRawFrontal, SyntheticFrontal
    from semseg.evaluation import evaluate_checkpoint
    from semseg.models import kNN2d
    from semseg.pretrained import load_checkpoint

    device = torch.device("cuda", 0)
    ckpt = load_checkpoint(args.ckpt_path)
    cfg = ckpt["cfg"]
    shape = tuple(args.shape) if args.shape is not None else tuple(cfg.dataset.shape)
    num_classes = int(cfg.dataset.num_classes)
    if args.synthetic is not None:
        val_set = SyntheticFrontal(length=args.synthetic, shape=shape, num_classes=num_classes)
    else:
        val_set = KITTIRawFrontal(root=args.data_root, split="val", shape=shape, omit_cyclist=True)
    loader = torch.utils.data.DataLoader(val_set, batch_size=args.batch_size, num_workers=0, shuffle=False, drop_last=False)
    knn = None
    if args.knn_enabled:
        knn = kNN2d(num_classes=num_classes, k=args.knn_k, kernel_size=args.knn_kernel_size).to(device)
    summary = evaluate_checkpoint(ckpt, loader, device, knn=knn, use_amp=True)
    class_list = list(val_set.class_list)[:num_classes]
    for line in format_table(class_list, summary):
        print(line)
    print(json.dumps(json_record(args, class_list, summary, len(val_set)), allow_nan=False), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
