"""native.knn: the kNN label filter of the range-image segmentation models (reference: semseg/models/knn.py:38-76)
over dgv2_knn2d, and the confusion counts of their evaluation (reference: test_semseg.py:23-42, 136-137) over
dgv2_seg_confusion (include/dgv2.h states the arithmetic of both).

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI, see the package docstring).  Neither has a
gradient: both produce integers.
"""
import torch

import dgv2_native as N

K_SIDE_MAX, CONFUSION_C_MAX = 5, 32


def check_knn_config(num_classes, k, kernel_size):
    """The range the kernel covers; ValueError outside it (there is no other path)."""
    kh, kw = kernel_size
    if int(num_classes) < 1:
        raise ValueError(f"knn2d: num_classes must be >= 1, got {num_classes}")
    if kh < 1 or kw < 1 or kh % 2 == 0 or kw % 2 == 0:
        raise ValueError(f"knn2d: the kernel size must be odd, got {(kh, kw)}")
    if kh > K_SIDE_MAX or kw > K_SIDE_MAX:
        raise ValueError(f"knn2d: kernel sizes up to ({K_SIDE_MAX}, {K_SIDE_MAX}) are supported, got {(kh, kw)}")
    if kh * kw == 1:
        raise ValueError("knn2d: a 1 x 1 window has a zero distance kernel (0 * inf); use a larger one")
    if not 1 <= int(k) <= kh * kw:
        raise ValueError(f"knn2d: 1 <= k <= {kh * kw} for a {(kh, kw)} window, got {k}")


def knn2d(depth, label, dist_kernel, k, num_classes, cutoff):
    """depth [B,1,H,W] (cast to float32), label [B,H,W] (cast to int64), dist_kernel [1,1,kh,kw] or [kh,kw] -> the
    filtered labels, int64 [B,H,W]: per pixel the majority label of the k window slots with the smallest
    distance-kernel-weighted depth jump, slots beyond `cutoff` (when > 0) discarded."""
    if depth.ndim != 4 or depth.shape[1] != 1:
        raise ValueError(f"knn2d: depth must be [B,1,H,W], got {tuple(depth.shape)}")
    B, _, H, W = depth.shape
    if min(B, H, W) < 1:
        raise ValueError(f"knn2d: empty depth {tuple(depth.shape)}")
    if tuple(label.shape) != (B, H, W):
        raise ValueError(f"knn2d: label must be [{B},{H},{W}], got {tuple(label.shape)}")
    if dist_kernel.ndim not in (2, 4) or dist_kernel.numel() != dist_kernel.shape[-2] * dist_kernel.shape[-1]:
        raise ValueError(f"knn2d: dist_kernel must be [1,1,kh,kw] or [kh,kw], got {tuple(dist_kernel.shape)}")
    kh, kw = dist_kernel.shape[-2:]
    check_knn_config(num_classes, k, (kh, kw))
    cutoff = float(cutoff)
    if cutoff != cutoff:
        raise ValueError("knn2d: cutoff is NaN")
    depth, label, dist_kernel = depth.detach().float().contiguous(), label.long().contiguous(), dist_kernel.detach().float().contiguous()
    N.check(depth, label, dist_kernel)
    out = torch.empty((B, H, W), device=depth.device, dtype=torch.int64)
    N.call("dgv2_knn2d", N.ptr(out), N.ptr(depth), N.ptr(label), N.ptr(dist_kernel), B, H, W, kh, kw, int(k),
           int(num_classes), cutoff, N.stream())
    return out


def seg_confusion(label, pred, num_classes, mask=None, out=None):
    """label, pred: integer tensors of one shape; mask: None or a tensor of that shape -> `out` (int64
    [num_classes+1, num_classes+1], zeros when None) with this call's counts ADDED: out[l, p] += 1 per pixel, the last
    row / column collecting values outside [0, num_classes).  Where mask == 0 both label and prediction count as 0 (the
    reference's preds * mask, label * mask); any other mask value counts as 1."""
    C = int(num_classes)
    if not 1 <= C <= CONFUSION_C_MAX:
        raise ValueError(f"seg_confusion: 1 <= num_classes <= {CONFUSION_C_MAX} is supported, got {num_classes}")
    if label.shape != pred.shape or (mask is not None and mask.shape != label.shape):
        raise ValueError(f"seg_confusion: label {tuple(label.shape)}, pred {tuple(pred.shape)}"
                         + (f", mask {tuple(mask.shape)}" if mask is not None else "") + " must have one shape")
    if label.numel() < 1:
        raise ValueError("seg_confusion: empty label")
    label, pred = label.long().contiguous(), pred.long().contiguous()
    mask = None if mask is None else mask.float().contiguous()
    if out is None:
        out = torch.zeros((C + 1, C + 1), device=label.device, dtype=torch.int64)
    elif tuple(out.shape) != (C + 1, C + 1) or out.dtype != torch.int64:
        raise ValueError(f"seg_confusion: out must be int64 [{C + 1},{C + 1}], got {out.dtype} {tuple(out.shape)}")
    N.check(label, pred, mask, out)
    N.call("dgv2_seg_confusion", N.ptr(out), N.ptr(label), N.ptr(pred), N.ptr(mask), label.numel(), C, N.stream())
    return out


__all__ = ["knn2d", "seg_confusion", "check_knn_config"]
