"""native.segloss: the training objective of the range-image segmentation models -- focal loss (reference:
semseg/models/loss.py:13-21) under the masked mean of train_semseg.py:194-197, with the step's predictions and training
confusion counts (its lines 270-273, 290-296) -- as autograd nodes over dgv2_seg_loss_forward / dgv2_seg_loss_backward
(include/dgv2.h states the arithmetic).

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI, see the package docstring).  Launches: the
per-pixel map takes one forward and one backward launch; the masked scalar takes two forward launches (the per-pixel
pass, then one block that folds the blocks' partial sums in a fixed order and divides) and one backward launch, which
reads the upstream gradient and the mask's sum on the device.  Nothing here synchronises or reads a value on the host.
First order only.
"""
import torch
from torch.autograd.function import once_differentiable

import dgv2_native as N

SEG_LOSS_C_MAX = 32
_DTYPE_CODES = {torch.float32: N.F32, torch.bfloat16: N.BF16, torch.float16: N.F16}


def check_seg_loss_config(num_classes, gamma):
    """The range the kernels cover; ValueError outside it (there is no other path).  0 < gamma < 1 is excluded
    because the reference's own gradient is NaN there wherever the label's probability rounds to 1."""
    if not 1 <= int(num_classes) <= SEG_LOSS_C_MAX:
        raise ValueError(f"seg_loss: 1 <= num_classes <= {SEG_LOSS_C_MAX} is supported, got {num_classes}")
    gamma = float(gamma)
    if not (gamma == 0.0 or gamma >= 1.0):
        raise ValueError(f"seg_loss: gamma must be 0 or >= 1, got {gamma}")


def _prepare(name, logit, label, mask, alpha, gamma, conf=None):
    if logit.ndim != 4:
        raise ValueError(f"{name}: logit must be [B,C,H,W], got {tuple(logit.shape)}")
    B, C, H, W = logit.shape
    check_seg_loss_config(C, gamma)
    if min(B, H, W) < 1:
        raise ValueError(f"{name}: empty logit {tuple(logit.shape)}")
    if tuple(label.shape) != (B, H, W):
        raise ValueError(f"{name}: label must be [{B},{H},{W}], got {tuple(label.shape)}")
    if mask is not None and tuple(mask.shape) != (B, H, W):
        raise ValueError(f"{name}: mask must be [{B},{H},{W}], got {tuple(mask.shape)}")
    if alpha is not None and alpha.numel() != C:
        raise ValueError(f"{name}: alpha needs {C} values, got {tuple(alpha.shape)}")
    if conf is not None and (tuple(conf.shape) != (C + 1, C + 1) or conf.dtype != torch.int64):
        raise ValueError(f"{name}: conf must be int64 [{C + 1},{C + 1}], got {conf.dtype} {tuple(conf.shape)}")
    if logit.dtype not in _DTYPE_CODES:
        logit = logit.float()
    logit, label = logit.contiguous(), label.long().contiguous()
    mask = None if mask is None else mask.detach().float().contiguous()
    alpha = None if alpha is None else alpha.detach().float().reshape(C).contiguous()
    N.check(logit, label, mask, alpha, conf)
    return logit, label, mask, alpha, float(gamma)


class _SegFocalLossMap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, label, alpha, gamma):
        B, C, H, W = logit.shape
        loss_map = torch.empty((B, H, W), device=logit.device, dtype=torch.float32)
        N.call("dgv2_seg_loss_forward", N.ptr(loss_map), None, None, None, None, 0, N.ptr(logit), N.ptr(label), None,
               N.ptr(alpha), B, C, H, W, gamma, _DTYPE_CODES[logit.dtype], N.stream())
        ctx.save_for_backward(logit, label, alpha)
        ctx.gamma = gamma
        return loss_map

    @staticmethod
    @once_differentiable
    def backward(ctx, g_map):
        logit, label, alpha = ctx.saved_tensors
        B, C, H, W = logit.shape
        g_map = g_map.float().contiguous()
        N.check(g_map)
        g_logit = torch.empty_like(logit)
        N.call("dgv2_seg_loss_backward", N.ptr(g_logit), N.ptr(logit), N.ptr(label), None, N.ptr(alpha), N.ptr(g_map),
               None, B, C, H, W, ctx.gamma, _DTYPE_CODES[logit.dtype], 1, N.stream())
        return g_logit, None, None, None


class _SegMaskedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, label, mask, alpha, gamma, conf, want_pred):
        B, C, H, W = logit.shape
        scratch = torch.empty(N.scratch_elems("dgv2_seg_loss_scratch", B, H, W), device=logit.device, dtype=torch.float32)
        sums = torch.empty(3, device=logit.device, dtype=torch.float32)
        pred = torch.empty((B, H, W), device=logit.device, dtype=torch.int64) if want_pred else None
        N.call("dgv2_seg_loss_forward", None, N.ptr(pred), N.ptr(conf), N.ptr(sums), N.ptr(scratch), scratch.numel(),
               N.ptr(logit), N.ptr(label), N.ptr(mask), N.ptr(alpha), B, C, H, W, gamma, _DTYPE_CODES[logit.dtype],
               N.stream())
        ctx.save_for_backward(logit, label, mask, alpha, sums)
        ctx.gamma = gamma
        ctx.set_materialize_grads(False)    # no [B,H,W] zeros for pred's absent gradient
        loss = sums[0]
        if pred is None:
            return loss, None
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _g_pred):
        if g_loss is None:
            return None, None, None, None, None, None, None
        logit, label, mask, alpha, sums = ctx.saved_tensors
        B, C, H, W = logit.shape
        g_loss = g_loss.float().contiguous()
        N.check(g_loss)
        g_logit = torch.empty_like(logit)
        N.call("dgv2_seg_loss_backward", N.ptr(g_logit), N.ptr(logit), N.ptr(label), N.ptr(mask), N.ptr(alpha),
               N.ptr(g_loss), N.ptr(sums), B, C, H, W, ctx.gamma, _DTYPE_CODES[logit.dtype], 0, N.stream())
        return g_logit, None, None, None, None, None, None


def seg_focal_loss_map(logit, label, alpha, gamma):
    """logit [B,C,H,W] (float32 / bfloat16 / float16 kept, anything else cast to float32), label [B,H,W] (cast to
    int64), alpha None or C class weights -> the focal loss per pixel, float32 [B,H,W], unmasked (the reference's
    reduction="none"): -alpha[y] (1 - p_y)^gamma log p_y, 0 where the label is outside [0, C).  gamma is 0 or >= 1.
    Differentiable in logit (the gradient comes back in logit's dtype); one launch each way.  Double backward raises."""
    logit, label, _, alpha, gamma = _prepare("seg_focal_loss_map", logit, label, None, alpha, gamma)
    return _SegFocalLossMap.apply(logit, label, alpha, gamma)


def seg_masked_loss(logit, label, mask, alpha, gamma, conf=None, want_pred=True):
    """logit, label, alpha, gamma as seg_focal_loss_map; mask [B,H,W] (cast to float32; None: ones) -> (loss, pred).
    loss: 0-dim float32, sum(mask * loss_map) / sum(mask) (NaN where the mask sums to 0, as the reference),
    differentiable in logit.  pred: int64 [B,H,W], argmax over the classes (lowest index among equals) times
    (mask != 0), not differentiable; None when want_pred is False.  conf: None or int64 [C+1,C+1] with this call's
    counts ADDED, exactly native.seg_confusion(label, logit.argmax(1), C, mask=mask).
    Two launches forward (per-pixel pass, fold of the partial sums), one backward; the float sums run in a fixed
    order, so the results are bit-identical from run to run.  Double backward raises."""
    logit, label, mask, alpha, gamma = _prepare("seg_masked_loss", logit, label, mask, alpha, gamma, conf)
    return _SegMaskedLoss.apply(logit, label, mask, alpha, gamma, conf, bool(want_pred))


__all__ = ["seg_focal_loss_map", "seg_masked_loss", "check_seg_loss_config", "SEG_LOSS_C_MAX"]
