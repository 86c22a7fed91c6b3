"""native.crf: the CRF-RNN mean-field refinement of the range-image segmentation models (reference:
semseg/models/crf_as_rnn.py:110-132) as one autograd node over dgv2_crf_rnn_forward / dgv2_crf_rnn_backward
(include/dgv2.h states the arithmetic).

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI, see the package docstring).  First order only.
"""
import torch
from torch.autograd.function import once_differentiable

import dgv2_native as N

C_MAX, KH_MAX, KW_MAX = 8, 5, 9


def check_crf_config(num_classes, kernel_size):
    """The range the kernels cover; ValueError outside it (there is no other path)."""
    kh, kw = kernel_size
    if not 1 <= int(num_classes) <= C_MAX:
        raise ValueError(f"crf_rnn: 1 <= num_classes <= {C_MAX} is supported, got {num_classes}")
    if kh < 1 or kw < 1 or kh % 2 == 0 or kw % 2 == 0:
        raise ValueError(f"crf_rnn: the kernel size must be odd, got {(kh, kw)}")
    if kh > KH_MAX or kw > KW_MAX:
        raise ValueError(f"crf_rnn: kernel sizes up to ({KH_MAX}, {KW_MAX}) are supported, got {(kh, kw)}")


class _CRFRNN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, unary, ws, wa, compat, xyz, mask, kg, ka, tb, num_iters):
        B, C, H, W = unary.shape
        kh, kw = kg.shape[2:]
        out = torch.empty_like(unary)
        qsave = torch.empty((num_iters - 1, B, C, H, W), device=unary.device, dtype=torch.float32) if num_iters > 1 else None
        N.call("dgv2_crf_rnn_forward", N.ptr(out), N.ptr(qsave), N.ptr(unary), N.ptr(xyz), N.ptr(mask), N.ptr(kg), N.ptr(ka),
               N.ptr(tb), N.ptr(ws), N.ptr(wa), N.ptr(compat), B, C, H, W, kh, kw, num_iters, N.stream())
        ctx.save_for_backward(unary, ws, wa, compat, xyz, mask, kg, ka, tb, qsave)
        ctx.num_iters = num_iters
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        unary, ws, wa, compat, xyz, mask, kg, ka, tb, qsave = ctx.saved_tensors
        B, C, H, W = unary.shape
        kh, kw = kg.shape[2:]
        g_out = g_out.float().contiguous()
        N.check(g_out)
        scratch = torch.empty(N.scratch_elems("dgv2_crf_rnn_backward_scratch", B, C, H, W, ctx.num_iters), device=unary.device,
                              dtype=torch.float32)
        g_unary, g_ws, g_wa, g_compat = (torch.empty_like(t) for t in (unary, ws, wa, compat))
        N.call("dgv2_crf_rnn_backward", N.ptr(g_unary), N.ptr(g_ws), N.ptr(g_wa), N.ptr(g_compat), N.ptr(scratch),
               scratch.numel(), N.ptr(g_out), N.ptr(qsave), N.ptr(unary), N.ptr(xyz), N.ptr(mask), N.ptr(kg), N.ptr(ka), N.ptr(tb),
               N.ptr(ws), N.ptr(wa), N.ptr(compat), B, C, H, W, kh, kw, ctx.num_iters, N.stream())
        return g_unary, g_ws, g_wa, g_compat, None, None, None, None, None, None


def crf_rnn(unary, xyz, mask, kernel_gamma, kernel_alpha, theta_beta, weight_smoothness, weight_appearance, compat,
            num_iters):
    """unary [B,C,H,W], xyz [B,3,H,W], mask [B,H,W] or [B,1,H,W] (multiplied in; may be non-binary) -> refined logits
    [B,C,H,W] float32 after `num_iters` mean-field iterations.  kernel_gamma / kernel_alpha [C,C,kh,kw] (diagonal
    read), theta_beta [C], weight_smoothness / weight_appearance C values, compat C x C values (any shape with that
    many elements; their gradients come back in the same shape).

    Gradients reach unary, weight_smoothness, weight_appearance and compat.  xyz and mask get none: the reference
    detaches the bilateral kernel, and the mask's gradient is not produced.  Double backward raises."""
    if unary.ndim != 4:
        raise ValueError(f"crf_rnn: unary must be [B,C,H,W], got {tuple(unary.shape)}")
    B, C, H, W = unary.shape
    if kernel_gamma.ndim != 4 or tuple(kernel_gamma.shape[:2]) != (C, C) or kernel_alpha.shape != kernel_gamma.shape:
        raise ValueError(f"crf_rnn: kernel_gamma / kernel_alpha must be [{C},{C},kh,kw], got "
                         f"{tuple(kernel_gamma.shape)} / {tuple(kernel_alpha.shape)}")
    check_crf_config(C, tuple(kernel_gamma.shape[2:]))
    if min(B, H, W) < 1:
        raise ValueError(f"crf_rnn: empty unary {tuple(unary.shape)}")
    if tuple(xyz.shape) != (B, 3, H, W):
        raise ValueError(f"crf_rnn: xyz must be [{B},3,{H},{W}], got {tuple(xyz.shape)}")
    if tuple(mask.shape) not in ((B, H, W), (B, 1, H, W)):
        raise ValueError(f"crf_rnn: mask must be [{B},{H},{W}] or [{B},1,{H},{W}], got {tuple(mask.shape)}")
    if theta_beta.numel() != C or weight_smoothness.numel() != C or weight_appearance.numel() != C or compat.numel() != C * C:
        raise ValueError("crf_rnn: theta_beta / weight_smoothness / weight_appearance need C values, compat C x C")
    num_iters = int(num_iters)
    if num_iters < 0:
        raise ValueError(f"crf_rnn: num_iters must be >= 0, got {num_iters}")
    if num_iters == 0:
        return unary
    unary, ws, wa, compat = (t.float().contiguous() for t in (unary, weight_smoothness, weight_appearance, compat))
    xyz, mask, kg, ka, tb = (t.detach().float().contiguous() for t in (xyz, mask.reshape(B, H, W), kernel_gamma,
                                                                        kernel_alpha, theta_beta))
    N.check(unary, ws, wa, compat, xyz, mask, kg, ka, tb)
    return _CRFRNN.apply(unary, ws, wa, compat, xyz, mask, kg, ka, tb, num_iters)


__all__ = ["crf_rnn", "check_crf_config"]
