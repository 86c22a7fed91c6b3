"""native.loss: the non-saturating GAN objective and its logged statistics in one launch.

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI; package docstring and DESIGN.md section 27: the import rules).
"""
import torch
from torch.autograd import Function

import dgv2_native as N


# ---------------------------------------------------------------------------------------
# non-saturating GAN objective + logged statistics in one launch (dgv2_nsgan_loss)
# ---------------------------------------------------------------------------------------
class _NsganLoss(Function):
    """loss = mean softplus(-y[:n_real]) + mean softplus(y[n_real:]); also returns (no gradient) the 4 statistics
    [loss, mean y_real, mean y_fake, sum sign(y_real)].  First order only (the R1 penalty does not go through it)."""

    @staticmethod
    def forward(ctx, y, n_real):
        yf = y.detach().float().contiguous().reshape(-1)
        n = yf.numel()
        stats = torch.empty(4, device=y.device, dtype=torch.float32)
        gy = torch.empty(n, device=y.device, dtype=torch.float32)
        N.check(yf)
        N.call("dgv2_nsgan_loss", N.ptr(stats), N.ptr(gy), N.ptr(yf), int(n_real), n - int(n_real), 1.0, None, None, N.stream())
        ctx.save_for_backward(gy)
        ctx.shape, ctx.dtype = y.shape, y.dtype
        ctx.mark_non_differentiable(stats)
        return stats[0].clone(), stats

    @staticmethod
    def backward(ctx, g, _):
        (gy,) = ctx.saved_tensors
        return (gy * g).reshape(ctx.shape).to(ctx.dtype), None


def nsgan_loss(y, n_real):
    """(loss, stats[4]) for logits y [n,1] with the first n_real rows judged as real (see _NsganLoss)."""
    return _NsganLoss.apply(y, n_real)


def nsgan_step(y, n_real, weight=1.0, cum=None):
    """The objective of a step body WITHOUT a scalar-loss graph: (stats[4], gy) with gy = weight * d loss / d y shaped like
    y -- the cotangent the body hands to y.backward(gy).  One launch; `(weight * loss).backward()` costs a clone, a scalar
    multiply, the ones_like seed, the multiply's backward and the broadcast product with the saved gradient on top.
    cum = (sign_cum, n_pred_cum): AdaptiveAugment's fp32 [1] buffers, updated in the same launch (its `cumulate`)."""
    yf = y.detach().float().contiguous().reshape(-1)
    n = yf.numel()
    stats = torch.empty(4, device=y.device, dtype=torch.float32)
    gy = torch.empty(n, device=y.device, dtype=torch.float32)
    N.check(yf)
    sc, nc = (None, None) if cum is None else cum
    if cum is not None and not all(t.is_cuda and t.dtype == torch.float32 and t.numel() == 1 for t in cum):
        raise ValueError("nsgan_step: cum = (sign_cum, n_pred_cum), fp32 [1] device tensors")
    N.call("dgv2_nsgan_loss", N.ptr(stats), N.ptr(gy), N.ptr(yf), int(n_real), n - int(n_real), float(weight), N.ptr(sc),
           N.ptr(nc), N.stream())
    return stats, gy.reshape(y.shape).to(y.dtype)


__all__ = ["nsgan_loss", "nsgan_step"]
