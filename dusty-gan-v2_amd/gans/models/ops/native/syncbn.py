"""native.syncbn: training-mode batch norm whose statistics run over every rank's samples (torch.nn.SyncBatchNorm's
semantics) on the dgv2_bn_* entries (csrc/syncbn.hip; include/dgv2.h "Synchronised batch norm" states the arithmetic,
DESIGN.md section 39 the measurements).

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI, see the package docstring).  Each direction is two
launches -- per-plane float64 partial sums, then the fold and the element-wise pass -- with ONE all_gather of the
[B,C,2] float64 block between them when more than one rank takes part.  The fold adds the samples' partials in global
sample order, so statistics, output and input gradient are the same bits however the batch is split over ranks.
Nothing here synchronises or reads a value on the host, except the once-per-shape agreement check of a multi-rank
group.  First order only.
"""
import torch
import torch.distributed as dist
from torch.autograd.function import once_differentiable

import dgv2_native as N

from gans import parallel

_BN_DTYPES = {torch.float32: N.F32, torch.bfloat16: N.BF16, torch.float16: N.F16}
_checked_shapes = set()


def _check_x(name, x):
    if x.ndim != 4:
        raise ValueError(f"{name}: x must be [B,C,H,W], got {tuple(x.shape)}")
    if x.dtype not in _BN_DTYPES:
        raise RuntimeError(f"{name}: unsupported dtype {x.dtype} (float32 / bfloat16 / float16 only)")
    if min(x.shape) < 1:
        raise ValueError(f"{name}: empty input {tuple(x.shape)}")
    N.check(x)


def _check_vec(name, what, t, C, dev, dtype=torch.float32):
    if t is None:
        return
    if tuple(t.shape) != (C,) or t.dtype != dtype:
        raise ValueError(f"{name}: {what} must be {dtype} [{C}], got {t.dtype} {tuple(t.shape)}")
    N.check(t)
    if t.device != dev:
        raise RuntimeError(f"{name}: {what} must be on x's device")


def _check_part(name, part, Btot, C, dev):
    if tuple(part.shape) != (Btot, C, 2) or part.dtype != torch.float64:
        raise ValueError(f"{name}: part must be float64 [{Btot},{C},2], got {part.dtype} {tuple(part.shape)}")
    N.check(part)
    if part.device != dev:
        raise RuntimeError(f"{name}: part must be on x's device")


def bn_partials(x):
    """x [B,C,H,W] (float32 / bfloat16 / float16, contiguous, on the device) -> float64 [B,C,2]: (sum x, sum x^2) of
    every (sample, channel) plane, added in an order that only H * W and the dtype fix.  One launch."""
    _check_x("bn_partials", x)
    B, C, H, W = x.shape
    part = torch.empty((B, C, 2), device=x.device, dtype=torch.float64)
    N.call("dgv2_bn_partials", N.ptr(part), N.ptr(x), B, C, H, W, _BN_DTYPES[x.dtype], N.stream())
    return part


def bn_apply(x, part, weight, bias, running_mean, running_var, num_batches_tracked, eps, momentum):
    """The fold and the normalisation.  part: float64 [Btot,C,2], the partials of every rank's samples in global sample
    order (one rank: bn_partials(x)).  -> (y in x's dtype, mean float32 [C], invstd float32 [C]); the running buffers
    and num_batches_tracked are updated in place as torch.nn.SyncBatchNorm updates them (None: not kept; momentum None:
    the cumulative average).  ValueError where Btot * H * W == 1, as torch.  One launch."""
    _check_x("bn_apply", x)
    B, C, H, W = x.shape
    dev = x.device
    if part.ndim != 3 or part.shape[0] < B:
        raise ValueError(f"bn_apply: part must be float64 [Btot >= {B},{C},2], got {tuple(part.shape)}")
    Btot = part.shape[0]
    _check_part("bn_apply", part, Btot, C, dev)
    for what, t in (("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var)):
        _check_vec("bn_apply", what, t, C, dev)
    if (running_mean is None) != (running_var is None):
        raise ValueError("bn_apply: running_mean and running_var come together")
    if num_batches_tracked is not None:
        if num_batches_tracked.numel() != 1 or num_batches_tracked.dtype != torch.int64:
            raise ValueError("bn_apply: num_batches_tracked must be one int64")
        N.check(num_batches_tracked)
    if Btot * H * W == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    if momentum is None:
        if running_mean is not None and num_batches_tracked is None:
            raise ValueError("bn_apply: the cumulative average (momentum None) needs num_batches_tracked")
        if num_batches_tracked is not None:
            num_batches_tracked.add_(1)   # the kernel reads the count of this batch included
        momentum = -1.0
    elif not 0.0 <= float(momentum) <= 1.0:
        raise ValueError(f"bn_apply: momentum must be in [0, 1] or None, got {momentum}")
    y = torch.empty_like(x)
    mean = torch.empty(C, device=dev, dtype=torch.float32)
    invstd = torch.empty(C, device=dev, dtype=torch.float32)
    N.call("dgv2_bn_apply", N.ptr(y), N.ptr(mean), N.ptr(invstd), N.ptr(running_mean), N.ptr(running_var),
           N.ptr(num_batches_tracked), N.ptr(x), N.ptr(part), N.ptr(weight), N.ptr(bias), B, Btot, C, H, W, float(eps),
           float(momentum), _BN_DTYPES[x.dtype], N.stream())
    return y, mean, invstd


def bn_bwd_partials(dy, x, mean, invstd):
    """dy, x [B,C,H,W] of one dtype; mean, invstd float32 [C] as bn_apply saved them -> float64 [B,C,2]:
    (sum dy, sum dy xhat) per plane, in bn_partials' order.  One launch."""
    _check_x("bn_bwd_partials", x)
    _check_x("bn_bwd_partials", dy)
    if dy.shape != x.shape or dy.dtype != x.dtype or dy.device != x.device:
        raise ValueError("bn_bwd_partials: dy and x must agree in shape, dtype and device")
    B, C, H, W = x.shape
    _check_vec("bn_bwd_partials", "mean", mean, C, x.device)
    _check_vec("bn_bwd_partials", "invstd", invstd, C, x.device)
    if mean is None or invstd is None:
        raise ValueError("bn_bwd_partials: mean and invstd are required")
    part = torch.empty((B, C, 2), device=x.device, dtype=torch.float64)
    N.call("dgv2_bn_bwd_partials", N.ptr(part), N.ptr(dy), N.ptr(x), N.ptr(mean), N.ptr(invstd), B, C, H, W,
           _BN_DTYPES[x.dtype], N.stream())
    return part


def bn_bwd_apply(dy, x, part, mean, invstd, weight, b_off=0, param_grads=True):
    """part: float64 [Btot,C,2], every rank's backward partials in global sample order; b_off: where this rank's B
    samples start in it.  -> (dx in x's dtype, dweight, dbias): the parameter gradients are float32 [C] sums over
    THIS rank's samples (None with param_grads False).  One launch."""
    _check_x("bn_bwd_apply", x)
    _check_x("bn_bwd_apply", dy)
    if dy.shape != x.shape or dy.dtype != x.dtype or dy.device != x.device:
        raise ValueError("bn_bwd_apply: dy and x must agree in shape, dtype and device")
    B, C, H, W = x.shape
    dev = x.device
    if part.ndim != 3 or not 0 <= int(b_off) <= part.shape[0] - B:
        raise ValueError(f"bn_bwd_apply: part must be float64 [Btot,{C},2] with 0 <= b_off <= Btot - {B}")
    Btot = part.shape[0]
    _check_part("bn_bwd_apply", part, Btot, C, dev)
    for what, t in (("mean", mean), ("invstd", invstd), ("weight", weight)):
        _check_vec("bn_bwd_apply", what, t, C, dev)
    if mean is None or invstd is None:
        raise ValueError("bn_bwd_apply: mean and invstd are required")
    if Btot * H * W == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    dx = torch.empty_like(x)
    dweight = torch.empty(C, device=dev, dtype=torch.float32) if param_grads else None
    dbias = torch.empty(C, device=dev, dtype=torch.float32) if param_grads else None
    N.call("dgv2_bn_bwd_apply", N.ptr(dx), N.ptr(dweight), N.ptr(dbias), N.ptr(dy), N.ptr(x), N.ptr(part), N.ptr(mean),
           N.ptr(invstd), N.ptr(weight), B, Btot, int(b_off), C, H, W, _BN_DTYPES[x.dtype], N.stream())
    return dx, dweight, dbias


def _gather(part, shape, group):
    """(the partials of every rank in global sample order, this rank's offset in them).  No process group, or one of a
    single rank: the block itself, no collective.  The ranks must hold equal B, H, W (the sampler and drop_last see to
    it): checked once per group and shape, with one small all_gather and a readback; counts are never gathered."""
    if not parallel.is_dist():
        return part, 0
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    B = part.shape[0]
    key = (id(group), tuple(shape))
    if world > 1 and key not in _checked_shapes:
        mine = torch.tensor([shape[0], shape[2], shape[3]], device=part.device, dtype=torch.int64)
        every = torch.empty(world * 3, device=part.device, dtype=torch.int64)
        dist.all_gather_into_tensor(every, mine, group=group)
        if not bool((every.view(world, 3) == mine).all()):
            raise RuntimeError(f"sync_batch_norm: the ranks hold different [B,H,W]: {every.view(world, 3).tolist()}")
        _checked_shapes.add(key)
    # (flat views: the gloo backend of the one-device tests takes the concatenated form only for 1-D tensors)
    out = torch.empty((world * B,) + tuple(part.shape[1:]), device=part.device, dtype=part.dtype)
    dist.all_gather_into_tensor(out.view(-1), part.view(-1), group=group)
    return out, rank * B


class _SyncBatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, num_batches_tracked, eps, momentum, group):
        part, b_off = _gather(bn_partials(x), x.shape, group)
        y, mean, invstd = bn_apply(x, part, weight, bias, running_mean, running_var, num_batches_tracked, eps, momentum)
        ctx.save_for_backward(x, weight, mean, invstd)
        ctx.group, ctx.b_off = group, b_off
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight, mean, invstd = ctx.saved_tensors
        dy = dy.to(x.dtype).contiguous()
        part, _ = _gather(bn_bwd_partials(dy, x, mean, invstd), x.shape, ctx.group)
        want = weight is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        dx, dweight, dbias = bn_bwd_apply(dy, x, part, mean, invstd, weight, b_off=ctx.b_off, param_grads=want)
        return (dx, dweight if ctx.needs_input_grad[1] else None, dbias if ctx.needs_input_grad[2] else None,
                None, None, None, None, None, None)


def sync_batch_norm(x, weight, bias, running_mean, running_var, num_batches_tracked, eps, momentum, group=None):
    """Training-mode batch norm of x [B,C,H,W] (float32 / bfloat16 / float16, contiguous NCHW, on the device) over the
    samples of every rank of `group` (None: the default group; no initialised group or a single rank: this process's
    samples, no collective).  weight, bias: float32 [C] or None; running_mean, running_var: float32 [C] updated in
    place, or None; num_batches_tracked: one int64, counted, or None; momentum: float, or None for the cumulative
    average.  -> y in x's dtype, differentiable in x, weight and bias; the parameter gradients are sums over this
    rank's samples (torch.nn.SyncBatchNorm's), to be averaged over ranks with the rest of the gradients.
    Every rank must hold the same B, H and W.  Two launches and at most one all_gather each way.  A CPU or
    non-contiguous tensor raises RuntimeError, a wrong shape ValueError; nothing is launched then."""
    _check_x("sync_batch_norm", x)
    for what, t in (("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var)):
        _check_vec("sync_batch_norm", what, t, x.shape[1], x.device)
    if (weight is None) != (bias is None):
        raise ValueError("sync_batch_norm: weight and bias come together")
    if not parallel.is_dist() and x.shape[0] * x.shape[2] * x.shape[3] == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    return _SyncBatchNorm.apply(x, weight, bias, running_mean, running_var, num_batches_tracked, eps, momentum, group)


__all__ = ["sync_batch_norm", "bn_partials", "bn_apply", "bn_bwd_partials", "bn_bwd_apply"]
