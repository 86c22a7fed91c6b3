"""native.sgd: the segmentation models' optimizer tail -- global-norm clip, loss scale and SGD step in 2 ceil(L/72) + 1 launches.

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI; package docstring and DESIGN.md section 27: the import rules).
"""
import torch

import dgv2_native as N


def fused_clip_sgd_step(opt, max_norm, scale_state=None, growth=2.0, backoff=0.5, growth_interval=2000):
    """One step of a torch.optim.SGD instance (single param group; dampening 0, no Nesterov, no maximize) with what the
    reference's loop runs around it (train_semseg.py:278-283) on the dgv2 kernels (csrc/sgd.hip):
    GradScaler.unscale_ + clip_grad_norm_(max_norm) become one factor on the raw gradients, GradScaler.step's overflow
    skip and GradScaler.update happen on the device.  The optimizer object, its hyper-parameters and its state_dict
    stay torch's (`momentum_buffer` per parameter; a state that load_state_dict brought is adopted); p.grad is only read.

    max_norm <= 0: no clipping.  scale_state: None, or a float32 [2] device tensor (loss scale, growth tracker) that
    the step updates in place.  -> sc, float32 [4] on the device: (unscaled total gradient norm, the factor applied to
    the raw gradients, 1 where the step was skipped for an overflow, the loss scale the step ran under).  No readback.
    sc is ONE buffer kept on the optimizer (opt._dgv2_sc) and the next step overwrites it: clone what must outlive it.
    Parameters without a gradient or without elements are skipped; every tensor must be float32, contiguous, on one
    device and shorter than dgv2_native.SGD_N_MAX elements.  None when no parameter is left.
    ceil(L/72) sum-of-squares launches, one prep launch, ceil(L/72) update launches."""
    (group,) = opt.param_groups
    if group["dampening"] != 0 or group["nesterov"] or group["maximize"]:
        raise RuntimeError("dgv2 fused SGD: unsupported optimizer options")
    params = [p for p in group["params"] if p.grad is not None and p.numel() > 0]
    if not params:
        return None
    dev = params[0].device
    momentum = float(group["momentum"])
    parts = getattr(opt, "_dgv2_parts", None)
    if parts is None or parts.shape[0] != len(params) or parts.device != dev:
        parts = opt._dgv2_parts = torch.zeros((len(params), N.SUMSQ_PARTS), device=dev, dtype=torch.float32)
        opt._dgv2_sc = torch.zeros(4, device=dev, dtype=torch.float32)
    sc = opt._dgv2_sc
    if momentum != 0:
        for p in params:
            st = opt.state[p]
            if st.get("momentum_buffer") is None:
                st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
    if scale_state is not None and (scale_state.dtype != torch.float32 or scale_state.numel() != 2 or scale_state.device != dev):
        raise RuntimeError("dgv2 fused SGD: scale_state must be a float32 [2] tensor (loss scale, growth tracker) on the parameters' device")
    chunks = []
    for i in range(0, len(params), 72):
        ch = params[i:i + 72]
        gs = [p.grad for p in ch]
        ms = [opt.state[p]["momentum_buffer"] for p in ch] if momentum != 0 else [None] * len(ch)
        N.check(*ch, *gs, *ms, scale_state)
        for t in (*ch, *gs, *(m for m in ms if m is not None)):
            if t.dtype != torch.float32:
                raise RuntimeError("dgv2 fused SGD: parameters, gradients and momentum buffers must be float32")
            if t.device != dev:
                raise RuntimeError("dgv2 fused SGD: parameters, gradients and momentum buffers must be on one device")
            if t.numel() > N.SGD_N_MAX:
                raise RuntimeError("dgv2 fused SGD: a tensor of 2^31 elements or more is not supported")
        chunks.append((i, ch, N.ptr_array(gs), N.ptr_array(ms), N.int_array([p.numel() for p in ch])))
    stream = N.stream()
    for i, ch, gs, _, n in chunks:
        N.call("dgv2_sumsq_list", gs, n, len(ch), parts.data_ptr() + 4 * N.SUMSQ_PARTS * i, stream)
    N.call("dgv2_clip_prep", N.ptr(parts), parts.numel(), float(max_norm), N.ptr(scale_state), float(growth),
           float(backoff), int(growth_interval), N.ptr(sc), stream)
    for i, ch, gs, ms, n in chunks:
        N.call("dgv2_sgd_step", N.ptr_array(ch), gs, ms, n, len(ch), N.ptr(sc), float(group["lr"]), momentum,
               float(group["weight_decay"]), stream)
    return sc


__all__ = ["fused_clip_sgd_step"]
