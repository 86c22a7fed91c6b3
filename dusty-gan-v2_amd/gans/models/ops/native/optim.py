"""native.optim: parameter updates -- list lerp (G_ema), the fused Adam step, the EMA scalar launches of the modulated layers.

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI; package docstring and DESIGN.md section 27: the import rules).
"""
import torch

import dgv2_native as N


def lerp_list(dst, src, weight):
    """dst[i] <- lerp(dst[i], src[i], weight) for lists of fp32 tensors, 72 per launch (the G_ema update)."""
    for i in range(0, len(dst), 72):
        d, s_ = dst[i:i + 72], src[i:i + 72]
        N.check(*d, *s_)
        N.call("dgv2_lerp_list", N.ptr_array(d), N.ptr_array(s_), N.int_array([t.numel() for t in d]), len(d),
               float(weight), N.stream())


def fused_adam_step(opt):
    """One step of a torch.optim.Adam instance (single param group, no weight decay / amsgrad / maximize) on the
    dgv2 kernels: the optimizer object, its hyper-parameters and its state_dict stay torch's, only the arithmetic
    moves (1 + ceil(L/72) launches at HBM speed instead of torch's multi-tensor kernels).  The per-parameter
    `step` entries alias ONE device counter."""
    (group,) = opt.param_groups
    if group["weight_decay"] != 0 or group["amsgrad"] or group["maximize"]:
        raise RuntimeError("dgv2 fused Adam: unsupported optimizer options")
    params = [p for p in group["params"] if p.grad is not None]
    if not params:
        return
    dev = params[0].device
    shared = getattr(opt, "_dgv2_step", None)
    if shared is None:
        shared = torch.zeros(1, device=dev, dtype=torch.float32)
        opt._dgv2_step = shared
        opt._dgv2_sc = torch.zeros(4, device=dev, dtype=torch.float32)
    for p in params:
        st = opt.state[p]
        if len(st) == 0:
            st["step"] = shared.view(())
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        elif st["step"].data_ptr() != shared.data_ptr():      # state came from load_state_dict: adopt its counter
            shared.copy_(st["step"].reshape(1).to(dev, torch.float32))
            st["step"] = shared.view(())
    b1, b2 = group["betas"]
    N.call("dgv2_adam_prep", N.ptr(opt._dgv2_sc), N.ptr(shared), float(b1), float(b2), N.stream())
    for i in range(0, len(params), 72):
        ch = params[i:i + 72]
        ms = [opt.state[p]["exp_avg"] for p in ch]
        vs = [opt.state[p]["exp_avg_sq"] for p in ch]
        gs = [p.grad for p in ch]
        N.check(*ch, *gs, *ms, *vs)
        N.call("dgv2_adam_step", N.ptr_array(ch), N.ptr_array(gs), N.ptr_array(ms), N.ptr_array(vs),
               N.int_array([p.numel() for p in ch]), len(ch), N.ptr(opt._dgv2_sc), float(group["lr"]), float(b1),
               float(b2), float(group["eps"]), N.stream())


def ema_update(ema, sumsq, add, count, weight, update=True, cvec=None):
    """ModConv2d's input-magnitude EMA (style.py:98-103) in one scalar launch: updates the 0-dim buffer `ema`
    in place with lerp(ema, (sumsq + add) / count, weight) and returns a fresh [1] snapshot of its value.
    cvec (fp32 [n], optional): filled with the layer's output factor 1/(sqrt(ema)+1e-8) instead (returns cvec)."""
    snap = None if cvec is not None else torch.empty(1, device=ema.device, dtype=torch.float32)
    N.call("dgv2_ema_scalar", N.ptr(ema), N.ptr(snap), N.ptr(sumsq), 0 if sumsq is None else sumsq.numel(), float(add),
           1.0 / float(count), float(weight), int(update), N.ptr(cvec), 0 if cvec is None else cvec.numel(), N.stream())
    return snap if cvec is None else cvec


def ema_update_group(emas, rows, sumsq, add, count, weight, update, cvec):
    """ema_update for up to 8 layers that share their input (the output heads of a level, dusty_v2.py:32-57) in ONE
    launch: emas[i] is updated as ema_update would, and rows[i] entries of cvec (behind those of the layers before it)
    get that layer's output factor."""
    assert 1 <= len(emas) <= 8 and cvec is not None and cvec.numel() >= sum(rows)
    N.check(*emas, cvec, sumsq)
    N.call("dgv2_ema_scalar_group", N.ptr_array(emas), N.int_array(rows), len(emas), N.ptr(sumsq),
           0 if sumsq is None else sumsq.numel(), float(add), 1.0 / float(count), float(weight), int(update), N.ptr(cvec),
           N.stream())
    return cvec


__all__ = ["lerp_list", "fused_adam_step", "ema_update", "ema_update_group"]
