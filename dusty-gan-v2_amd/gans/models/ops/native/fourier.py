"""native.fourier: the positional encoding -- Fourier features and the angle pyramid, the angle gradient of the encoding
(reference: autograd through ops/fourier.py:77-82), and the generator's level input (FIR up-2 written next to the encoding).

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI; package docstring and DESIGN.md section 27: the import rules).
"""
import torch
from torch.autograd import Function

import dgv2_native as N
from .act_resample import _dt, _resample_raw


# ---------------------------------------------------------------------------------------
# Fourier features / angle pyramid (no gradient: angles are inputs of the training path)
# ---------------------------------------------------------------------------------------
def fourier_feature_into(out, c0, angle, shift, freqs2, phase):
    """Write cat(sin, cos) of the encoding into channels [c0, c0+2F) of `out` [B,H,W,ld]."""
    B, H, W, ld = out.shape
    F = phase.numel()
    N.check(out, angle, shift, freqs2, phase)
    N.call("dgv2_fourier_feature", N.ptr(out), N.ptr(angle), N.ptr(shift), N.ptr(freqs2), N.ptr(phase),
           B, angle.shape[0], H, W, F, ld, c0, _dt(out), N.stream())


def downsample_angle(angle, shift, taps, B, ring=True):
    Ba, _, H, W = angle.shape
    N.check(angle, shift, taps)
    out = torch.empty((B, 2, H // 2, W // 2), device=angle.device, dtype=torch.float32)
    N.call("dgv2_downsample_angle", N.ptr(out), N.ptr(angle), N.ptr(shift), N.ptr(taps), B, Ba, H, W, int(ring),
           N.stream())
    return out


# ---------------------------------------------------------------------------------------
# angle gradient of the positional encoding (reference: autograd through ops/fourier.py:77-82)
# ---------------------------------------------------------------------------------------
def fourier_feature_bwd(g, c0, angle, shift, freqs2, phase):
    """g_angle (angle's shape, fp32) from the gradient `g` [B,H,W,ld] of an activation whose channels [c0, c0+2F) hold
    the encoding of `angle` [B or 1,2,H,W] (+ shift [B] on the azimuth)."""
    B, H, W, ld = g.shape
    Ba = angle.shape[0]
    out = torch.empty((B, 2, H, W), device=g.device, dtype=torch.float32)
    N.check(g, angle, shift, freqs2, phase)
    N.call("dgv2_fourier_feature_bwd", N.ptr(out), N.ptr(g), N.ptr(angle), N.ptr(shift), N.ptr(freqs2), N.ptr(phase),
           B, Ba, H, W, phase.numel(), ld, c0, N.dtype_code(g), N.stream())
    return out if Ba == B else out.sum(dim=0, keepdim=True)


class _FourierFeature(Function):
    @staticmethod
    def forward(ctx, angle, shift, freqs2, phase, dtype, B):
        _, _, H, W = angle.shape
        angle = angle.detach().float().contiguous()
        out = torch.empty((B, H, W, 2 * phase.numel()), device=angle.device, dtype=dtype)
        fourier_feature_into(out, 0, angle, shift, freqs2, phase)
        ctx.cfg = (angle, shift, freqs2, phase)
        return out

    @staticmethod
    def backward(ctx, g):
        angle, shift, freqs2, phase = ctx.cfg
        return fourier_feature_bwd(g.contiguous(), 0, angle, shift, freqs2, phase), None, None, None, None, None


def fourier_feature(angle, shift, freqs2, phase, dtype=torch.float32, B=None):
    """[B,H,W,2F] channels-last encoding of `angle`, differentiable w.r.t. the angles."""
    return _FourierFeature.apply(angle, shift, freqs2, phase, dtype, angle.shape[0] if B is None else B)


# ---------------------------------------------------------------------------------------
# level input of the generator: FIR up-2 of h written next to the positional encoding
# (reference: SynthesisBlock.forward, gans/models/dusty_v2.py:153-159 -- resample + cat)
# ---------------------------------------------------------------------------------------
class _UpCatPE(Function):
    @staticmethod
    def forward(ctx, h, spec, angle, shift, freqs2, phase, dtype, B):
        F2 = 2 * phase.numel()
        if h is None:
            H, W = angle.shape[2:]
            Cin = 0
        else:
            h = h.contiguous()
            B = h.shape[0]
            Cin = h.shape[3]
            H, W = spec.out_size(h.shape[1], h.shape[2])
        x1 = torch.empty((B, H, W, Cin + F2), device=angle.device, dtype=dtype)
        if h is not None:
            _resample_raw(h, spec, False, (h.shape[1], h.shape[2]), out=x1, ldy=Cin + F2)
        angle_d = angle.detach().float().contiguous()
        fourier_feature_into(x1, Cin, angle_d, shift, freqs2, phase)
        ctx.cfg = (spec, None if h is None else (h.shape[1], h.shape[2]), Cin)
        # the angle gradient (inversion: demo_inversion.py:164 optimises angle + phase) recomputes the encoding from these
        ctx.pe = (angle_d, shift, freqs2, phase) if ctx.needs_input_grad[2] else None
        return x1

    @staticmethod
    def backward(ctx, g):
        spec, in_hw, Cin = ctx.cfg
        g = g.contiguous()
        gh = ga = None
        if in_hw is not None and ctx.needs_input_grad[0]:
            gh = _resample_raw(g, spec, True, in_hw, ldx=g.shape[3], C=Cin)
        if ctx.pe is not None:
            ga = fourier_feature_bwd(g, Cin, *ctx.pe)
        return gh, None, ga, None, None, None, None, None


def up_cat_pe(h, spec, angle, shift, freqs2, phase, dtype, B):
    """[B,H,W,Cin+2F] = cat(FIR-up2(h), PE(angle (+shift on azimuth))) without a concat pass."""
    return _UpCatPE.apply(h, spec, angle, shift, freqs2, phase, dtype, B)


__all__ = ["fourier_feature_into", "downsample_angle", "fourier_feature_bwd", "fourier_feature", "up_cat_pe"]
