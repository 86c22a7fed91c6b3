"""native.inversion: the differentiable pieces GAN inversion needs (reference: gans/inversion.py, demo_inversion.py):
multi-scale masked loss, range conversion (plain, and with an input gradient).  The angle gradient of the positional
encoding is in native.fourier.

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI; package docstring and DESIGN.md section 27: the import rules).
"""
import torch
from torch.autograd import Function

import dgv2_native as N


_METRICS = {"l1": 0, "mse": 1}


# ---------------------------------------------------------------------------------------
# multi-scale masked loss (reference: MultiScaleMaskedLoss, gans/inversion.py:32-76)
# ---------------------------------------------------------------------------------------
class MsmlTarget:
    """The target side of the loss for one (ref, mask): levels of ref / mask / norm and 1 / (sum(mask_i) + 1e-8),
    built by ONE launch (dgv2_msml_prepare) and reused by every forward / backward on that target."""

    def __init__(self, ref, mask, levels):
        B, C, H, W = ref.shape
        if tuple(mask.shape) != (B, 1, H, W):
            raise ValueError(f"msml: mask must be [B,1,H,W] = {(B, 1, H, W)}, got {tuple(mask.shape)}")
        ref = ref.detach().float().contiguous()
        mask = mask.detach().float().contiguous()
        N.check(ref, mask)
        self.shape, self.levels = (B, C, H, W), int(levels)
        px = 0
        for _ in range(self.levels):
            px += H * W
            H, W = (H + 1) // 2, (W + 1) // 2
        self.pixels = px   # per sample and channel, all levels
        dev = ref.device
        self.refp = torch.empty(B * C * px, device=dev, dtype=torch.float32)
        self.maskp = torch.empty(B * px, device=dev, dtype=torch.float32)
        self.normp = torch.empty(B * px, device=dev, dtype=torch.float32)
        self.invm = torch.empty(self.levels * B, device=dev, dtype=torch.float32)
        B, C, H, W = self.shape
        N.call("dgv2_msml_prepare", N.ptr(self.refp), N.ptr(self.maskp), N.ptr(self.normp), N.ptr(self.invm), N.ptr(ref),
               N.ptr(mask), B, C, H, W, self.levels, N.stream())

    def upper(self):
        """Element count of levels 1 .. L-1 of a [B,C,.,.] pyramid."""
        B, C, H, W = self.shape
        return B * C * (self.pixels - H * W)


class _MsmlLoss(Function):
    @staticmethod
    def forward(ctx, gen, target, metric, relative):
        B, C, H, W = target.shape
        if tuple(gen.shape) != target.shape:
            raise ValueError(f"msml_loss: gen {tuple(gen.shape)} does not match the prepared target {target.shape}")
        gen = gen.detach().float().contiguous()
        N.check(gen)
        loss = torch.empty(B, device=gen.device, dtype=torch.float32)
        genp = torch.empty(target.upper(), device=gen.device, dtype=torch.float32) if target.levels > 1 else None
        N.call("dgv2_msml_fwd", N.ptr(loss), N.ptr(genp), N.ptr(gen), N.ptr(target.refp), N.ptr(target.maskp),
               N.ptr(target.normp), N.ptr(target.invm), B, C, H, W, target.levels, metric, int(relative), N.stream())
        ctx.cfg = (target, metric, relative, gen, genp)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        target, metric, relative, gen, genp = ctx.cfg
        B, C, H, W = target.shape
        gloss = gloss.float().contiguous()
        ggen = torch.empty_like(gen)
        gp = torch.empty_like(genp) if genp is not None else None
        N.check(gloss)
        N.call("dgv2_msml_bwd", N.ptr(ggen), N.ptr(gp), N.ptr(gloss), N.ptr(gen), N.ptr(genp), N.ptr(target.refp),
               N.ptr(target.maskp), N.ptr(target.normp), N.ptr(target.invm), B, C, H, W, target.levels, metric,
               int(relative), N.stream())
        return ggen, None, None, None


def msml_prepare(ref, mask, levels):
    return MsmlTarget(ref, mask, levels)


def msml_loss(gen, prepared, metric="l1", relative=True):
    """loss [B] of `gen` [B,C,H,W] against a prepared target: one launch forward, one backward; only gen gets a
    gradient (first order)."""
    return _MsmlLoss.apply(gen, prepared, _METRICS[metric], bool(relative))


# ---------------------------------------------------------------------------------------
# range conversion, plain and with an input gradient (reference: CoordBridge.convert and autograd through it, gans/coords.py:88-185)
# ---------------------------------------------------------------------------------------
def coords_convert(x, mode, min_depth, max_depth, angle=None, mask=None, raydrop_const=-1.0, out=None):
    B, _, H, W = x.shape
    x = x.contiguous().float()
    N.check(x, angle, mask, out)
    shape = (B, 3 if mode >= 2 else 1, H, W)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"coords_convert: out must be a contiguous fp32 {shape} tensor")
    N.call("dgv2_coords_convert", N.ptr(out), N.ptr(x), N.ptr(mask), N.ptr(angle), B, H, W, float(min_depth),
           float(max_depth), float(raydrop_const), mode, N.stream())
    return out


class _CoordsConvert(Function):
    @staticmethod
    def forward(ctx, x, mode, min_depth, max_depth, angle, mask, raydrop_const):
        x = x.detach().contiguous().float()
        ctx.cfg = (x, mode, min_depth, max_depth, angle, mask)
        return coords_convert(x, mode, min_depth, max_depth, angle, mask, raydrop_const)

    @staticmethod
    def backward(ctx, g):
        x, mode, min_depth, max_depth, angle, mask = ctx.cfg
        B, _, H, W = x.shape
        g = g.contiguous().float()
        gx = torch.empty_like(x)
        N.check(g, x, mask, angle)
        N.call("dgv2_coords_convert_bwd", N.ptr(gx), N.ptr(g), N.ptr(x), N.ptr(mask), N.ptr(angle), B, H, W,
               float(min_depth), float(max_depth), mode, N.stream())
        return gx, None, None, None, None, None, None


def coords_convert_diff(x, mode, min_depth, max_depth, angle=None, mask=None, raydrop_const=-1.0):
    """native.coords_convert as an autograd node (first order; the gradient goes to x alone)."""
    return _CoordsConvert.apply(x, mode, min_depth, max_depth, angle, mask, raydrop_const)


__all__ = ["MsmlTarget", "msml_prepare", "msml_loss", "coords_convert", "coords_convert_diff"]
