"""The cases of tests/test_gpu_conv_direct.py, shared with tests/golden/make_conv_direct_golden.py: the smallest shapes
that reach each route of the direct conv engine (csrc/conv_direct.hip) through the Python call sites that exist on both
sides of ABI 59 -- native._conv_fwd_raw, _conv_dgrad_raw, _conv_dgrad_direct, _conv_fwd_fp8.

A case is (name, kind, B, H, W, C, O, k, stride, dtype, opts): (H, W) the conv's INPUT size, C -> O its channels; a data
gradient maps gy [B,Ho,Wo,O] back to gx [B,H,W,C].  run() returns the device outputs of a case (a data gradient: without
and with the residual) and, for integer operands, what the float64 ring conv (helpers.conv_oracle) and its autograd give.
"""
import hashlib

import torch

from helpers import conv_oracle

DEV = "cuda"
FP8 = torch.float8_e4m3fn
BF16, F32 = torch.bfloat16, torch.float32

CASES = [
    # name                  kind     B   H    W    C    O  k  s  dtype  opts                                  route
    ("fwd_strip_act",      "fwd",    2, 16,  32,  32,  32, 3, 1, BF16, dict(bias=True, act=True)),          # strip kernel
    ("fwd_strip_bare",     "fwd",    2, 16,  32,  32,  32, 3, 1, BF16, dict()),
    ("fwd_s1_resid",       "fwd",    2,  8,  32,  64,  64, 3, 1, BF16, dict(resid=True)),                   # conv8 / pipe F33=1
    ("fwd_pairs",          "fwd",   16,  4, 256,  32, 512, 3, 1, BF16, dict()),                             # image pairs (hper)
    ("fwd_s2",             "fwd",    2, 16,  64,  32,  64, 3, 2, BF16, dict()),                             # pipe F33=3
    ("fwd_1x1_bias",       "fwd",    2,  8,  32,  32,  64, 1, 1, BF16, dict(bias=True)),                    # pipe generic
    ("fwd_f32",            "fwd",    2,  8,  32,  16,  16, 3, 1, F32,  dict()),                             # fp32 MFMA, TO=16
    ("fwd_w8",             "fwd",    2,  8,   8,  32,  32, 3, 1, BF16, dict()),                             # wrap refused: sync kernel
    ("fp8_s1",             "fp8",    2,  8,  32,  64,  64, 3, 1, BF16, dict(bias=True, act=True)),
    ("fp8_s2",             "fp8",    2,  8,  32,  64,  64, 3, 2, BF16, dict(resid=True)),
    ("dgrad_strip",        "dgrad",  2, 16,  32,  32,  32, 3, 1, BF16, dict()),                             # strip with border
    ("dgrad_s1_bf16",      "dgrad",  2,  8,  32,  64,  64, 3, 1, BF16, dict()),                             # pipe F33=2, border
    ("dgrad_s1_bf16_h2",   "dgrad",  2,  2,  32,  64,  64, 3, 1, BF16, dict()),
    ("dgrad_s1_f32",       "dgrad",  2,  8,  32,  64,  64, 3, 1, F32,  dict()),
    ("dgrad_s1_f32_h2",    "dgrad",  2,  2,  32,  64,  64, 3, 1, F32,  dict()),
    ("dgrad_split",        "dgrad",  3,  4,  32, 144,  64, 3, 1, BF16, dict()),                             # channel ranges 128 + 16
    ("dgrad_w8",           "dgrad",  2,  8,   8,  32,  32, 3, 1, BF16, dict(direct=True)),                  # fused refused: 3 launches
    ("dgrad_s2",           "dgrad",  2, 16,  64,  32,  64, 3, 2, BF16, dict()),                             # four classes, s2d
    ("dgrad_s2_w16",       "dgrad",  2, 16,  16,  32,  64, 3, 2, BF16, dict(direct=True)),                  # fused refused: 4 + 2
    ("dgrad_1x1_f32",      "dgrad",  2,  8,  32,  16,  16, 1, 1, F32,  dict()),                             # single tap, hzero
]
IDS = [c[0] for c in CASES]
ALPHA, GAIN = 0.25, 0.5      # leaky ReLU slope and gain: powers of two, exact on integers


def _draw(gen, shape, exact, lo=-2, hi=2, std=1.0):
    if exact:
        return torch.randint(lo, hi + 1, shape, generator=gen).float()
    return torch.randn(shape, generator=gen) * std


def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


def run(nat, case, exact):
    """-> (outputs on the device, float64 CPU references [B,H,W,C] or None when not `exact`)."""
    name, kind, B, H, W, C, O, k, stride, dtype, opts = case
    gen = torch.Generator().manual_seed(1000 + IDS.index(name))
    geom = nat.ConvGeom(k, k, stride, k // 2, True)
    Ho, Wo = geom.out_hw(H, W)
    x = _draw(gen, (B, H, W, C), exact)
    w = _draw(gen, (O, k, k, C), exact, std=0.125)
    bias = _draw(gen, (O,), exact, -3, 3) if opts.get("bias") else None
    dev = lambda t: None if t is None else t.to(DEV, dtype)
    act = (3, ALPHA, GAIN) if opts.get("act") else (0, 0.2, 1.0)
    if kind in ("fwd", "fp8"):
        resid = _draw(gen, (B, Ho, Wo, O), exact, -3, 3) if opts.get("resid") else None
        bdev = None if bias is None else bias.to(DEV)
        if kind == "fwd":
            got = nat._conv_fwd_raw(dev(x), dev(w), geom, bdev, *act, dev(resid))
        else:
            (w8, descale), = nat.fp8_quant_weights([(w.permute(0, 3, 1, 2).contiguous().to(DEV), 1.0)])
            got = nat._conv_fwd_fp8(x.to(DEV).to(FP8), w8, descale, geom, bdev, *act, dev(resid))
        if not exact:
            return [got], None
        want = conv_oracle(_nchw(x), _nchw(w), stride, k // 2, True).permute(0, 2, 3, 1)
        if resid is not None:
            want = want + resid.double()
        if bias is not None:
            want = want + bias.double()
        if opts.get("act"):
            want = torch.where(want > 0, want, want * ALPHA) * GAIN
        return [got], [want]
    gy = _draw(gen, (B, Ho, Wo, O), exact)
    resid = _draw(gen, (B, H, W, C), exact, -3, 3)
    xshape = (B, H, W, C)
    if opts.get("direct"):
        wt3 = dev(w).permute(3, 1, 2, 0).contiguous().reshape(C, k * k, O)
        call = lambda r: nat._conv_dgrad_direct(dev(gy), wt3, geom, xshape, r)
    else:
        call = lambda r: nat._conv_dgrad_raw(dev(gy), dev(w), geom, xshape, resid=r)
    got = [call(None), call(dev(resid))]
    if not exact:
        return got, None
    xz = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad(conv_oracle(xz, _nchw(w), stride, k // 2, True), [xz], _nchw(gy))
    gx = gx.permute(0, 2, 3, 1)
    return got, [gx, gx + resid.double()]


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
