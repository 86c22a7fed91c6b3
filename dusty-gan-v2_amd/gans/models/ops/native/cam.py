"""native.cam: the evaluation-mode context-aggregation module of SqueezeSegV2 (reference:
semseg/models/squeezeseg_v2.py:20-36) as one launch of dgv2_cam_fwd (include/dgv2.h states the arithmetic, DESIGN.md
section 35 the kernel).

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI, see the package docstring).  Forward only: the CAM
of semseg.models calls this under eval() with grad mode off and runs the composition of library ops otherwise.
Nothing is cached between calls: the launch reads the parameter tensors it is handed.
"""
import torch

import dgv2_native as N

CAM_C_MAX, CAM_CR_MAX = 128, 8
CAM_SAMPLE_MAX = 2 ** 31 - 1   # C * H * W of one sample: the kernel's offsets inside a sample are 32-bit
_CAM_DTYPES = {torch.float32: N.F32, torch.bfloat16: N.BF16, torch.float16: N.F16}


def cam_supported(C, Cr, dtype=torch.float32):
    """Whether dgv2_cam_fwd covers a CAM with C channels squeezed to Cr on activations of `dtype`: C a multiple of 16
    in [16, 128], 1 <= Cr <= 8; float32, bfloat16 or float16."""
    return (dtype in _CAM_DTYPES and isinstance(C, int) and isinstance(Cr, int)
            and 16 <= C <= CAM_C_MAX and C % 16 == 0 and 1 <= Cr <= CAM_CR_MAX)


def _param(name, t, shape):
    if t is None or tuple(t.shape) != tuple(shape):
        raise ValueError(f"cam_forward: {name} must have shape {tuple(shape)}, got {None if t is None else tuple(t.shape)}")
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def cam_forward(x, w1, b1, w2, b2):
    """x [B,C,H,W] (float32 / bfloat16 / float16, CUDA) -> x * sigmoid(W2 relu(W1 maxpool7x7(x) + b1) + b2) in x's
    dtype.  w1 [Cr,C,1,1], b1 [Cr], w2 [C,Cr,1,1], b2 [C] are the two 1x1 convs, read as float32.
    ValueError outside cam_supported's range, for mismatched shapes, an empty input or a sample of more than 2^31 - 1
    elements; RuntimeError for CPU tensors.  One launch."""
    if x.ndim != 4:
        raise ValueError(f"cam_forward: x must be [B,C,H,W], got {tuple(x.shape)}")
    B, C, H, W = x.shape
    if w1 is None or w1.ndim != 4:
        raise ValueError("cam_forward: w1 must be [Cr,C,1,1]")
    Cr = w1.shape[0]
    if not cam_supported(C, Cr, x.dtype):
        raise ValueError(f"cam_forward: CAM({C} -> {Cr}) on {x.dtype} is outside the kernel's range (C a multiple of 16 up "
                         f"to {CAM_C_MAX}, Cr <= {CAM_CR_MAX}; float32 / bfloat16 / float16)")
    if min(B, H, W) < 1:
        raise ValueError(f"cam_forward: empty input {tuple(x.shape)}")
    if C * H * W > CAM_SAMPLE_MAX:
        raise ValueError(f"cam_forward: a sample of {C * H * W} elements does not fit the kernel's 32-bit offsets "
                         f"(at most {CAM_SAMPLE_MAX})")
    w1, b1 = _param("w1", w1, (Cr, C, 1, 1)), _param("b1", b1, (Cr,))
    w2, b2 = _param("w2", w2, (C, Cr, 1, 1)), _param("b2", b2, (C,))
    x = x.detach().contiguous()
    N.check(x, w1, b1, w2, b2)
    y = torch.empty_like(x)
    N.call("dgv2_cam_fwd", N.ptr(y), N.ptr(x), N.ptr(w1), N.ptr(b1), N.ptr(w2), N.ptr(b2), B, C, Cr, H, W,
           _CAM_DTYPES[x.dtype], N.stream())
    return y


__all__ = ["cam_forward", "cam_supported", "CAM_C_MAX", "CAM_CR_MAX", "CAM_SAMPLE_MAX"]
