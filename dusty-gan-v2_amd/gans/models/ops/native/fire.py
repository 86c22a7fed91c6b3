"""native.fire: the evaluation-mode Fire module of the SqueezeSeg trunks (reference: semseg/models/squeezeseg_v2.py:39-56,
squeezeseg_v1.py:8-24, with the decoder's residual adds of squeezeseg_v2.py:169-172) as one launch of dgv2_fire_fwd
(include/dgv2.h states the arithmetic, DESIGN.md section 31 the kernel).

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI, see the package docstring).  Forward only: the
modules of semseg.models call this under eval() with grad mode off and run the composition of library ops otherwise.
Nothing is cached between calls: the launch reads the parameter and buffer tensors it is handed.
"""
import torch

import dgv2_native as N

FIRE_CIN_MAX, FIRE_CS_MAX, FIRE_E_MAX = 512, 64, 256
_FIRE_DTYPES = {torch.float32: N.F32, torch.bfloat16: N.BF16, torch.float16: N.F16}


def fire_supported(in_ch, s1x1, e1x1, e3x3, dtype=torch.float32):
    """Whether dgv2_fire_fwd covers a Fire(in_ch, s1x1, e1x1, e3x3) on activations of `dtype`: channel counts in
    multiples of 16, in_ch <= 512, s1x1 <= 64, e1x1, e3x3 <= 256; float32, bfloat16 or float16."""
    chans = ((in_ch, FIRE_CIN_MAX), (s1x1, FIRE_CS_MAX), (e1x1, FIRE_E_MAX), (e3x3, FIRE_E_MAX))
    return dtype in _FIRE_DTYPES and all(isinstance(c, int) and 16 <= c <= top and c % 16 == 0 for c, top in chans)


def _param(name, t, shape):
    if t is None or tuple(t.shape) != tuple(shape):
        raise ValueError(f"fire_forward: {name} must have shape {tuple(shape)}, got {None if t is None else tuple(t.shape)}")
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t    # the kernel reads the weights with 16-byte loads


def _norm(name, bn, ch):
    """None, or (weight, bias, running_mean, running_var, eps) -> four float32 [ch] tensors (or Nones) and eps."""
    if bn is None:
        return None, None, None, None, 0.0
    if len(bn) != 5 or any(t is None for t in bn[:4]):
        raise ValueError(f"fire_forward: {name} must be None or (weight, bias, running_mean, running_var, eps)")
    eps = float(bn[4])
    if not eps >= 0.0:
        raise ValueError(f"fire_forward: {name} eps must be >= 0, got {eps}")
    return tuple(_param(f"{name}[{i}]", t, (ch,)) for i, t in enumerate(bn[:4])) + (eps,)


def fire_forward(x, w_s, b_s, bn_s, w_d, b_d, w_1, b_1, bn_1, w_3, b_3, bn_3, skip=None):
    """x [B,Cin,H,W] (float32 / bfloat16 / float16, CUDA) -> cat(e1, e3) [+ skip], [B,E1+E3,H,Wout] in x's dtype.
    w_s [Cs,Cin,1,1], w_1 [E1,Cs,1,1], w_3 [E3,Cs,3,3] and their biases are the three convs; w_d [Cs,Cs,1,4], b_d the
    ConvTranspose2d of an up-sampling Fire (Wout = 2 W) or both None (Wout = W); bn_* is None (ConvReLU) or the tuple
    (weight, bias, running_mean, running_var, eps) of the BatchNorm2d after that conv's ReLU.  Parameters are read as
    float32.  skip: None or a tensor of the output's shape and dtype, added after the concatenation.
    ValueError outside fire_supported's range or for mismatched shapes; RuntimeError for CPU tensors.  One launch."""
    if x.ndim != 4:
        raise ValueError(f"fire_forward: x must be [B,Cin,H,W], got {tuple(x.shape)}")
    B, Cin, H, W = x.shape
    if w_s.ndim != 4 or w_1.ndim != 4 or w_3.ndim != 4:
        raise ValueError("fire_forward: conv weights must be 4-d")
    Cs, E1, E3 = w_s.shape[0], w_1.shape[0], w_3.shape[0]
    if not fire_supported(Cin, Cs, E1, E3, x.dtype):
        raise ValueError(f"fire_forward: Fire({Cin}, {Cs}, {E1}, {E3}) on {x.dtype} is outside the kernel's range "
                         f"(multiples of 16; in_ch <= {FIRE_CIN_MAX}, s1x1 <= {FIRE_CS_MAX}, e <= {FIRE_E_MAX}; "
                         "float32 / bfloat16 / float16)")
    if min(B, H, W) < 1:
        raise ValueError(f"fire_forward: empty input {tuple(x.shape)}")
    up = w_d is not None
    if up != (b_d is not None):
        raise ValueError("fire_forward: w_d and b_d come together")
    Wout = 2 * W if up else W
    w_s, b_s = _param("w_s", w_s, (Cs, Cin, 1, 1)), _param("b_s", b_s, (Cs,))
    w_1, b_1 = _param("w_1", w_1, (E1, Cs, 1, 1)), _param("b_1", b_1, (E1,))
    w_3, b_3 = _param("w_3", w_3, (E3, Cs, 3, 3)), _param("b_3", b_3, (E3,))
    if up:
        w_d, b_d = _param("w_d", w_d, (Cs, Cs, 1, 4)), _param("b_d", b_d, (Cs,))
    ns, n1, n3 = _norm("bn_s", bn_s, Cs), _norm("bn_1", bn_1, E1), _norm("bn_3", bn_3, E3)
    if skip is not None:
        if tuple(skip.shape) != (B, E1 + E3, H, Wout) or skip.dtype != x.dtype:
            raise ValueError(f"fire_forward: skip must be {x.dtype} {(B, E1 + E3, H, Wout)}, got {skip.dtype} {tuple(skip.shape)}")
        skip = skip.detach().contiguous()
    x = x.detach().contiguous()
    N.check(x, skip, w_s, b_s, w_d, b_d, w_1, b_1, w_3, b_3, *ns[:4], *n1[:4], *n3[:4])
    y = torch.empty((B, E1 + E3, H, Wout), device=x.device, dtype=x.dtype)
    fire_forward_into(y, x, skip, w_s, b_s, ns, w_d, b_d, w_1, b_1, n1, w_3, b_3, n3)
    return y


def fire_forward_into(y, x, skip, w_s, b_s, ns, w_d, b_d, w_1, b_1, n1, w_3, b_3, n3):
    """The launch itself on prepared operands (contiguous, float32 parameters, ns / n1 / n3 five-tuples as _norm
    returns): writes y, which may be a view into a larger buffer.  RuntimeError on a non-zero return code."""
    B, Cin, H, W = x.shape
    N.call("dgv2_fire_fwd", N.ptr(y), N.ptr(x), N.ptr(skip),
           N.ptr(w_s), N.ptr(b_s), N.ptr(ns[0]), N.ptr(ns[1]), N.ptr(ns[2]), N.ptr(ns[3]), N.ptr(w_d), N.ptr(b_d),
           N.ptr(w_1), N.ptr(b_1), N.ptr(n1[0]), N.ptr(n1[1]), N.ptr(n1[2]), N.ptr(n1[3]),
           N.ptr(w_3), N.ptr(b_3), N.ptr(n3[0]), N.ptr(n3[1]), N.ptr(n3[2]), N.ptr(n3[3]),
           ns[4], n1[4], n3[4], B, Cin, w_s.shape[0], w_1.shape[0], w_3.shape[0], H, W, int(w_d is not None),
           _FIRE_DTYPES[x.dtype], N.stream())


__all__ = ["fire_forward", "fire_forward_into", "fire_supported", "FIRE_CIN_MAX", "FIRE_CS_MAX", "FIRE_E_MAX"]
