"""Building blocks of the SqueezeSeg trunks (reference: semseg/models/common.py): weight initialisers, the conv /
norm / activation sequences whose state-dict layout the published checkpoints fix, and the routing of an
evaluation-mode Fire module and of an evaluation-mode context-aggregation module onto their one-launch native kernels
(gans.models.ops.native.fire; gans.models.ops.native.cam, section 35).
"""
import torch
from torch import nn

from gans.models.ops.native import cam as _cam
from gans.models.ops.native import fire as _fire

# False forces the composition of library ops in every Fire module (tests, A/B timing); read at every call
FIRE_NATIVE = True
# the same switch for the context-aggregation modules; DESIGN.md section 35 has the measurement behind its default
CAM_NATIVE = True

_INPUT_CHANNELS = {"xyz": 3, "depth": 1, "reflectance": 1, "mask": 1}


def _init_conv_or_linear(module, fill):
    if isinstance(module, (nn.Conv2d, nn.Linear)):
        fill(module.weight)
        if getattr(module, "bias", None) is not None:
            nn.init.zeros_(module.bias)


def init_weights_trunc_normal(module, std=0.001):
    """Truncated-normal weights, zero biases, on Conv2d and Linear; other modules are left alone."""
    _init_conv_or_linear(module, lambda w: nn.init.trunc_normal_(w, std=std))


def init_weights_xavier(module):
    """Xavier-uniform weights, zero biases, on Conv2d and Linear; other modules are left alone."""
    _init_conv_or_linear(module, nn.init.xavier_uniform_)


def init_weights_bilinear(module):
    """A (1, 4) ConvTranspose2d with as many outputs as inputs becomes a per-channel bilinear x2 up-sampler along
    the width: [1, 3, 3, 1] / 4 on the diagonal, zero elsewhere, zero bias."""
    assert isinstance(module, nn.ConvTranspose2d)
    assert tuple(module.kernel_size) == (1, 4)
    assert module.in_channels == module.out_channels
    taps = torch.tensor([1.0, 3.0, 3.0, 1.0])
    taps = taps / taps.sum() * 2
    with torch.no_grad():
        module.weight.zero_()
        module.bias.zero_()
        idx = torch.arange(module.in_channels)
        module.weight[idx, idx, 0] = taps.to(module.weight)


def setup_in_ch(inputs):
    """Number of image channels of a list of modality names."""
    return sum(_INPUT_CHANNELS[name] for name in inputs)


class ConvNorm(nn.Sequential):
    def __init__(self, in_ch, out_ch, kernel_size, stride, padding, bn_momentum):
        super().__init__(nn.Conv2d(in_ch, out_ch, kernel_size, stride, padding, bias=False),
                         nn.BatchNorm2d(out_ch, momentum=bn_momentum))


class ConvReLU(nn.Sequential):
    def __init__(self, in_ch, out_ch, kernel_size, stride, padding):
        super().__init__(nn.Conv2d(in_ch, out_ch, kernel_size, stride, padding, bias=True), nn.ReLU(inplace=True))


class ConvNormReLU(nn.Sequential):
    def __init__(self, in_ch, out_ch, kernel_size, stride, padding, bn_momentum):
        super().__init__(nn.Conv2d(in_ch, out_ch, kernel_size, stride, padding, bias=False),
                         nn.BatchNorm2d(out_ch, momentum=bn_momentum), nn.ReLU(inplace=True))


class ConvReLUNorm(nn.Sequential):
    def __init__(self, in_ch, out_ch, kernel_size, stride, padding, bn_momentum):
        super().__init__(nn.Conv2d(in_ch, out_ch, kernel_size, stride, padding, bias=True), nn.ReLU(inplace=True),
                         nn.BatchNorm2d(out_ch, momentum=bn_momentum))


class ConvNormLReLU(nn.Sequential):
    def __init__(self, in_ch, out_ch, kernel_size, stride, padding, bn_momentum):
        super().__init__(nn.Conv2d(in_ch, out_ch, kernel_size, stride, padding, bias=False),
                         nn.BatchNorm2d(out_ch, momentum=bn_momentum), nn.LeakyReLU(0.1, inplace=True))


class DeconvReLU(nn.Sequential):
    """Transposed conv, ReLU.  With init_method "bilinear" the weights start as the bilinear up-sampler and apply()
    is a no-op on this module, so that a model-wide model.apply(init) leaves them in place."""

    def __init__(self, in_ch, out_ch, kernel_size, stride, padding, init_method="bilinear"):
        super().__init__(nn.ConvTranspose2d(in_ch, out_ch, kernel_size, stride, padding), nn.ReLU(inplace=True))
        self.init_method = init_method
        if init_method == "bilinear":
            init_weights_bilinear(self[0])

    def apply(self, fn):
        if self.init_method == "bilinear":
            return self
        return super().apply(fn)


class Head(nn.Sequential):
    """Channel dropout (the identity in evaluation), then the classifier conv."""

    def __init__(self, in_ch, out_ch, kernel_size, dropout_p):
        super().__init__(nn.Dropout2d(p=dropout_p), nn.Conv2d(in_ch, out_ch, kernel_size, 1, kernel_size // 2))


def _conv_and_norm(seq):
    """(conv, None) of a ConvReLU or (conv, bn tuple) of a ConvReLUNorm, read from the module as it is NOW."""
    conv = seq[0]
    bn = seq[2] if len(seq) > 2 else None
    if bn is None:
        return conv, None
    return conv, (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)


def fire_uses_native(fire, x):
    """The routing rule of both Fire classes: a CUDA input, eval(), grad mode off, the switch on, and a configuration
    the kernel covers (DESIGN.md section 31 lists which those are and what was measured)."""
    if not (FIRE_NATIVE and x.is_cuda and not fire.training and not torch.is_grad_enabled()):
        return False
    sq, e1, e3 = fire.squeeze1x1[0], fire.expand1x1[0], fire.expand3x3[0]
    for seq in (fire.squeeze1x1, fire.expand1x1, fire.expand3x3):
        bn = seq[2] if len(seq) > 2 else None
        if bn is not None and (bn.running_mean is None or bn.weight is None):
            return False
    return x.ndim == 4 and _fire.fire_supported(sq.in_channels, sq.out_channels, e1.out_channels, e3.out_channels, x.dtype)


def fire_native(fire, x, skip=None):
    """One native launch for a Fire module (either class): squeeze, optional up-sampling, both expands, the
    concatenation and the optional residual add.  Reads the module's current parameters and buffers."""
    sq, ns = _conv_and_norm(fire.squeeze1x1)
    e1, n1 = _conv_and_norm(fire.expand1x1)
    e3, n3 = _conv_and_norm(fire.expand3x3)
    up = fire.upsample[0] if fire.upsample is not None else None
    return _fire.fire_forward(x, sq.weight, sq.bias, ns, None if up is None else up.weight,
                              None if up is None else up.bias, e1.weight, e1.bias, n1, e3.weight, e3.bias, n3, skip=skip)


def fire_composition(fire, x, skip=None):
    """The same module as library tensor ops, differentiable: the training path and the native path's yardstick."""
    h = fire.squeeze1x1(x)
    if fire.upsample is not None:
        h = fire.upsample(h)
    y = torch.cat((fire.expand1x1(h), fire.expand3x3(h)), dim=1)
    return y if skip is None else y + skip


def fire_forward(fire, x, skip=None):
    if fire_uses_native(fire, x):
        return fire_native(fire, x, skip)
    return fire_composition(fire, x, skip)


def cam_uses_native(cam, x):
    """The routing rule of the context-aggregation module, Fire's rule: a CUDA input, eval(), grad mode off, the
    switch on, and a configuration the kernel covers."""
    if not (CAM_NATIVE and x.is_cuda and not cam.training and not torch.is_grad_enabled()):
        return False
    squeeze, excite = cam.attn[1], cam.attn[3]
    if squeeze.bias is None or excite.bias is None:
        return False
    return x.ndim == 4 and _cam.cam_supported(squeeze.in_channels, squeeze.out_channels, x.dtype)


def cam_native(cam, x):
    """One native launch for a context-aggregation module.  Reads the module's current parameters."""
    squeeze, excite = cam.attn[1], cam.attn[3]
    return _cam.cam_forward(x, squeeze.weight, squeeze.bias, excite.weight, excite.bias)


def cam_composition(cam, x):
    """The same module as library tensor ops, differentiable: the training path and the native path's yardstick."""
    return x * cam.attn(x)


def cam_forward(cam, x):
    if cam_uses_native(cam, x):
        return cam_native(cam, x)
    return cam_composition(cam, x)
