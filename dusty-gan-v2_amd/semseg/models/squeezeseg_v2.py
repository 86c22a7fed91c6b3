"""SqueezeSegV2 trunk for range images (reference: semseg/models/squeezeseg_v2.py): V1's layout with a batch norm
after every ReLU and three context-aggregation modules in the encoder.  Module tree and state-dict layout are the
reference's, so a published checkpoint's ckpt["model"] loads with strict=True; in eval() with grad mode off every
Fire module and every context-aggregation module is one native launch.  The SqueezeNet initialisation is read from a local file only."""
from functools import partial
from pathlib import Path

import joblib
import torch
from torch import nn

from .common import (ConvReLUNorm, DeconvReLU, Head, cam_forward, fire_forward, init_weights_trunc_normal,
                     init_weights_xavier, setup_in_ch)
from .crf_as_rnn import CRFRNN

# encoder Fire modules -> their names in the SqueezeNet v1.1 pickle
_SQUEEZENET_NAMES = {"fire_2_3.1": "fire2", "fire_2_3.3": "fire3", "fire_4_5.1": "fire4", "fire_4_5.2": "fire5",
                     "fire_6_9.1": "fire6", "fire_6_9.2": "fire7", "fire_6_9.3": "fire8", "fire_6_9.4": "fire9"}
SQUEEZENET_FILE = Path(__file__).parent / "pretrained" / "squeezenet_v1.1.pkl"


class CAM(nn.Module):
    """Context aggregation module: the input gated by a squeeze-and-excite map of its 7x7 max-pool.  In eval() with
    grad mode off it is one native launch (common.cam_forward has the rule)."""

    def __init__(self, ch, reduction=16):
        super().__init__()
        self.attn = nn.Sequential(nn.MaxPool2d(7, 1, 3), nn.Conv2d(ch, ch // reduction, 1, 1, 0), nn.ReLU(inplace=True),
                                  nn.Conv2d(ch // reduction, ch, 1, 1, 0), nn.Sigmoid())

    def forward(self, x):
        return cam_forward(self, x)


class Fire(nn.Module):
    """Squeeze 1x1, optional x2 transposed conv along the width, then 1x1 and 3x3 expands side by side, each conv
    followed by ReLU and batch norm.  forward(x, skip) also adds `skip` to the output (the decoder's residual)."""

    def __init__(self, in_ch, s1x1, e1x1, e3x3, bn_momentum, up=False):
        super().__init__()
        self.squeeze1x1 = ConvReLUNorm(in_ch, s1x1, 1, 1, 0, bn_momentum)
        self.upsample = DeconvReLU(s1x1, s1x1, (1, 4), (1, 2), (0, 1)) if up else None
        self.expand1x1 = ConvReLUNorm(s1x1, e1x1, 1, 1, 0, bn_momentum)
        self.expand3x3 = ConvReLUNorm(s1x1, e3x3, 3, 1, 1, bn_momentum)

    def forward(self, x, skip=None):
        return fire_forward(self, x, skip)


def load_squeezenet(encoder, path):
    """Copy the SqueezeNet v1.1 conv weights and biases of the joblib pickle at `path` into the encoder's Fires."""
    table = joblib.load(path)
    with torch.no_grad():
        for name, module in encoder.named_modules():
            if not isinstance(module, Fire):
                continue
            for layer in ("squeeze1x1", "expand1x1", "expand3x3"):
                weight, bias = table[f"{_SQUEEZENET_NAMES[name]}/{layer}"]
                conv = getattr(module, layer)[0]
                conv.weight.copy_(torch.as_tensor(weight))
                conv.bias.copy_(torch.as_tensor(bias))


class SqueezeSegV2(nn.Module):
    """pretrained_weights: False / None skips the SqueezeNet initialisation, a path loads that pickle, True loads
    SQUEEZENET_FILE beside this module and raises FileNotFoundError where it is missing.  No file is fetched from anywhere."""

    def __init__(self, inputs, num_classes, bn_momentum=0.001, head_dropout_p=0.5, use_crf=False,
                 crf_kernel_size=(3, 5), crf_init_weight_smoothness=0.02, crf_init_weight_appearance=0.1,
                 crf_theta_gamma=0.9, crf_theta_alpha=0.9, crf_theta_beta=0.015, crf_num_iters=3,
                 pretrained_weights=True):
        super().__init__()
        in_ch = setup_in_ch(inputs)
        mom = bn_momentum

        def pool():
            return nn.MaxPool2d(3, (1, 2), 1)

        self.encoder = nn.ModuleDict({
            "conv_1a": nn.Sequential(ConvReLUNorm(in_ch, 64, 3, (1, 2), 1, mom), CAM(64)),
            "conv_1b": ConvReLUNorm(in_ch, 64, 1, 1, 0, mom),
            "fire_2_3": nn.Sequential(pool(), Fire(64, 16, 64, 64, mom), CAM(128), Fire(128, 16, 64, 64, mom), CAM(128)),
            "fire_4_5": nn.Sequential(pool(), Fire(128, 32, 128, 128, mom), Fire(256, 32, 128, 128, mom)),
            "fire_6_9": nn.Sequential(pool(), Fire(256, 48, 192, 192, mom), Fire(384, 48, 192, 192, mom),
                                      Fire(384, 64, 256, 256, mom), Fire(512, 64, 256, 256, mom)),
        })
        self.decoder = nn.ModuleDict({
            "fire_10": Fire(512, 64, 128, 128, mom, up=True),
            "fire_11": Fire(256, 32, 64, 64, mom, up=True),
            "fire_12": Fire(128, 16, 32, 32, mom, up=True),
            "fire_13": Fire(64, 16, 32, 32, mom, up=True),
            "head": Head(64, num_classes, 3, head_dropout_p),
        })
        self.crf = None
        if use_crf:
            self.crf = CRFRNN(num_classes=num_classes, kernel_size=crf_kernel_size,
                              init_weight_smoothness=crf_init_weight_smoothness,
                              init_weight_appearance=crf_init_weight_appearance, theta_gamma=crf_theta_gamma,
                              theta_alpha=crf_theta_alpha, theta_beta=crf_theta_beta, num_iters=crf_num_iters)

        self.encoder.apply(partial(init_weights_trunc_normal, std=0.001))
        for module in self.encoder.modules():
            if isinstance(module, CAM):
                module.apply(init_weights_xavier)
        if pretrained_weights:
            path = SQUEEZENET_FILE if pretrained_weights is True else Path(pretrained_weights)
            if not path.is_file():
                raise FileNotFoundError(f"SqueezeNet v1.1 weights not found at {path}: place squeezenet_v1.1.pkl there, "
                                        "pass its path, or pass pretrained_weights=False")
            load_squeezenet(self.encoder, path)
        self.decoder.apply(partial(init_weights_trunc_normal, std=0.1))

    def forward(self, img, xyz=None, mask=None):
        """img [B,C,H,W] with W a multiple of 16 -> logits [B,num_classes,H,W]; xyz and mask feed the CRF."""
        enc, dec = self.encoder, self.decoder
        h_1b = enc["conv_1b"](img)
        h_1a = enc["conv_1a"](img)
        h_3 = enc["fire_2_3"](h_1a)
        h_5 = enc["fire_4_5"](h_3)
        h = enc["fire_6_9"](h_5)
        h = dec["fire_10"](h, h_5)
        h = dec["fire_11"](h, h_3)
        h = dec["fire_12"](h, h_1a)
        h = dec["fire_13"](h, h_1b)
        logit = dec["head"](h)
        if self.crf is not None:
            assert xyz is not None and mask is not None, "the CRF needs xyz and mask"
            logit = self.crf(logit, xyz, mask)
        return logit
