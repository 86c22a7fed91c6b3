"""SqueezeSeg (V1) trunk for range images (reference: semseg/models/squeezeseg_v1.py): a two-branch stem, eight
encoder and four up-sampling decoder Fire modules with skip adds, a 3x3 head and the optional CRF-RNN.  Module tree
and state-dict layout are the reference's; in eval() with grad mode off every Fire module is one native launch."""
from torch import nn

from .common import ConvReLU, DeconvReLU, Head, fire_forward, init_weights_trunc_normal, setup_in_ch
from .crf_as_rnn import CRFRNN


class Fire(nn.Module):
    """Squeeze 1x1, optional x2 transposed conv along the width, then 1x1 and 3x3 expands side by side.
    forward(x, skip) also adds `skip` to the concatenated output (the decoder's residual)."""

    def __init__(self, in_ch, s1x1, e1x1, e3x3, up=False):
        super().__init__()
        self.squeeze1x1 = ConvReLU(in_ch, s1x1, 1, 1, 0)
        self.upsample = DeconvReLU(s1x1, s1x1, (1, 4), (1, 2), (0, 1)) if up else None
        self.expand1x1 = ConvReLU(s1x1, e1x1, 1, 1, 0)
        self.expand3x3 = ConvReLU(s1x1, e3x3, 3, 1, 1)

    def forward(self, x, skip=None):
        return fire_forward(self, x, skip)


class SqueezeSegV1(nn.Module):
    def __init__(self, inputs, num_classes, head_dropout_p=0.5, use_crf=False, crf_kernel_size=(3, 5),
                 crf_init_weight_smoothness=0.02, crf_init_weight_appearance=0.1, crf_theta_gamma=0.9,
                 crf_theta_alpha=0.9, crf_theta_beta=0.015, crf_num_iters=3):
        super().__init__()
        in_ch = setup_in_ch(inputs)

        def pool():
            return nn.MaxPool2d(3, (1, 2), 1)

        self.conv1a = ConvReLU(in_ch, 64, 3, (1, 2), 1)
        self.conv1b = ConvReLU(in_ch, 64, 1, 1, 0)
        self.fire2_3 = nn.Sequential(pool(), Fire(64, 16, 64, 64), Fire(128, 16, 64, 64))
        self.fire4_5 = nn.Sequential(pool(), Fire(128, 32, 128, 128), Fire(256, 32, 128, 128))
        self.fire6_9 = nn.Sequential(pool(), Fire(256, 48, 192, 192), Fire(384, 48, 192, 192),
                                     Fire(384, 64, 256, 256), Fire(512, 64, 256, 256))
        self.fire10 = Fire(512, 64, 128, 128, up=True)
        self.fire11 = Fire(256, 32, 64, 64, up=True)
        self.fire12 = Fire(128, 16, 32, 32, up=True)
        self.fire13 = Fire(64, 16, 32, 32, up=True)
        self.head = Head(64, num_classes, 3, head_dropout_p)
        self.crf = None
        if use_crf:
            self.crf = CRFRNN(num_classes=num_classes, kernel_size=crf_kernel_size,
                              init_weight_smoothness=crf_init_weight_smoothness,
                              init_weight_appearance=crf_init_weight_appearance, theta_gamma=crf_theta_gamma,
                              theta_alpha=crf_theta_alpha, theta_beta=crf_theta_beta, num_iters=crf_num_iters)
        self.apply(init_weights_trunc_normal)

    def forward(self, img, xyz=None, mask=None):
        """img [B,C,H,W] with W a multiple of 16 -> logits [B,num_classes,H,W]; xyz and mask feed the CRF."""
        h_1b = self.conv1b(img)
        h_1a = self.conv1a(img)
        h_3 = self.fire2_3(h_1a)
        h_5 = self.fire4_5(h_3)
        h = self.fire6_9(h_5)
        h = self.fire10(h, h_5)
        h = self.fire11(h, h_3)
        h = self.fire12(h, h_1a)
        h = self.fire13(h, h_1b)
        logit = self.head(h)
        if self.crf is not None:
            assert xyz is not None and mask is not None, "the CRF needs xyz and mask"
            logit = self.crf(logit, xyz, mask)
        return logit
