"""CRF-RNN refinement layer [Zheng et al., ICCV 2015] as SqueezeSeg [Wu et al., ICRA 2018] uses it on range images:
the module of the reference's semseg/models/crf_as_rnn.py:8-132 -- same constructor, parameters, buffers and state-dict
layout -- with the mean-field iterations on the native kernels (gans.models.ops.native.crf_rnn, csrc/crf.hip).

Per iteration, with P = softmax(Q) and n over the window offsets (outside the image: 0):
    S_c = sum_n kernel_gamma[c,c](n) P_c(p+n)          L_c = sum_n kernel_alpha[c,c](n) P_c(p+n)
    A_c = mask(p) sum_{n != 0} exp(-|xyz(p+n) - xyz(p)|^2 / (2 theta_beta[c]^2)) mask(p+n) P_c(p+n)
    Q_c = unary_c - sum_c' label_compatibility[c,c'] (weight_smoothness[c'] S_c' + weight_appearance[c'] A_c' L_c')
"""
import torch
from torch import nn
from torch.nn.modules.utils import _ntuple, _pair

from gans.models.ops.native.crf import check_crf_config, crf_rnn


def gaussian_window(num_classes, kernel_size, theta):
    """[C,C,kh,kw] float32, zero off the diagonal; [c,c] = exp(-(dy^2 + dx^2) / (2 theta[c]^2)) with a zero centre tap."""
    kh, kw = kernel_size
    dy = torch.arange(kh) - kh // 2
    dx = torch.arange(kw) - kw // 2
    dist2 = dy[:, None] ** 2 + dx[None, :] ** 2
    window = torch.zeros(num_classes, num_classes, kh, kw)
    for c in range(num_classes):
        window[c, c] = torch.exp(-dist2 / (2 * theta[c] ** 2))
        window[c, c, kh // 2, kw // 2] = 0
    return window


class CRFRNN(nn.Module):
    """Drop-in for the reference's CRFRNN.  Each theta is a scalar or a per-class sequence.  Supported by the kernels:
    num_classes <= 8, odd kernel sizes up to (5, 9); anything else raises ValueError here."""

    def __init__(self, num_classes, kernel_size=(3, 5), init_weight_smoothness=0.02, init_weight_appearance=0.1,
                 theta_gamma=0.9, theta_alpha=0.9, theta_beta=0.015, num_iters=3):
        super().__init__()
        self.num_classes = num_classes
        self.num_iters = num_iters
        self.kernel_size = _pair(kernel_size)
        check_crf_config(num_classes, self.kernel_size)
        self.padding = (self.kernel_size[0] // 2, self.kernel_size[1] // 2)
        per_class = _ntuple(num_classes)
        for name, theta in (("theta_gamma", theta_gamma), ("theta_alpha", theta_alpha), ("theta_beta", theta_beta)):
            self.register_buffer(name, torch.tensor(per_class(theta), dtype=torch.float32))
        self.register_buffer("kernel_gamma", gaussian_window(num_classes, self.kernel_size, self.theta_gamma))
        self.register_buffer("kernel_alpha", gaussian_window(num_classes, self.kernel_size, self.theta_alpha))
        self.weight_appearance = nn.Parameter(torch.full((1, num_classes, 1, 1), float(init_weight_appearance)))
        self.weight_smoothness = nn.Parameter(torch.full((1, num_classes, 1, 1), float(init_weight_smoothness)))
        # Potts model: a label is penalised by every OTHER label's message
        self.label_compatibility = nn.Conv2d(num_classes, num_classes, 1, bias=False)
        with torch.no_grad():
            self.label_compatibility.weight.copy_(1 - torch.eye(num_classes)[:, :, None, None])

    def apply(self, fn):
        """Returns self untouched: the backbone's weight-init functions must not reach this layer."""
        return self

    def forward(self, unary, xyz, mask):
        """unary [B,C,H,W], xyz [B,3,H,W], mask [B,H,W] or [B,1,H,W] -> refined logits [B,C,H,W] (num_iters = 0:
        unary itself).  The mask's gradient is not produced."""
        return crf_rnn(unary, xyz, mask, self.kernel_gamma, self.kernel_alpha, self.theta_beta, self.weight_smoothness,
                       self.weight_appearance, self.label_compatibility.weight, self.num_iters)
