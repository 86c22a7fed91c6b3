"""kNN label filter of RangeNet++ [Milioto et al., IROS 2019] in the simplified form of the reference's
semseg/models/knn.py:19-76 -- same constructor, attributes and `dist_kernel` buffer -- on the native kernel
(gans.models.ops.native.knn2d, csrc/knn.hip).

Per pixel p, over the K = kh kw window slots o_k (outside the image: depth 0, label 0; a negative neighbour depth
counts as +inf, the anchor is used raw):
    dist_k(p) = sum_j dist_kernel(o_j) |depth(p + o_j + o_k) - depth(p + o_j)|      (anchors inside the image only)
the k slots of smallest dist_k(p) (ties: lower slot first) vote for label(p + o_k) unless cutoff > 0 and
dist_k(p) > cutoff; the result is the most voted class (ties and no votes: the lowest).  All in float32.
"""
import torch
from torch import nn
from torch.nn.modules.utils import _pair

from gans.models.ops.native.knn import check_knn_config, knn2d


def get_gaussian_kernel(kernel_size, sigma, device="cpu"):
    """[kh,kw] float32 exp(-(dy^2 + dx^2) / (2 sigma^2)), normalised to sum 1; the operations and their order are the
    reference's (semseg/models/knn.py:7-16), so the values are too."""
    kh, kw = _pair(kernel_size)
    if kh % 2 != 1 or kw % 2 != 1:
        raise ValueError(f"get_gaussian_kernel: the kernel size must be odd, got {(kh, kw)}")
    hs = torch.arange(kh, device=device) - kh // 2
    ws = torch.arange(kw, device=device) - kw // 2
    pdist = torch.stack(torch.meshgrid(hs, ws, indexing="ij"), dim=-1).pow(2).sum(dim=-1)
    kernel = torch.exp(-pdist / (2 * sigma**2))
    kernel /= kernel.sum()
    return kernel


class kNN2d(nn.Module):
    """Drop-in for the reference's kNN2d.  Supported by the kernel: odd kernel sizes up to 5 per side (rectangular
    ones included, 1 x 1 excluded: its distance kernel is zero), 1 <= k <= kh kw; anything else raises ValueError here."""

    def __init__(self, num_classes, k=3, kernel_size=3, sigma=1.0, cutoff=1.0):
        super().__init__()
        self.num_classes = num_classes
        self.k = k
        self.kernel_size = _pair(kernel_size)
        check_knn_config(num_classes, k, self.kernel_size)
        self.padding = (self.kernel_size[0] // 2, self.kernel_size[1] // 2)
        self.sigma = sigma
        self.cutoff = cutoff
        # inverse gaussian kernel: far slots cost more
        self.register_buffer("dist_kernel", (1 - get_gaussian_kernel(self.kernel_size, self.sigma))[None, None])

    def forward(self, depth, label):
        """depth [B,1,H,W], label [B,H,W] -> filtered labels, int64 [B,H,W]."""
        return knn2d(depth, label, self.dist_kernel, self.k, self.num_classes, self.cutoff)
