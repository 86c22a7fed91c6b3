"""Training objective of the range-image segmentation models: the focal loss [Lin et al., ICCV 2017] of the reference's
semseg/models/loss.py:5-21 -- same constructor, `alpha` buffer and forward -- and the masked mean its training loop
takes of it (train_semseg.py:194-197), on the native kernels (gans.models.ops.native.segloss, csrc/segloss.hip).

Per pixel with logits z, label y and class weights alpha (None: 1), all in float32 whatever the logits' dtype:
    L = -alpha[y] (1 - p_y)^gamma log p_y,   p = softmax(z)           (0 where y is outside [0, C))
    MaskedSegLoss: loss = sum(mask L) / sum(mask),  pred = argmax_c z_c * (mask != 0)
gamma is 0 (plain weighted cross-entropy, the configs' `cross_entropy` branch) or >= 1.
"""
from torch import nn

from gans.models.ops.native.segloss import check_seg_loss_config, seg_focal_loss_map, seg_masked_loss


class FocalLoss(nn.Module):
    """Drop-in for the reference's FocalLoss: forward(logit [B,C,H,W], label [B,H,W]) -> the loss per pixel, float32
    [B,H,W] (reduction="none"), or its mean (reduction="mean").  One launch forward, one backward.  Supported by the
    kernels: 1 <= C <= 32, gamma == 0 or gamma >= 1; anything else raises ValueError."""

    def __init__(self, gamma, alpha=None, reduction="none"):
        super().__init__()
        check_seg_loss_config(1, gamma)
        self.gamma = gamma
        self.register_buffer("alpha", alpha)
        self.reduction = reduction
        assert self.reduction in ("none", "mean")

    def forward(self, logit, label):
        focal_loss = seg_focal_loss_map(logit, label, self.alpha, self.gamma)
        if self.reduction == "none":
            return focal_loss
        elif self.reduction == "mean":
            return focal_loss.mean()


class MaskedSegLoss(nn.Module):
    """The reference's masked_loss over FocalLoss(gamma, alpha, reduction="none") (gamma = 0: over CrossEntropyLoss(
    weight=alpha, reduction="none")), with what its loop computes next to it: forward(logit, label, mask, conf=None)
    -> (loss, pred).  loss: 0-dim float32 sum(mask L) / sum(mask), NaN where the mask sums to 0; pred: int64 [B,H,W]
    logit.argmax(1) * (mask != 0), detached; conf: None or the int64 [C+1,C+1] confusion matrix of the training scores
    (semseg.metrics reads it), with this step's counts of (label * mask, pred) added.  Two launches forward, one
    backward, no host synchronisation."""

    def __init__(self, gamma, alpha=None):
        super().__init__()
        check_seg_loss_config(1, gamma)
        self.gamma = gamma
        self.register_buffer("alpha", alpha)

    def forward(self, logit, label, mask, conf=None):
        return seg_masked_loss(logit, label, mask, self.alpha, self.gamma, conf=conf)
