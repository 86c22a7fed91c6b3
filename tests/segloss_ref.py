"""Test-side oracle of the segmentation training objective: the arithmetic of include/dgv2.h ("training objective of
the range-image segmentation models") in closed form, in plain torch ops, in the dtype and on the device of `logit`
(float64 and float32 on the CPU in the tests).  No autograd: the gradient is the header's formula.

    p = softmax(z),  lp = log p_y,  L = -a_y (1 - p_y)^gamma lp           (gamma == 0: (1 - p_y)^gamma = 1 exactly)
    loss = sum m L / sum m
    dL/dz_j = a_y (delta_jy - p_j) (gamma p_y (1 - p_y)^(gamma-1) lp - (1 - p_y)^gamma)
    a label outside [0, C): L = 0, gradient 0, its mask weight still in sum m
    pred = lowest index among the largest logits, times (m != 0)

1 - p_y is taken as the other classes' share of the softmax sum, which has no cancellation (the float32 run of this
file is the yardstick's error estimate for shapes outside the fixture, so it should be a good float32 evaluation).
"""
import torch


def _pieces(logit, label, alpha, gamma):
    B, C, H, W = logit.shape
    dt = logit.dtype
    in_range = (label >= 0) & (label < C)
    y = torch.where(in_range, label, torch.zeros_like(label))
    onehot = torch.zeros_like(logit).scatter_(1, y[:, None], 1.0)
    e = torch.exp(logit - logit.max(dim=1, keepdim=True).values)
    s = e.sum(dim=1, keepdim=True)
    p = e / s
    lp = (torch.log_softmax(logit, dim=1) * onehot).sum(dim=1)
    py = (p * onehot).sum(dim=1)
    q = (e * (1 - onehot)).sum(dim=1) / s[:, 0]                     # 1 - p_y
    a = torch.ones(C, dtype=dt, device=logit.device) if alpha is None else alpha.to(dt)
    ay = a[y] * in_range.to(dt)                                     # 0 switches an out-of-range pixel off
    return onehot, p, lp, py, q, ay


def loss_map(logit, label, alpha, gamma):
    """[B,H,W] in logit's dtype."""
    _, _, lp, _, q, ay = _pieces(logit, label, alpha, gamma)
    w = torch.ones_like(q) if gamma == 0 else q ** gamma
    return -ay * w * lp


def masked_loss(logit, label, mask, alpha, gamma):
    m = mask.to(logit.dtype)
    return (loss_map(logit, label, alpha, gamma) * m).sum() / m.sum()


def grad_map(logit, label, alpha, gamma, gout):
    """Gradient of sum_q gout(q) L(q) with respect to logit: [B,C,H,W]."""
    onehot, p, lp, py, q, ay = _pieces(logit, label, alpha, gamma)
    # delta_jy - p_j, with the label's own entry from the other classes' share
    d = torch.where(onehot > 0, q[:, None].expand_as(p), -p)
    if gamma == 0:
        k = -torch.ones_like(q)
    else:
        k = gamma * py * q ** (gamma - 1) * lp - q ** gamma
    return (gout.to(logit.dtype) * ay * k)[:, None] * d


def masked_grad(logit, label, mask, alpha, gamma, gout=1.0):
    """Gradient of gout * masked_loss with respect to logit."""
    m = mask.to(logit.dtype)
    return grad_map(logit, label, alpha, gamma, gout * m / m.sum())


def pred(logit, mask=None):
    """int64 [B,H,W]: torch.argmax returns the first of equal maxima on the CPU; written out here so that the rule
    does not rest on that."""
    C = logit.shape[1]
    top = logit.max(dim=1, keepdim=True).values
    idx = torch.arange(C, device=logit.device).view(1, C, 1, 1).expand_as(logit)
    first = torch.where(logit == top, idx, torch.full_like(idx, C)).min(dim=1).values
    return first if mask is None else first * (mask != 0).long()
