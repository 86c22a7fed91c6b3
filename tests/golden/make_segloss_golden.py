#!/usr/bin/env python3
"""Generate tests/golden/segloss.npz by running the REFERENCE's FocalLoss and masked mean on CPU (build machine only).

    python tests/golden/make_segloss_golden.py

The reference's semseg/models/loss.py is loaded from the reference tree by file path (its package shares its name with
this project's) and run twice per case, in float32 and in float64, on the same seeded float32 inputs.  What is written
is data only: logits, labels, mask and class weights of each case, and per precision the reference's per-pixel loss
(reduction="none"), its masked scalar sum(loss * mask) / sum(mask) (train_semseg.py:194-197) and logit.grad of that
scalar.  gamma == 0 cases also carry F.cross_entropy(weight=alpha, reduction="none"), which the script asserts to
equal the module's result: the configs' `cross_entropy` branch is the module at gamma = 0.

The mask is about 80 % ones in horizontal runs; case c1's mask is non-binary (weights in (0.5, 1.5)).  Before anything
is written the script ASSERTS that every float64 value is finite, that every class occurs in cases of at least 100
pixels, and that the saturated case holds a pixel whose float32 p_y is exactly 1 and a pixel with a loss above 50.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _refshim import REFERENCE_ROOT  # noqa: E402

REFERENCE_FILE = os.path.join(REFERENCE_ROOT, "semseg", "models", "loss.py")
OUT = os.path.join(HERE, "segloss.npz")

# (B, C, H, W, gamma, logit scale)
CASES = [
    (2, 3, 9, 37, 2.0, 1.0),
    (1, 4, 7, 130, 2.0, 4.0),      # non-binary mask
    (1, 20, 5, 33, 2.0, 8.0),
    (2, 32, 3, 5, 1.0, 4.0),
    (1, 4, 7, 40, 0.0, 4.0),       # plain weighted cross-entropy
    (1, 4, 7, 40, 2.0, 30.0),      # saturated: p_y rounds to 1 and to 0
    (1, 1, 1, 9, 2.0, 1.0),        # C = 1: the loss is identically 0
    (1, 3, 6, 50, 1.5, 4.0),       # non-integer gamma
]
NON_BINARY, SATURATED = 1, 5


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_semseg_loss", REFERENCE_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FocalLoss


def run_mask(shape, g):
    """About 80 % ones: zeros in horizontal runs of 1 to 4."""
    B, H, W = shape
    seeds = torch.rand(B, H, W, generator=g) < 0.08
    length = torch.randint(1, 5, (B, H, W), generator=g)
    zero = torch.zeros(B, H, W, dtype=torch.bool)
    for n in range(4):
        hit = seeds & (length > n)
        zero[:, :, n:] |= hit[:, :, :W - n]
    return (~zero).float()


def run_reference(FocalLoss, logit, label, mask, alpha, gamma, dtype):
    z = logit.detach().clone().to(dtype).requires_grad_(True)
    crit = FocalLoss(gamma=gamma, alpha=alpha.to(dtype), reduction="none")
    loss_map = crit(z, label)
    scalar = (loss_map * mask.to(dtype)).sum() / mask.to(dtype).sum()
    scalar.backward()
    return loss_map.detach(), scalar.detach(), z.grad


def main():
    torch.set_num_threads(4)
    FocalLoss = load_reference()
    out = {"cases": np.array([f"c{i}" for i in range(len(CASES))])}
    for i, (B, C, H, W, gamma, scale) in enumerate(CASES):
        g = torch.Generator().manual_seed(5500 + i)
        logit = scale * torch.randn(B, C, H, W, generator=g)
        label = torch.randint(0, C, (B, H, W), generator=g)
        mask = run_mask((B, H, W), g)
        if i == NON_BINARY:
            mask = mask * (0.5 + torch.rand(B, H, W, generator=g))
        alpha = 0.25 + 3.5 * torch.rand(C, generator=g)
        map32, loss32, grad32 = run_reference(FocalLoss, logit, label, mask, alpha, gamma, torch.float32)
        map64, loss64, grad64 = run_reference(FocalLoss, logit, label, mask, alpha, gamma, torch.float64)
        assert map32.dtype == torch.float32 and grad32.dtype == torch.float32 and map64.dtype == torch.float64
        for t in (map64, loss64, grad64):
            assert bool(torch.isfinite(t).all()), (i, "float64 reference not finite")
        for t in (map32, loss32, grad32):
            assert bool(torch.isfinite(t).all()), (i, "float32 reference not finite")
        if B * H * W >= 100:
            assert torch.bincount(label.flatten(), minlength=C).min() > 0, (i, "a class does not occur")
        py32 = F.softmax(logit, dim=1).gather(1, label[:, None]).squeeze(1)
        if i == SATURATED:
            assert bool((py32 == 1).any()) and bool((map64 > 50).any()), "the saturated case is not saturated"
        if C == 1:
            assert float(map64.abs().max()) == 0
        pre = f"c{i}."
        out[pre + "config"] = np.array([B, C, H, W])
        out[pre + "gamma_scale"] = np.array([gamma, scale], dtype=np.float64)
        for key, v in (("logit", logit), ("label", label), ("mask", mask), ("alpha", alpha), ("loss_map32", map32),
                       ("loss32", loss32), ("grad32", grad32), ("loss_map64", map64), ("loss64", loss64), ("grad64", grad64)):
            out[pre + key] = v.numpy()
        if gamma == 0:
            for dtype, tag, own in ((torch.float32, "xent32", map32), (torch.float64, "xent64", map64)):
                xent = F.cross_entropy(logit.to(dtype), label, weight=alpha.to(dtype), reduction="none")
                assert torch.equal(xent, own), "gamma = 0 is not F.cross_entropy"
                out[pre + tag] = xent.numpy()
        print(f"c{i} {(B, C, H, W)} gamma {gamma} scale {scale}: mask mean {float(mask.mean()):.3f}, loss {float(loss64):.6g}, "
              f"max L {float(map64.max()):.4g}, E_ref map {float((map32.double() - map64).abs().max()):.2e}, "
              f"scalar {abs(float(loss32) - float(loss64)):.2e}, grad {float((grad32.double() - grad64).abs().max()):.2e} "
              f"(max |grad| {float(grad64.abs().max()):.2e}), p_y == 1 at {int((py32 == 1).sum())} pixels")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
