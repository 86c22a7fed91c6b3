#!/usr/bin/env python3
"""Generate tests/golden/knn2d.npz by running the REFERENCE's kNN2d and evaluate on CPU (build machine only).

    python tests/golden/make_knn_golden.py

The reference's semseg/models/knn.py is loaded from the reference tree by file path (its package shares its name with
this project's) and run in float32 -- it cannot run in float64: its label_bins tensor is float32.  `evaluate` is taken
from the text of the reference's test_semseg.py (the function's syntax tree alone is compiled: the file's imports of
the dataset modules never run).  What is written is data only: seeded depth and labels, the module's dist_kernel
buffer, the reference's filtered labels and the configuration of each case; and for evaluate two (label, pred, mask)
triples with the reference's tp / fp / fn.

Depth is a smooth walk along both axes plus object-like offsets; short runs of pixels are invalid: -1 (a negative
depth, which the filter turns into +inf) in about 1-2 % and 0 (the datasets' invalid value) in about 2 %.  Labels are
piecewise constant with salt noise.  Before anything is written the script ASSERTS, in every case of at least 100
pixels, that the fixture exercises the filter: between 5 % and 95 % of the selected neighbours pass the cutoff (where
there is one: with cutoff = 0 nothing is ever cut), the filter changes between 2 % and 90 % of the labels, and an
infinite distance exists wherever negatives were planted.  The knob is the depth scale of a case, not the asserts.
"""
import ast
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _refshim import REFERENCE_ROOT  # noqa: E402

REFERENCE_FILE = os.path.join(REFERENCE_ROOT, "semseg", "models", "knn.py")
REFERENCE_CLI = os.path.join(REFERENCE_ROOT, "test_semseg.py")
OUT = os.path.join(HERE, "knn2d.npz")

# (B, H, W, C, k, kernel_size, sigma, cutoff), plant negatives, depth scale (the walk's step; offsets are 10 steps)
CASES = [
    ((2, 9, 37, 4, 3, 3, 1.0, 1.0), True, 0.06),
    ((1, 7, 40, 20, 5, 5, 1.0, 1.0), True, 0.012),
    ((1, 7, 40, 20, 5, 5, 1.0, 0.0), False, 0.012),     # depth all >= 0: no inf, so no unspecified inf ties
    ((1, 5, 33, 3, 7, (3, 5), 0.7, 2.0), True, 0.05),
    ((1, 1, 9, 2, 1, 3, 1.0, 1.0), True, 0.06),
    ((1, 3, 5, 3, 9, 3, 1.0, 1.0), True, 0.06),          # k = K
    ((1, 33, 130, 4, 5, 5, 1.0, 1.0), True, 0.012),      # several tiles on both axes
]


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_knn", REFERENCE_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kNN2d


def load_reference_evaluate():
    tree = ast.parse(open(REFERENCE_CLI).read())
    (fn,) = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "evaluate"]
    scope = {"torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), REFERENCE_CLI, "exec"), scope)
    return scope["evaluate"]


def runs(shape, share, g):
    """A boolean map with about `share` of the pixels set, in horizontal runs of 1 to 3."""
    B, H, W = shape
    seeds = torch.rand(B, H, W, generator=g) < share / 2
    length = torch.randint(1, 4, (B, H, W), generator=g)
    out = torch.zeros(B, H, W, dtype=torch.bool)
    for n in range(3):
        hit = seeds & (length > n)
        out[:, :, n:] |= hit[:, :, :W - n]
    return out


def make_inputs(cfg, negatives, scale, g):
    B, H, W, C = cfg[:4]
    walk = (scale * torch.randn(B, 1, 1, W, generator=g)).cumsum(3) + (scale * torch.randn(B, 1, H, 1, generator=g)).cumsum(2)
    depth = 1.0 + walk + 0.3 * scale * torch.randn(B, 1, H, W, generator=g)
    # objects: rectangles standing in front of the background
    labels = torch.zeros(B, H, W, dtype=torch.int64)
    for _ in range(max(2, H * W // 60)):
        b = int(torch.randint(0, B, (1,), generator=g))
        h0, w0 = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
        hh, ww = int(torch.randint(1, max(2, H // 2), (1,), generator=g)), int(torch.randint(2, max(3, W // 4), (1,), generator=g))
        depth[b, 0, h0:h0 + hh, w0:w0 + ww] -= 10 * scale * float(torch.rand(1, generator=g))
        labels[b, h0:h0 + hh, w0:w0 + ww] = int(torch.randint(0, C, (1,), generator=g))
    salt = torch.rand(B, H, W, generator=g) < 0.08
    labels = torch.where(salt, torch.randint(0, C, (B, H, W), generator=g), labels)
    depth = depth.clamp_min(0.05)
    zero = runs((B, H, W), 0.02, g)
    neg = runs((B, H, W), 0.015, g) & ~zero if negatives else torch.zeros_like(zero)
    depth[:, 0][zero] = 0.0
    depth[:, 0][neg] = -1.0
    return depth, labels, zero, neg


def statistics(knn, depth, labels):
    """share of the selected neighbours within the cutoff, share of infinite distances (the module's own op sequence
    up to the distances, restated: the module does not expose them)"""
    sys.path.insert(0, os.path.dirname(HERE))
    from knn_ref import distances
    dist = distances(depth, knn.dist_kernel)
    d_sel = dist.sort(dim=1, stable=True)[0][:, :knn.k]
    return float((d_sel <= knn.cutoff).float().mean()), float(torch.isinf(dist).float().mean())


def main():
    torch.set_num_threads(4)
    kNN2d = load_reference()
    evaluate = load_reference_evaluate()
    out = {"cases": np.array([f"c{i}" for i in range(len(CASES))])}
    for i, (cfg, negatives, scale) in enumerate(CASES):
        B, H, W, C, k, ks, sigma, cutoff = cfg
        g = torch.Generator().manual_seed(5200 + i)
        depth, labels, zero, neg = make_inputs(cfg, negatives, scale, g)
        knn = kNN2d(C, k=k, kernel_size=ks, sigma=sigma, cutoff=cutoff)
        assert knn.dist_kernel.dtype == torch.float32
        refined = knn(depth.clone(), labels.clone())
        within, inf_share = statistics(knn, depth, labels)
        changed = float((refined != labels).float().mean())
        print(f"c{i} {cfg}: zero {float(zero.float().mean()):.3f}, negative {float(neg.float().mean()):.3f}, selected within "
              f"the cutoff {within:.3f}, infinite distances {inf_share:.3f}, labels changed {changed:.3f}")
        if H * W >= 100:
            if cutoff > 0:
                assert 0.05 <= within <= 0.95, (cfg, within)
            assert 0.02 <= changed <= 0.90, (cfg, changed)
            assert not negatives or (bool(neg.any()) and inf_share > 0), cfg
            assert negatives or float(depth.min()) >= 0
        kh, kw = knn.kernel_size
        pre = f"c{i}."
        out[pre + "config"] = np.array([B, H, W, C, k, kh, kw])
        out[pre + "sigma_cutoff"] = np.array([sigma, cutoff], dtype=np.float64)
        out[pre + "depth"] = depth.numpy()
        out[pre + "label"] = labels.numpy()
        out[pre + "dist_kernel"] = knn.dist_kernel.numpy()
        out[pre + "refined"] = refined.numpy()

    # evaluate: the reference applies the mask by multiplication before it counts (test_semseg.py:136-137)
    for j, (shape, C, stray) in enumerate([((2, 9, 37), 4, False), ((1, 11, 23), 6, True)]):
        g = torch.Generator().manual_seed(5300 + j)
        label = torch.randint(0, C, shape, generator=g)
        pred = torch.where(torch.rand(shape, generator=g) < 0.6, label, torch.randint(0, C, shape, generator=g))
        if stray:   # values outside [0, C) on both sides
            label = torch.where(torch.rand(shape, generator=g) < 0.05, torch.full(shape, C + 2), label)
            pred = torch.where(torch.rand(shape, generator=g) < 0.05, torch.full(shape, -1), pred)
            pred = torch.where(torch.rand(shape, generator=g) < 0.03, torch.full(shape, C), pred)
        mask = (torch.rand(shape, generator=g) < 0.8).float()
        _, tp, fp, fn = evaluate(label * mask, pred * mask, C)
        pre = f"e{j}."
        out[pre + "num_classes"] = np.array(C)
        for key, v in (("label", label), ("pred", pred), ("mask", mask), ("tp", tp.long()), ("fp", fp.long()), ("fn", fn.long())):
            out[pre + key] = v.numpy()
        print(f"e{j}: tp {tp.long().tolist()}, fp {fp.long().tolist()}, fn {fn.long().tolist()}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
