#!/usr/bin/env python3
"""Generate tests/golden/crf_rnn.npz by running the REFERENCE's CRFRNN on CPU (build machine only).

    python tests/golden/make_crf_golden.py

The reference's semseg/models/crf_as_rnn.py is loaded from the reference tree by file path (its package shares its name
with this project's).  What is written is data only: seeded float32 inputs, the module's state dict, and the reference's
output and gradients for a recorded cotangent, evaluated in float64 (module.double() on the upcast inputs) and in
float32 -- the deviation between the two is what the GPU tests derive their tolerance from.  The script ASSERTS that
the bilateral weights its xyz produces are spread between 0 and 1 before it writes anything.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _refshim import REFERENCE_ROOT  # noqa: E402

REFERENCE_FILE = os.path.join(REFERENCE_ROOT, "semseg", "models", "crf_as_rnn.py")
OUT = os.path.join(HERE, "crf_rnn.npz")

# (B, C, H, W, (kh, kw)), iterations, mask kind
CASES = [
    ((2, 3, 5, 9, (3, 5)), 3, "binary"),
    ((1, 4, 3, 5, (3, 5)), 3, "uniform"),     # a float mask, as the reference's __main__ draws it
    ((1, 2, 1, 7, (3, 5)), 3, "binary"),
    ((1, 3, 4, 6, (1, 3)), 1, "binary"),
    ((1, 2, 6, 7, (5, 3)), 3, "binary"),
    ((1, 3, 33, 130, (3, 5)), 3, "binary"),
    ((1, 8, 4, 6, (3, 5)), 3, "binary"),
]


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_crf_as_rnn", REFERENCE_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CRFRNN


def make_inputs(shape, mask_kind, g):
    B, C, H, W, _ = shape
    unary = torch.randn(B, C, H, W, generator=g) * 2
    # a smooth walk: independent steps of about 0.02 along both axes around an offset of about 10
    steps_w = 0.02 * torch.randn(B, 3, 1, W, generator=g)
    steps_h = 0.02 * torch.randn(B, 3, H, 1, generator=g)
    xyz = 10.0 + steps_w.cumsum(3) + steps_h.cumsum(2) + 0.004 * torch.randn(B, 3, H, W, generator=g)
    if mask_kind == "binary":
        mask = (torch.rand(B, H, W, generator=g) < 0.8).float()
    else:
        mask = torch.rand(B, H, W, generator=g)
    cot = torch.randn(B, C, H, W, generator=g)
    return unary, xyz, mask, cot


def build(CRFRNN, shape, iters, g):
    _, C, _, _, ks = shape
    idx = torch.arange(C, dtype=torch.float32)
    crf = CRFRNN(C, kernel_size=ks, theta_gamma=tuple((0.9 + 0.15 * idx).tolist()),
                 theta_alpha=tuple((0.7 + 0.2 * idx).tolist()), theta_beta=tuple((0.015 * (1 + idx)).tolist()),
                 num_iters=iters)
    with torch.no_grad():
        crf.weight_smoothness.mul_(1 + 0.5 * torch.rand(1, C, 1, 1, generator=g))
        crf.weight_appearance.mul_(1 + 0.5 * torch.rand(1, C, 1, 1, generator=g))
        crf.label_compatibility.weight.add_(0.3 * torch.randn(C, C, 1, 1, generator=g))   # off Potts, asymmetric
    return crf


def beta_quantiles(crf, xyz):
    beta = crf.precompute_kernel_beta(xyz).flatten()
    beta = beta[beta > 0] if bool((beta > 0).any()) else beta      # unfold's padding gives exp(-huge) = 0
    q = torch.quantile(beta.double(), torch.tensor([0.1, 0.9], dtype=torch.float64))
    return float(q[0]), float(q[1])


def run(crf, unary, xyz, mask, cot, dtype):
    crf = crf.to(dtype)
    crf.zero_grad()
    u = unary.to(dtype).clone().requires_grad_(True)
    out = crf(u, xyz.to(dtype), mask.to(dtype))
    (out * cot.to(dtype)).sum().backward()
    return {"out": out.detach(), "g_unary": u.grad, "g_weight_smoothness": crf.weight_smoothness.grad.clone(),
            "g_weight_appearance": crf.weight_appearance.grad.clone(),
            "g_label_compatibility.weight": crf.label_compatibility.weight.grad.clone()}


def main():
    torch.set_num_threads(4)
    CRFRNN = load_reference()
    out = {"cases": np.array([f"c{i}" for i in range(len(CASES))])}
    for i, (shape, iters, mask_kind) in enumerate(CASES):
        g = torch.Generator().manual_seed(4100 + i)
        unary, xyz, mask, cot = make_inputs(shape, mask_kind, g)
        crf = build(CRFRNN, shape, iters, g)
        if shape[2] * shape[3] >= 15:
            lo, hi = beta_quantiles(crf, xyz)
            assert hi - lo > 0.3, (shape, lo, hi)
        sd = {k: v.clone() for k, v in crf.state_dict().items()}
        assert all(v.dtype == torch.float32 for v in sd.values())
        pre = f"c{i}."
        out[pre + "shape"] = np.array(list(shape[:4]) + list(shape[4]) + [iters])
        for k, v in (("unary", unary), ("xyz", xyz), ("mask", mask), ("cot", cot)):
            out[pre + k] = v.numpy()
        for k, v in sd.items():
            out[pre + "sd." + k] = v.numpy()
        if i == 0:
            out["sd_keys"] = np.array(list(sd))
        out[pre + "sd_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        r32 = run(crf, unary, xyz, mask, cot, torch.float32)
        r64 = run(crf, unary, xyz, mask, cot, torch.float64)
        for k in r64:
            out[pre + k + ".f64"] = r64[k].numpy()
            out[pre + k + ".f32"] = r32[k].numpy()
            dev = float((r32[k].double() - r64[k]).abs().max())
            print(f"{pre}{k}: max |f64| {float(r64[k].abs().max()):.3g}, f32-vs-f64 deviation {dev:.2e}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
