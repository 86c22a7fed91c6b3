#!/usr/bin/env python3
"""Generate tests/golden/cam.npz by running the REFERENCE's context-aggregation module (CAM,
semseg/models/squeezeseg_v2.py:20-36) on CPU (build machine only).

    python tests/golden/make_cam_golden.py

The reference's semseg/models directory is imported under an alias package, as make_squeezeseg_golden.py does.
Inputs and weights are NOT stored: tests/cam_ref.py regenerates them from the integer hash of squeezeseg_ref.  What
is written is data only, per case of cam_ref.CAM_CASES: the reference module's eval() output in float32 and in float64
(module.double() on the upcast input) at squeezeseg_ref.sample_index -- every element of an output of up to 4096
elements, 4096 hashed flat indices of a larger one -- with E_ref = max |ref32 - ref64| and max |ref64| over the WHOLE
output, and the same two figures over the border pixels alone (those whose 7x7 window leaves the image).
Before anything is written the script ASSERTS that cam_ref.cam_ref in float64 equals the reference's float64 output
over the whole output within 1e-12 max|ref64|, and that a zero-padded maximum would differ at the border of the
all-negative case.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _refshim import REFERENCE_ROOT  # noqa: E402
import cam_ref as R  # noqa: E402

OUT = os.path.join(HERE, "cam.npz")
ALIAS = "reference_semseg_models"


def load_reference():
    pkg = types.ModuleType(ALIAS)
    pkg.__path__ = [os.path.join(REFERENCE_ROOT, "semseg", "models")]
    sys.modules[ALIAS] = pkg
    return importlib.import_module(ALIAS + ".squeezeseg_v2")


def main():
    torch.manual_seed(0)
    v2 = load_reference()
    out = {}
    with torch.no_grad():
        for i, (B, C, H, W, kind) in enumerate(R.CAM_CASES):
            name = R.cam_case_name(i)
            cam = v2.CAM(C, R.REDUCTION)
            sd = R.cam_case_state_dict(i, cam.state_dict())
            cam.load_state_dict(sd, strict=True)
            cam.eval()
            x = R.cam_case_input(i)
            ref32 = cam(x.clone())
            ref64 = cam.double()(x.double())
            mine = R.cam_ref(sd, x)
            top = float(ref64.abs().max())
            dev = float((mine - ref64).abs().max())
            assert dev <= 1e-12 * top, (name, dev, top)
            assert top > 0.1 and torch.isfinite(ref64).all(), (name, top)
            border = R.border_mask(H, W)
            if kind == "negative":   # what a zero padding would change: the pooled maximum of every border pixel
                assert float(x.max()) < -0.9
                zero_padded = torch.nn.functional.max_pool2d(torch.nn.functional.pad(x.double(), (3, 3, 3, 3)), 7, 1, 0)
                assert bool((zero_padded[..., border] == 0).all())
            if kind == "corners":
                flat = x.flatten(2).argmax(dim=2)
                corners = torch.tensor([0, W - 1, (H - 1) * W, H * W - 1])
                assert bool(torch.isin(flat, corners).all())
            err = (ref32.double() - ref64).abs()
            idx = R.sample_index(name, ref64.numel())
            out[name + "/ref32"] = ref32.flatten()[idx].numpy()
            out[name + "/ref64"] = ref64.flatten()[idx].numpy()
            out[name + "/e_ref"] = np.float64(err.max())
            out[name + "/max64"] = np.float64(top)
            out[name + "/e_ref_border"] = np.float64(err[..., border].max())
            out[name + "/max64_border"] = np.float64(ref64[..., border].abs().max())
            print(f"{name}: max|ref64| {top:.3f}  E_ref {float(err.max()):.3e}  border E_ref "
                  f"{float(err[..., border].max()):.3e}  restatement dev {dev:.1e}")

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
