#!/usr/bin/env python3
"""Generate tests/golden/squeezeseg.npz by running the REFERENCE's Fire modules and SqueezeSeg trunks on CPU (build
machine only).

    python tests/golden/make_squeezeseg_golden.py

The reference's semseg/models directory is imported under an alias package (its files use relative imports, and its
package shares its name with this project's): a synthetic parent module whose __path__ is that directory.
SqueezeSegV2 is built with pretrained_weights=False; nothing touches the network.

Weights and Fire inputs are NOT stored: tests/squeezeseg_ref.py regenerates them from an integer hash of (key, flat
index), exactly, in uint64 numpy (conv weights with He's variance, biases / running means in [-0.3, 0.3), batch-norm
weights / running variances in [0.5, 1.5): no affine is the identity and N_s(relu(b_s)) != 0).  What is written is data
only:
  (a) per Fire case of squeezeseg_ref.FIRE_CASES: the reference module's eval() output in float32 and in float64
      (module.double() on the upcast input) at squeezeseg_ref.sample_index -- every element of an output of up to 4096
      elements, 4096 hashed flat indices of a larger one (the whole outputs of the eight cases would be 3 MB) -- with
      E_ref = max |ref32 - ref64| and max |ref64| over the WHOLE output;
  (b) per whole-model case of MODEL_CASES: img, xyz, mask and the float32 and float64 logits, whole;
  (c) the state-dict key|shape|dtype listings of V1 and V2, with and without the CRF.
Before anything is written the script ASSERTS that squeezeseg_ref.fire_ref in float64 equals the reference's float64
output over the whole output within 1e-12 max|ref64|, and that the squeeze's value at an all-bias pixel is not 0.
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
import squeezeseg_ref as R  # noqa: E402

OUT = os.path.join(HERE, "squeezeseg.npz")
ALIAS = "reference_semseg_models"


def load_reference():
    pkg = types.ModuleType(ALIAS)
    pkg.__path__ = [os.path.join(REFERENCE_ROOT, "semseg", "models")]
    sys.modules[ALIAS] = pkg
    return (importlib.import_module(ALIAS + ".squeezeseg_v1"), importlib.import_module(ALIAS + ".squeezeseg_v2"))


def main():
    torch.manual_seed(0)
    v1, v2 = load_reference()
    out = {}
    with torch.no_grad():
        for i, (ver, B, Cin, Cs, E, H, W, up) in enumerate(R.FIRE_CASES):
            name = R.fire_case_name(i)
            fire = v1.Fire(Cin, Cs, E, E, up=up) if ver == 1 else v2.Fire(Cin, Cs, E, E, 0.001, up=up)
            sd = R.hash_fill_state_dict(fire.state_dict(), salt=name + "/")
            fire.load_state_dict(sd, strict=True)
            fire.eval()
            x = R.fire_case_input(i)
            ref32 = fire(x.clone())
            ref64 = fire.double()(x.double())
            mine = R.fire_ref(sd, x)
            top = float(ref64.abs().max())
            dev = float((mine - ref64).abs().max())
            assert dev <= 1e-12 * top, (name, dev, top)
            assert top > 0.1 and torch.isfinite(ref64).all(), (name, top)
            if ver == 2:   # what a wrong padding would put outside the image
                ghost = R.fire_ref(sd, torch.zeros(1, Cin, 1, 1))
                assert float(ghost.abs().max()) > 1e-3
            idx = R.sample_index(name, ref64.numel())
            out[name + "/ref32"] = ref32.flatten()[idx].numpy()
            out[name + "/ref64"] = ref64.flatten()[idx].numpy()
            out[name + "/e_ref"] = np.float64((ref32.double() - ref64).abs().max())
            out[name + "/max64"] = np.float64(top)
            print(f"{name}: max|ref64| {top:.3f}  E_ref {float(out[name + '/e_ref']):.3e}  restatement dev {dev:.1e}")

        for i, (ver, B, H, W, crf) in enumerate(R.MODEL_CASES):
            name = R.model_case_name(i)
            if ver == 1:
                model = v1.SqueezeSegV1(R.MODEL_INPUTS, R.MODEL_CLASSES, use_crf=crf)
            else:
                model = v2.SqueezeSegV2(R.MODEL_INPUTS, R.MODEL_CLASSES, use_crf=crf, pretrained_weights=False)
            model.load_state_dict(R.hash_fill_state_dict(model.state_dict(), salt=f"v{ver}/"), strict=True)
            model.eval()
            img, xyz, mask = R.model_case_inputs(i)
            l32 = model(img.clone(), xyz, mask)
            l64 = model.double()(img.double(), xyz.double(), mask.double())
            assert torch.isfinite(l64).all()
            for key, val in (("img", img), ("xyz", xyz), ("mask", mask), ("logit32", l32), ("logit64", l64)):
                out[f"{name}/{key}"] = val.numpy()
            print(f"{name}: max|logit64| {float(l64.abs().max()):.3f}  E_ref {float((l32.double() - l64).abs().max()):.3e}")

        for ver, mod in ((1, v1), (2, v2)):
            for crf in (False, True):
                if ver == 1:
                    model = mod.SqueezeSegV1(R.MODEL_INPUTS, R.MODEL_CLASSES, use_crf=crf)
                else:
                    model = mod.SqueezeSegV2(R.MODEL_INPUTS, R.MODEL_CLASSES, use_crf=crf, pretrained_weights=False)
                out[f"listing_v{ver}{'_crf' if crf else ''}"] = np.array(R.listing(model.state_dict()))

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
