#!/usr/bin/env python3
"""Generate tests/golden/pointnet.npz by running the REFERENCE's PointNet1(k=16) (gans/metrics/pointnet.py) on CPU
(build machine only).

    python tests/golden/make_pointnet_golden.py

The reference's file is imported under an alias module, none of it is copied.  Weights come from recipe.fill_pointnet,
inputs from pointnet_ref.case_points: recipe.point_clouds(100 + n, 2, n) + (2.0, -1.0, 0.5) for n in pointnet_ref.CASES.
The shift keeps the origin away from the clouds, so that a padded lane entering a maximum as the image of the origin
changes the result (the script asserts it: one appended origin point must change the transformer trunk's and the feature
trunk's outputs).  Inputs and weights are NOT stored.  What is written is data only, per case n:
  n/ref32, n/ref64   the module's [2, 1808] output in float32 and in float64 (module.double() on the upcast input)
  n/e_ref, n/max64   max |ref32 - ref64| and max |ref64|
  n/trans64          the float64 [2, 3, 3] transform
  n/stn64            the float64 [2, 1024] output of the transformer's trunk (max over the points of relu(bn3(conv3)))
Before anything is written the script ASSERTS that tests/pointnet_ref.py in float64 equals the reference's float64
outputs within 1e-12 max|ref64|.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _refshim import REFERENCE_ROOT  # noqa: E402
import pointnet_ref as R  # noqa: E402
import recipe  # noqa: E402

OUT = os.path.join(HERE, "pointnet.npz")


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_pointnet", os.path.join(REFERENCE_ROOT, "gans", "metrics", "pointnet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(net, x):
    """(features, trans, transformer-trunk output) of the reference module on x [B,3,n]."""
    kept = {}
    hooks = [net.feat.stn.bn3.register_forward_hook(lambda m, i, o: kept.__setitem__("stn", torch.relu(o).amax(dim=2))),
             net.feat.stn.register_forward_hook(lambda m, i, o: kept.__setitem__("trans", o))]
    try:
        y = net(x)
    finally:
        for h in hooks:
            h.remove()
    return y, kept["trans"], kept["stn"]


def main():
    ref = load_reference()
    net32 = ref.PointNet1(k=16)
    recipe.fill_pointnet(net32.state_dict())
    net32.eval().requires_grad_(False)
    sd = {k: v.clone() for k, v in net32.state_dict().items()}
    net64 = ref.PointNet1(k=16)
    net64.load_state_dict(sd, strict=True)
    net64.double().eval().requires_grad_(False)
    out = {}
    with torch.no_grad():
        for n in R.CASES:
            pts = R.case_points(n)
            ref32, _, _ = run(net32, pts.transpose(1, 2).contiguous())
            ref64, trans64, stn64 = run(net64, pts.double().transpose(1, 2).contiguous())
            top = float(ref64.abs().max())
            mine = R.pointnet1(sd, pts)
            mine_trans, mine_stn = R.stn(sd, pts)
            for a, b in ((mine, ref64), (mine_trans, trans64), (mine_stn, stn64)):
                assert float((a - b).abs().max()) <= 1e-12 * top, (n, float((a - b).abs().max()), top)
            # one origin point more must show: in the transformer trunk's output and in the whole feature vector
            more = torch.cat([pts, torch.zeros(2, 1, 3)], dim=1).double().transpose(1, 2).contiguous()
            ref64_o, _, stn64_o = run(net64, more)
            ch_stn, ch_feat = int((stn64_o != stn64).sum()), int((ref64_o[:, :1024] != ref64[:, :1024]).sum())
            assert ch_stn >= 100 and ch_feat >= 1024, (n, ch_stn, ch_feat)
            e_ref = float((ref32.double() - ref64).abs().max())
            out[f"{n}/ref32"], out[f"{n}/ref64"] = ref32.numpy(), ref64.numpy()
            out[f"{n}/e_ref"], out[f"{n}/max64"] = np.float64(e_ref), np.float64(top)
            out[f"{n}/trans64"], out[f"{n}/stn64"] = trans64.numpy(), stn64.numpy()
            print(f"n={n}: max|ref64| {top:.3f}  E_ref {e_ref:.3e}  restatement dev "
                  f"{float((mine - ref64).abs().max()):.1e}  an origin point changes {ch_stn} / 2048 of the transformer "
                  f"trunk, {ch_feat} / 2048 of the feature trunk")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
