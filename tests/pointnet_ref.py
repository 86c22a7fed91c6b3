"""Float64 restatement of the FPD / KPD PointNet (include/dgv2.h "PointNet trunk" for the two trunks, gans/metrics/
pointnet.py for the tails), written from the arithmetic and not from either implementation: plain matrix products on a
state dict.  tests/golden/make_pointnet_golden.py asserts that it equals the reference's own float64 module; the tests
use it where no fixture exists (the kernel's tile edges, shifted biases).  Also the shared inputs of those tests."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import recipe  # noqa: E402

CASES = (1, 2, 63, 64, 65, 257, 500, 2048)          # points per cloud of the fixture cases, two clouds each
SHIFT = (2.0, -1.0, 0.5)                            # keeps the origin away from every cloud
EPS = 1e-5                                          # nn.BatchNorm1d's default


def case_points(n, B=2):
    """The fixture's input of case n, float32 [B,n,3]."""
    return recipe.point_clouds(100 + n, B, n) + torch.tensor(SHIFT)


def state_dict():
    """PointNet1(k=16) weights by recipe, float32, under the reference's key names."""
    from gans.metrics.pointnet import PointNet1
    net = PointNet1(k=16)
    return {k: v.clone() for k, v in recipe.fill_pointnet(net.state_dict()).items()}


def fold(sd, lin, bn=None, dtype=torch.float64):
    """(W [out,in], b [out]) of `bn`(`lin`(x)) in evaluation mode, from the state dict, computed in `dtype`."""
    w = sd[lin + ".weight"].to(dtype)
    w, b = w.reshape(w.shape[0], -1), sd[lin + ".bias"].to(dtype)
    if bn is None:
        return w, b
    s = sd[bn + ".weight"].to(dtype) / torch.sqrt(sd[bn + ".running_var"].to(dtype) + EPS)
    return w * s[:, None], (b - sd[bn + ".running_mean"].to(dtype)) * s + sd[bn + ".bias"].to(dtype)


def trunk_layers(sd, prefix, dtype=torch.float64):
    """The three folded per-point layers of the trunk at `prefix` ("feat.stn." or "feat.")."""
    return [fold(sd, f"{prefix}conv{i}", f"{prefix}bn{i}", dtype) for i in (1, 2, 3)]


def trunk(pts, trans, layers, relu_last):
    """pts [B,N,3], trans [B,3,3] or None, layers = three (W, b) -> [B,1024], in the dtype of the operands."""
    q = pts if trans is None else torch.einsum("bpi,bij->bpj", pts, trans)
    (w1, b1), (w2, b2), (w3, b3) = layers
    h = torch.relu(q @ w1.T + b1)
    h = torch.relu(h @ w2.T + b2)
    h = h @ w3.T + b3
    if relu_last:
        h = torch.relu(h)
    return h.amax(dim=1)


def stn(sd, pts):
    """(trans [B,3,3], the transformer trunk's [B,1024]) in float64."""
    pts = pts.double()
    g = trunk(pts, None, trunk_layers(sd, "feat.stn."), True)
    x = torch.relu(g @ fold(sd, "feat.stn.fc1", "feat.stn.bn4")[0].T + fold(sd, "feat.stn.fc1", "feat.stn.bn4")[1])
    x = torch.relu(x @ fold(sd, "feat.stn.fc2", "feat.stn.bn5")[0].T + fold(sd, "feat.stn.fc2", "feat.stn.bn5")[1])
    x = x @ fold(sd, "feat.stn.fc3")[0].T + fold(sd, "feat.stn.fc3")[1]
    return x.view(-1, 3, 3) + torch.eye(3, dtype=torch.float64, device=x.device), g


def pointnet1(sd, pts):
    """pts [B,N,3] -> the [B,1808] feature of PointNet1(k=16), in float64."""
    trans, _ = stn(sd, pts)
    x1 = trunk(pts.double(), trans, trunk_layers(sd, "feat."), False)
    x2 = torch.relu(x1 @ fold(sd, "fc1", "bn1")[0].T + fold(sd, "fc1", "bn1")[1])
    x3 = torch.relu(x2 @ fold(sd, "fc2", "bn2")[0].T + fold(sd, "fc2", "bn2")[1])
    x4 = x3 @ fold(sd, "fc3")[0].T + fold(sd, "fc3")[1]
    return torch.cat((x1, x2, x3, x4), dim=1)


def bound(e_ref, max64):
    """The float32 bound of DESIGN.md 31.3: four times the reference's own float32 deviation plus 2^-22 of the scale."""
    return 4.0 * float(e_ref) + 2.0 ** -22 * float(max64)


def load_fixture():
    return np.load(os.path.join(GOLDEN, "pointnet.npz"))
