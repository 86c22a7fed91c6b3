"""Earth mover's distance by approximate matching on the MI355X: dgv2_emd_approxmatch / _matchcost / _matchcost_grad,
and dgv2_emd_pairwise_cost for the all-pairs cost matrices of COV / MMD / 1-NNA (no match matrix, no gradient).

Mirror of the reference's gans/metrics/distance/emd/earth_mover_distance.py:18-41: cost (B,) = sum of matched
distances (callers divide by the number of points, cov_mmd_1nna.py:22); the backward treats the match as fixed.
"""
import torch

from dgv2_native import call, check, ptr, stream, try_call

PAIR_MAX_POINTS = 4096   # DGV2_EMD_PAIR_MAX_POINTS: n + m that dgv2_emd_pairwise_cost takes
PAIRS_PER_LAUNCH = 1 << 14


def _shapes(xyz1, xyz2):
    if xyz1.dtype != torch.float32 or xyz2.dtype != torch.float32:
        raise RuntimeError("earth_mover_distance: float32 point clouds expected")
    if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.size(2) != 3 or xyz2.size(2) != 3 or xyz1.size(0) != xyz2.size(0):
        raise RuntimeError(f"earth_mover_distance: expected (B,N,3) and (B,M,3), got {tuple(xyz1.shape)}, {tuple(xyz2.shape)}")
    check(xyz1, xyz2)   # the reference's CHECK_INPUT: device-resident and contiguous
    return xyz1.size(0), xyz1.size(1), xyz2.size(1)


def approxmatch_forward(xyz1, xyz2):
    """-> (match (B, M, N), temp (B, 2 (N + M)))  (earth_mover_distance.cpp:26-50)."""
    B, n, m = _shapes(xyz1, xyz2)
    match = torch.empty(B, m, n, device=xyz1.device)
    temp = torch.empty(B, (n + m) * 2, device=xyz1.device)
    call("dgv2_emd_approxmatch", ptr(match), ptr(temp), ptr(xyz1), ptr(xyz2), B, n, m, stream())
    return match, temp


def matchcost_forward(xyz1, xyz2, match):
    B, n, m = _shapes(xyz1, xyz2)
    check(match)
    cost = torch.empty(B, device=xyz1.device)
    call("dgv2_emd_matchcost", ptr(cost), ptr(match), ptr(xyz1), ptr(xyz2), B, n, m, stream())
    return cost


def matchcost_backward(xyz1, xyz2, match):
    B, n, m = _shapes(xyz1, xyz2)
    check(match)
    g1 = torch.empty_like(xyz1)
    g2 = torch.empty_like(xyz2)
    call("dgv2_emd_matchcost_grad", ptr(g1), ptr(g2), ptr(match), ptr(xyz1), ptr(xyz2), B, n, m, stream())
    return g1, g2


class EarthMoverDistanceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2):
        match, _ = approxmatch_forward(xyz1, xyz2)
        ctx.save_for_backward(xyz1, xyz2, match)
        return matchcost_forward(xyz1, xyz2, match)

    @staticmethod
    def backward(ctx, grad_cost):
        xyz1, xyz2, match = ctx.saved_tensors
        g1, g2 = matchcost_backward(xyz1, xyz2, match)
        scale = grad_cost.reshape(-1, 1, 1)
        return g1 * scale, g2 * scale


earth_mover_distance = EarthMoverDistanceFunction.apply


@torch.no_grad()
def pairwise_emd_cost(xyz1, xyz2, chunk=256):
    """(B1, N, 3), (B2, M, 3) -> (B1, B2): cost[i, j] = earth_mover_distance(xyz1[i], xyz2[j]), not divided by N.

    dgv2_emd_pairwise_cost, one workgroup per pair (the match matrix never exists), launched in slabs of rows.  Above
    its cap on N + M the same matrix comes from the batched entries, row by row in chunks of `chunk` clouds."""
    if xyz1.dtype != torch.float32 or xyz2.dtype != torch.float32:
        raise RuntimeError("pairwise_emd_cost: float32 point clouds expected")
    if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.size(2) != 3 or xyz2.size(2) != 3:
        raise RuntimeError(f"pairwise_emd_cost: expected (B1,N,3) and (B2,M,3), got {tuple(xyz1.shape)}, {tuple(xyz2.shape)}")
    check(xyz1, xyz2)
    B1, n, B2, m = xyz1.size(0), xyz1.size(1), xyz2.size(0), xyz2.size(1)
    cost = torch.empty(B1, B2, device=xyz1.device)
    if B1 == 0 or B2 == 0:
        return cost
    # rows of xyz1 per launch: a launch stays near PAIRS_PER_LAUNCH workgroups (about half a second at 2048 + 2048
    # points), so the protocol's 2048 x 2048 matrix is 256 launches, not one that holds the device for two minutes
    rows = max(1, min(PAIRS_PER_LAUNCH // B2, 65535))
    native = True
    for i in range(0, B1, rows):
        r = min(rows, B1 - i)
        native = try_call("dgv2_emd_pairwise_cost", ptr(cost[i:i + r]), ptr(xyz1[i:i + r]), ptr(xyz2), r, B2, n, m, stream())
        if not native:   # the cap is on n + m: the first launch answers for all of them
            break
    if native:
        return cost
    for i in range(B1):
        for j in range(0, B2, chunk):
            rhs = xyz2[j:j + chunk]
            lhs = xyz1[i:i + 1].expand(rhs.size(0), -1, -1).contiguous()
            match, _ = approxmatch_forward(lhs, rhs)
            cost[i, j:j + rhs.size(0)] = matchcost_forward(lhs, rhs, match)
    return cost


class EarthMoverDistance(torch.nn.Module):
    def forward(self, input1, input2):
        return EarthMoverDistanceFunction.apply(input1, input2)
