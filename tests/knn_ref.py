"""Test-side oracle of the kNN label filter: the arithmetic of include/dgv2.h ("kNN label filter") in plain torch ops,
in the dtype and on the device of `depth` (float64 and float32 on the CPU in the tests; scripts/mb_knn.py times it in
float32 on the GPU as the tensor-op composition).

    nb_k(q) = depth(q + o_k) (0 outside the image), +inf where < 0      jump_k(q) = |nb_k(q) - depth(q)|
    dist_k(p) = sum_j w(o_j) jump_k(p + o_j)  (0 for anchors outside the image)
    the k slots of smallest dist_k(p), ties to the lower slot, vote for label(p + o_k) unless cutoff > 0 and
    dist_k(p) > cutoff or the label is outside [0, C); the result is the most voted class, ties to the lowest.

Beside the labels it returns every distance and, per pixel, the DECISION MARGIN: how far the distances are from a
value at which the selection or a cutoff decision would flip -- the smaller of
    the gap between the k-th and the (k+1)-th smallest distance, where the latter is finite and k < K;
    the smallest |dist_k(p) - cutoff| over the slots, when cutoff > 0
(+inf where neither applies).  A pixel whose margin is below the rounding of the distances is one where float32 and
float64 may legitimately disagree.
"""
import torch
import torch.nn.functional as F


def distances(depth, dist_kernel):
    """depth [B,1,H,W], dist_kernel [kh,kw] (or [1,1,kh,kw]) -> dist [B,K,H,W] in depth's dtype."""
    B, _, H, W = depth.shape
    kh, kw = dist_kernel.shape[-2:]
    K, pad = kh * kw, (kh // 2, kw // 2)
    nb = F.unfold(depth, (kh, kw), padding=pad).reshape(B, K, H, W)
    nb = torch.where(nb < 0, torch.full_like(nb, float("inf")), nb)
    jump = (nb - depth).abs()
    w = dist_kernel.reshape(1, 1, kh, kw).to(depth.dtype).expand(K, 1, kh, kw)
    return F.conv2d(jump, w, padding=pad, groups=K)


def knn_ref(depth, label, dist_kernel, k, num_classes, cutoff, with_margin=True):
    """-> (labels int64 [B,H,W], dist [B,K,H,W], margin [B,H,W] or None)."""
    B, _, H, W = depth.shape
    kh, kw = dist_kernel.shape[-2:]
    K, C = kh * kw, num_classes
    dist = distances(depth, dist_kernel)
    d_sorted, order = dist.sort(dim=1, stable=True)            # ties: the lower slot first
    d_sel, slots = d_sorted[:, :k], order[:, :k]
    lab = F.unfold(label[:, None].to(depth.dtype), (kh, kw), padding=(kh // 2, kw // 2)).reshape(B, K, H, W).long()
    lab_sel = lab.gather(1, slots)
    discard = (lab_sel < 0) | (lab_sel >= C)
    if cutoff > 0:
        discard = discard | (d_sel > cutoff)
    bins = torch.zeros(B, C + 1, H, W, dtype=depth.dtype, device=depth.device)
    bins.scatter_add_(1, torch.where(discard, torch.full_like(lab_sel, C), lab_sel), torch.ones_like(d_sel))
    labels = bins[:, :C].argmax(dim=1)
    if not with_margin:
        return labels, dist, None
    inf = torch.full((B, H, W), float("inf"), dtype=depth.dtype, device=depth.device)
    margin = inf
    if k < K:
        nxt = d_sorted[:, k]
        margin = torch.where(torch.isfinite(nxt), nxt - d_sorted[:, k - 1], inf)
    if cutoff > 0:
        away = (dist - cutoff).abs()
        margin = torch.minimum(margin, torch.where(torch.isfinite(away), away, torch.full_like(away, float("inf"))).amin(dim=1))
    return labels, dist, margin


def fragile_threshold(dist64, dist32):
    """1e-6 S + 4 D: S the largest finite float64 distance, D the largest deviation of the float32 distances from the
    float64 ones over entries finite in both."""
    fin = torch.isfinite(dist64) & torch.isfinite(dist32)
    S = float(dist64[torch.isfinite(dist64)].max()) if bool(torch.isfinite(dist64).any()) else 0.0
    D = float((dist32.double() - dist64)[fin].abs().max()) if bool(fin.any()) else 0.0
    return 1e-6 * S + 4 * D, S, D
