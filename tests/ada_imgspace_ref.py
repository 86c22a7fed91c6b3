"""Float64 restatement of the image-space stages of the reference's AdaptiveAugment.forward
(gans/augment/adaptive_augment.py:547-621: band filter, additive noise, cutout) with every random draw INJECTED, and
the operator algebra that folds the band filter into the separable form  y = a (Ay x Cx^T) + c  of the native path.

Test-side oracle only: tests/test_ada_imgspace_cpu.py holds it to tests/golden/ada_imgspace.npz (outputs of the
reference itself), the GPU tests use it where the fixture has no entry (single stages, all selects off).
"""
import numpy as np
import torch

F = torch.nn.functional
# the reference builds this vector in float32 (:550-552) whatever the image's dtype
EXPECTED_POWER = torch.tensor(np.array([10, 1, 1, 1]) / 13, dtype=torch.float32).double()


def band_gains(select, log2_gain):
    """select [B,4] bool, log2_gain [B,4] -> g [B,4]: per band, in order, the gain vector (1, .., t_i, .., 1) with
    t_i = 2^log2_gain where selected, divided by the root of its expected power, accumulated by product (:556-572)."""
    select, log2_gain = torch.as_tensor(select).bool(), torch.as_tensor(log2_gain).double()
    B, nb = log2_gain.shape
    g = torch.ones(B, nb, dtype=torch.float64)
    for i in range(nb):
        t_i = torch.where(select[:, i], torch.exp2(log2_gain[:, i]), torch.ones(B, dtype=torch.float64))
        t = torch.ones(B, nb, dtype=torch.float64)
        t[:, i] = t_i
        t = t / (EXPECTED_POWER * t.square()).sum(dim=-1, keepdim=True).sqrt()
        g = g * t
    return g


def single_band_gain(i, log2_gain):
    """Closed form of band_gains when band i alone is selected: g_i = t / sqrt(1 - e_i + e_i t^2), t = 2^log2_gain."""
    e = float(EXPECTED_POWER[i])
    t = torch.exp2(torch.as_tensor(log2_gain).double())
    return t / torch.sqrt(float(EXPECTED_POWER.sum()) - e + e * t * t)


def cutout_mask(cut, H, W):
    """cut [B,4] = (centre x, centre y, size x, size y) -> keep mask [B,1,H,W] (:616-620; plain abs(), no ring)."""
    cut = cut.double()
    cx, cy, sx, sy = (cut[:, k].view(-1, 1, 1, 1) for k in range(4))
    coord_x = torch.arange(W).reshape(1, 1, 1, -1)
    coord_y = torch.arange(H).reshape(1, 1, -1, 1)
    mask_x = ((coord_x + 0.5) / W - cx).abs() >= sx / 2
    mask_y = ((coord_y + 0.5) / H - cy).abs() >= sy / 2
    return torch.logical_or(mask_x, mask_y).double()


def image_space_f64(img, fbank, g=None, sigma=None, cut=None, eps=None):
    """Lines 547-621 on img [B,1,H,W] in float64.  g [B,4] (None: no filter stage), sigma [B] + eps [B,1,H,W] (None: no
    noise stage), cut [B,4] (None: no cutout stage)."""
    img = img.double()
    B, ch, H, W = img.shape
    if g is not None:
        hz = g.double() @ fbank.double()                        # [B, taps]
        p = fbank.shape[1] // 2
        x = img.reshape(1, B * ch, H, W)
        x = F.pad(x, (p, p, 0, 0), mode="circular")
        x = F.pad(x, (0, 0, p, p), mode="reflect")
        x = F.conv2d(x, hz[:, None, None, :], groups=B * ch)
        x = F.conv2d(x, hz[:, None, :, None], groups=B * ch)
        img = x.reshape(B, ch, H, W)
    if sigma is not None:
        img = img + eps.double() * sigma.double().view(B, 1, 1, 1)
    if cut is not None:
        img = img * cutout_mask(cut, H, W)
    return img


# ---------------------------------------------------------------------------- operator form
def circulant(kx, off, sgn, W):
    """Cx [W,W] with (x Cx^T)[j] = sum_t kx[t] x[(sgn j + off + t) mod W]  (include/dgv2.h, dgv2_ada_apply)."""
    C = torch.zeros(W, W, dtype=torch.float64)
    for j in range(W):
        for t in range(len(kx)):
            C[j, (sgn * j + off + t) % W] += float(kx[t])
    return C


def row_filter_matrix(h, H):
    """Fy [H,H]: correlation with h over the reflect-padded (no edge repeat) rows."""
    T = len(h)
    p = T // 2
    Fy = torch.zeros(H, H, dtype=torch.float64)
    for i in range(H):
        for u in range(T):
            r = abs(i + u - p)
            r = 2 * (H - 1) - r if r > H - 1 else r
            Fy[i, r] += float(h[u])
    return Fy


def fold(Ay, kx, off, sgn, c, h, W):
    """The fold of dgv2_ada_fold for one sample in float64: (Ay', kx', off', c')."""
    h = torch.as_tensor(h).double()
    kx = torch.as_tensor(kx).double()
    T, K = len(h), len(kx)
    hh = h if sgn > 0 else h.flip(0)
    k2 = torch.zeros(K + T - 1, dtype=torch.float64)
    for t in range(K):
        k2[t:t + T] += kx[t] * hh
    return row_filter_matrix(h, Ay.shape[0]) @ Ay.double(), k2, (off - T // 2) % W, c * float(h.sum()) ** 2
