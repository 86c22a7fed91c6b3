"""Test-side oracle of the CRF-RNN layer: the arithmetic of include/dgv2.h ("CRF-RNN refinement layer") in plain torch
ops, in the dtype and on the device of its arguments (float64 on the CPU in the tests; scripts/mb_crf.py times it in
float32 on the GPU as the tensor-op composition).  Gradients come from autograd.

    P = softmax(Q);  S_c = sum_n g_c(n) P_c(p+n);  L_c = sum_n a_c(n) P_c(p+n)
    A_c = m(p) sum_{n != 0} exp(-|xyz(p+n) - xyz(p)|^2 / (2 theta_beta[c]^2)) m(p+n) P_c(p+n)
    Q_c = U_c - sum_c' M[c,c'] (ws[c'] S_c' + wa[c'] A_c' L_c')
"""
import torch
import torch.nn.functional as F


def crf_ref(unary, xyz, mask, kernel_gamma, kernel_alpha, theta_beta, weight_smoothness, weight_appearance, compat,
            num_iters):
    B, C, H, W = unary.shape
    kh, kw = kernel_gamma.shape[2:]
    ph, pw = kh // 2, kw // 2
    m = mask.reshape(B, 1, H, W)
    diag = torch.arange(C)
    g, a = kernel_gamma[diag, diag], kernel_alpha[diag, diag]            # [C,kh,kw]
    ws, wa, M = weight_smoothness.reshape(1, C, 1, 1), weight_appearance.reshape(1, C, 1, 1), compat.reshape(C, C)
    taps = [(dy, dx) for dy in range(kh) for dx in range(kw)]

    def shifted(x):
        xp = F.pad(x, (pw, pw, ph, ph))
        return {t: xp[:, :, t[0]:t[0] + H, t[1]:t[1] + W] for t in taps}

    inv = 1.0 / (2 * theta_beta.reshape(1, C, 1, 1) ** 2)
    beta = {t: torch.exp(-(x - xyz).pow(2).sum(1, keepdim=True) * inv)
            for t, x in shifted(xyz.detach()).items() if t != (ph, pw)}
    Q = unary
    for _ in range(num_iters):
        P = torch.softmax(Q, dim=1)
        sP, smP = shifted(P), shifted(m * P)
        S = sum(g[:, dy, dx].reshape(1, C, 1, 1) * sP[dy, dx] for dy, dx in taps)
        L = sum(a[:, dy, dx].reshape(1, C, 1, 1) * sP[dy, dx] for dy, dx in taps)
        A = m * sum(beta[t] * smP[t] for t in taps if t != (ph, pw))
        T = ws * S + wa * A * L
        Q = unary - torch.einsum("cd,bdhw->bchw", M, T)
    return Q


def from_state_dict(sd, unary, xyz, mask, num_iters):
    """crf_ref on a CRFRNN state dict (tensors already in the wanted dtype)."""
    return crf_ref(unary, xyz, mask, sd["kernel_gamma"], sd["kernel_alpha"], sd["theta_beta"], sd["weight_smoothness"],
                   sd["weight_appearance"], sd["label_compatibility.weight"], num_iters)
