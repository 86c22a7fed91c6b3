"""Restatement of dgv2_latent_step's contract (include/dgv2.h "Latent fitting") in torch on the CPU, in float64 by
default and in float32 on request (the "float32 torch restatement" whose distance from float64 sets the GPU tolerance).

The C ABI carries the scalars as floats: every scalar is rounded to float32 first, then used in double, as the kernel
does.  tests/test_sim2real_cpu.py holds this file to torch.optim.Adam + LambdaLR + autograd through
gans.inversion.geocross_loss (and SphericalOptimizer) in float64."""
import math

import numpy as np
import torch


def f32(x):
    """The value the C ABI delivers for a float argument."""
    return float(np.float32(x))


def lr_gamma(k, num_steps, rampup_ratio, rampdown_ratio):
    """demo_inversion.py:147-152 on the float32-rounded ratios, in double."""
    up, down = f32(rampup_ratio), f32(rampdown_ratio)
    t = k / num_steps
    gamma = min(1.0, (1.0 - t) / down)
    gamma = 0.5 - 0.5 * math.cos(gamma * math.pi)
    return gamma * (min(1.0, t / up) if up > 0 else 1.0)


def geocross_ref(x):
    """x [N,D] -> (mean over the N^2 ordered pairs of atan2(A, B)^3, its gradient [N,D]), in x's dtype, the sums taken
    over the differences themselves."""
    n = x.shape[0]
    diff = x[:, None, :] - x[None, :, :]
    summ = x[:, None, :] + x[None, :, :]
    A = (diff.pow(2).sum(-1) + 1e-9).sqrt()
    Bq = (summ.pow(2).sum(-1) + 1e-9).sqrt()
    th = torch.atan2(A, Bq)
    den = A * A + Bq * Bq
    wa = 3 * th * th * (Bq / (den * A))
    wb = 3 * th * th * (A / (den * Bq))
    grad = (wa[:, :, None] * diff - wb[:, :, None] * summ).sum(1) * (2.0 / (n * n))
    return (th * th * th).mean(), grad


def latent_step_ref(z, g_z, m_z, v_z, step, loss_terms, loss_log, geo, *, lr0, num_steps, rampup_ratio=0.05,
                    rampdown_ratio=0.25, beta1=0.9, beta2=0.999, eps=1e-8, geo_coef=0.0, hypersphere=False,
                    phase=None, g_phase=None, m_p=None, v_p=None, dtype=torch.float64):
    """One call of the kernel.  Takes CPU tensors of any float dtype, returns a dict of NEW tensors of `dtype`
    (step: int32) with every argument the kernel may write: z, g_z, m_z, v_z, phase, m_p, v_p, step, loss_log, geo."""
    c = lambda t: None if t is None else t.detach().to(dtype).clone()   # noqa: E731
    out = {"z": c(z), "g_z": c(g_z), "m_z": c(m_z), "v_z": c(v_z), "phase": c(phase), "m_p": c(m_p), "v_p": c(v_p),
           "step": step.clone(), "loss_log": c(loss_log), "geo": c(geo)}
    gp = c(g_phase)
    lt = c(loss_terms)
    b1, b2, e, coef, lr0 = f32(beta1), f32(beta2), f32(eps), f32(geo_coef), f32(lr0)
    B, n, _ = z.shape

    def adam(p, g, m, v, k):
        m += (1.0 - b1) * (g - m)
        v.mul_(b2).add_((1.0 - b2) * (g * g))
        step_size = lr0 * lr_gamma(k, num_steps, rampup_ratio, rampdown_ratio) / (1.0 - b1 ** (k + 1))
        denom = v.sqrt() / math.sqrt(1.0 - b2 ** (k + 1)) + e
        p -= step_size * (m / denom)

    for b in range(B):
        k = int(step[b])
        if k < 0 or k >= num_steps:
            continue
        gv = torch.zeros((), dtype=dtype)
        if coef != 0.0:
            gv, gg = geocross_ref(out["z"][b])
            out["g_z"][b] += coef * gg
        out["geo"][b] = gv
        out["loss_log"][k, b] = lt[b] + coef * gv
        adam(out["z"][b], out["g_z"][b], out["m_z"][b], out["v_z"][b], k)
        if phase is not None:
            adam(out["phase"][b], gp[b], out["m_p"][b], out["v_p"][b], k)
        if hypersphere:
            row = out["z"][b]
            row /= (row.pow(2).mean(dim=-1, keepdim=True) + 1e-9).sqrt()
        out["step"][b] = k + 1
    return out
