"""native.latent: one launch for everything a stage-1 inversion step does after backward() (reference:
gans/inversion.py:10-20,81-90, demo_inversion.py:147-152) on dgv2_latent_step (include/dgv2.h states the arithmetic,
DESIGN.md section 38 the kernel).

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI, see the package docstring).  In place, float32, no
allocation and no host readback: the call is safe under a hipGraph capture.
"""
import torch

import dgv2_native as N

LATENT_MAX_ND = 16384   # floats of one sample's latent the kernel holds in LDS


def _state(name, t, shape, dtype=torch.float32):
    if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
        raise ValueError(f"latent_step: {name} must be a {dtype} tensor of shape {tuple(shape)}, got "
                         f"{None if t is None else (t.dtype, tuple(t.shape))}")
    return t


def latent_step(z, g_z, m_z, v_z, step, loss_terms, loss_log, geo, *, lr, rampup_ratio=0.05, rampdown_ratio=0.25,
                betas=(0.9, 0.999), eps=1e-8, geo_coef=0.0, hypersphere=False, phase=None, g_phase=None, m_p=None,
                v_p=None):
    """One optimisation step on every sample of the batch, IN PLACE (dgv2_latent_step): g_z += geo_coef * d geocross,
    loss_log[step] = loss_terms + geo_coef * geo, lr = lr * lr_schedule(step), Adam on z (and phase), the hypersphere
    projection, step += 1.  z, g_z, m_z, v_z [B,N,D]; phase, g_phase, m_p, v_p [B,2] or all None; step int32 [B];
    loss_terms, geo [B]; loss_log [num_steps,B].  A sample whose counter has reached num_steps is left untouched.
    ValueError for shapes / dtypes outside the contract, RuntimeError for CPU or non-contiguous tensors."""
    if z.ndim != 3:
        raise ValueError(f"latent_step: z must be [B,N,D], got {tuple(z.shape)}")
    B, n, D = z.shape
    if min(B, n, D) < 1 or n * D > LATENT_MAX_ND:
        raise ValueError(f"latent_step: z {tuple(z.shape)} is outside the kernel's range (N * D <= {LATENT_MAX_ND})")
    if loss_log.ndim != 2 or loss_log.shape[0] < 1:
        raise ValueError(f"latent_step: loss_log must be [num_steps,B], got {tuple(loss_log.shape)}")
    num_steps = loss_log.shape[0]
    if geo_coef != 0.0 and n < 2:
        raise ValueError("latent_step: the geocross term needs two styles at least (geo_coef != 0 with N = 1)")
    for name, t in (("z", z), ("g_z", g_z), ("m_z", m_z), ("v_z", v_z)):
        _state(name, t, (B, n, D))
    ph = (phase, g_phase, m_p, v_p)
    if any(t is None for t in ph) != all(t is None for t in ph):
        raise ValueError("latent_step: phase, g_phase, m_p and v_p go together (all four or none)")
    if phase is not None:
        for name, t in (("phase", phase), ("g_phase", g_phase), ("m_p", m_p), ("v_p", v_p)):
            _state(name, t, (B, 2))
    _state("step", step, (B,), torch.int32)
    _state("loss_terms", loss_terms, (B,))
    _state("geo", geo, (B,))
    _state("loss_log", loss_log, (num_steps, B))
    N.check(z, g_z, m_z, v_z, step, loss_terms, loss_log, geo, *ph)
    N.call("dgv2_latent_step", N.ptr(z), N.ptr(g_z), N.ptr(m_z), N.ptr(v_z), N.ptr(phase), N.ptr(g_phase), N.ptr(m_p),
           N.ptr(v_p), N.ptr(step), N.ptr(loss_terms), N.ptr(loss_log), N.ptr(geo), B, n, D, num_steps, float(lr),
           float(rampup_ratio), float(rampdown_ratio), float(betas[0]), float(betas[1]), float(eps), float(geo_coef),
           int(bool(hypersphere)), N.stream())


__all__ = ["latent_step", "LATENT_MAX_ND"]
