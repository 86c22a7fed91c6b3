"""GAN inversion and pivotal tuning (reference: gans/inversion.py, demo_inversion.py:97-266).

MultiScaleMaskedLoss keeps the reference's interface and state-dict layout; its arithmetic runs in three kernels of
csrc/inversion.hip: the target's pyramid once per (ref, mask), then ONE launch forward and ONE backward per call, for
any number of levels.  SphericalOptimizer, geocross_loss and normalize_noise_ touch a few KB and stay tensor ops.
`invert` is the two-stage optimisation of demo_inversion.py without its display code, for a batch of targets."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from .models import ops
from .models.ops import native
from .utils import set_requires_grad, tanh_to_sigmoid

__all__ = ["SphericalOptimizer", "MultiScaleMaskedLoss", "geocross_loss", "normalize_noise_", "lr_schedule", "invert"]


class SphericalOptimizer(torch.optim.Adam):
    def __init__(self, params, **kwargs):
        params = list(params)
        super().__init__(params, **kwargs)
        self.params = params

    @torch.no_grad()
    def step(self, closure=None):
        loss = super().step(closure)
        for param in self.params:
            param.data.div_(param.pow(2).mean(dim=-1, keepdim=True).add(1e-9).sqrt())
        return loss


def _metric_of(loss_fn):
    """The kernels' metric name of a reference-style `loss_fn`; F.l1_loss and F.mse_loss (or a functools.partial of
    either without arguments of its own) only: there is no slow path behind the kernels."""
    fn = loss_fn
    if isinstance(fn, functools.partial) and not fn.args and not fn.keywords:
        fn = fn.func
    if fn is F.l1_loss:
        return "l1"
    if fn is F.mse_loss:
        return "mse"
    raise NotImplementedError(f"MultiScaleMaskedLoss: loss_fn must be torch.nn.functional.l1_loss or "
                              f"torch.nn.functional.mse_loss (the two the kernels implement), got {loss_fn!r}")


class MultiScaleMaskedLoss(torch.nn.Module):
    """reference: gans/inversion.py:32-76.  forward(gen, ref, mask) -> loss [B]; gen [B,C,H,W], mask [B,1,H,W].
    Only `gen` receives a gradient (the reference's callers pass constant targets).  The target's side (pyramid of ref,
    mask, norm, mask sums) is prepared once and cached on the module for the very `ref` / `mask` tensor OBJECTS it was
    computed from, at the versions they had (the rule of FourierFeature.encoded): the reference's call pattern -- the
    same targets on every one of a thousand steps -- prepares once, an in-place edit or another tensor prepares again.
    The entry keeps copies, not views, of its sources."""

    max_cached_targets = 4   # demo_inversion.py alternates two targets (depth, inverse depth) on one criterion

    def __init__(self, loss_fn, level=None, relative=True):
        super().__init__()
        self.pad = ops.Pad(padding=1, mode="replicate", ring=True)
        blur_kernel = torch.tensor([1, 2, 1], dtype=torch.float32)
        blur_kernel = torch.outer(blur_kernel, blur_kernel)
        blur_kernel /= blur_kernel.sum()
        self.register_buffer("blur_kernel", blur_kernel[None, None])      # state-dict layout of the reference; the
        mask_kernel = torch.ones_like(blur_kernel)                        # kernels carry these taps as constants
        self.register_buffer("mask_kernel", mask_kernel[None, None])
        self.metric = _metric_of(loss_fn)
        self.relative = bool(relative)
        self.level = level
        self._targets = []   # [(ref, mask, key, MsmlTarget)], most recent first

    def num_levels(self, H):
        level = int(np.log2(H)) if self.level is None else self.level
        return max(1, level)

    def prepared(self, ref, mask, levels):
        key = (ref._version, mask._version, tuple(ref.shape), levels, ref.device)
        for i, (r, m, k, t) in enumerate(self._targets):
            if r is ref and m is mask and k == key:
                if i:
                    self._targets.insert(0, self._targets.pop(i))
                return t
        if ref.requires_grad or mask.requires_grad:
            raise NotImplementedError("MultiScaleMaskedLoss: ref and mask are constants of the optimisation (only gen "
                                      "gets a gradient)")
        t = native.msml_prepare(ref, mask, levels)
        self._targets = [e for e in self._targets if not (e[0] is ref and e[1] is mask)]
        self._targets.insert(0, (ref, mask, key, t))
        del self._targets[self.max_cached_targets:]
        return t

    def forward(self, gen, ref, mask):
        _, C, H, W = gen.shape
        if tuple(ref.shape) != tuple(gen.shape):
            raise ValueError(f"MultiScaleMaskedLoss: gen {tuple(gen.shape)} and ref {tuple(ref.shape)} differ")
        target = self.prepared(ref, mask, self.num_levels(H))
        return native.msml_loss(gen, target, self.metric, self.relative)


def geocross_loss(latents):
    # PULSE
    B, N, D = latents.shape
    X = latents.view(B, 1, N, D)
    Y = latents.view(B, N, 1, D)
    A = ((X - Y).pow(2).sum(-1) + 1e-9).sqrt()
    B = ((X + Y).pow(2).sum(-1) + 1e-9).sqrt()
    D = 2 * torch.atan2(A, B)
    D = (D.pow(2) * D).mean((1, 2)) / 8.0
    return D


def normalize_noise_(noises):
    for noise in noises:
        mean = noise.mean()
        std = noise.std()
        noise.data.add_(-mean).div_(std)


def lr_schedule(iteration, num_steps, rampup_ratio=0.05, rampdown_ratio=0.25):
    """StyleGAN2's projector schedule (demo_inversion.py:147-152): cosine ramp-down, linear ramp-up."""
    t = iteration / num_steps
    gamma = min(1.0, (1.0 - t) / rampdown_ratio)
    gamma = 0.5 - 0.5 * np.cos(gamma * np.pi)
    gamma = gamma * min(1.0, t / rampup_ratio)
    return gamma


def invert(G, coord, depth, mask, *, latent_type="w", num_steps_1st=500, num_steps_2nd=500, lr_1st=5e-2, lr_2nd=5e-4,
           lr_1st_rampup_ratio=0.05, lr_1st_rampdown_ratio=0.25, optimize_phase=False, perturb_z=False,
           hypersphere_z=False, noise_ratio=0.75, noise_coef=0.05 / 10, generator=None, num_z_samples=10_000):
    """Fit a latent code (and a sensor phase) to measured scans, then tune the generator around it
    (demo_inversion.py:97-266 without the display code).

    G: a generator in eval mode on the device of `coord`; stage 2 (pivotal tuning) UPDATES ITS PARAMETERS in place.
    depth, mask [B,1,H,W]: metric depth and validity of B targets.  generator: the torch.Generator every random draw
    comes from (the latent samples behind the average latent, the initial z of latent_type "z", the optimised noise
    maps, the latent perturbation), made on the generator's device; None = torch's global generator of G's device.

    Returns {"latent": z (the optimised code: [B,D] for "z" / "w", [B,N,D] for "w+"), "phase" [B,2,1,1],
    "inv_depth", "inv_depth_orig", "raydrop_prob" [B,1,H,W] (the final images), "loss" [steps, B] (stage 1, then 2)}."""
    if latent_type not in ("z", "w", "w+"):
        raise ValueError(f"{latent_type=}")
    dev = coord.angle.device
    gdev = dev if generator is None else generator.device

    def randn(*shape):
        return torch.randn(*shape, generator=generator, device=gdev).to(dev)

    t_depth = depth.to(dev).float()
    t_mask = mask.to(dev).float().contiguous()
    B = len(t_depth)
    t_depth = coord.convert(t_depth, "depth", "depth_norm")
    t_inv_depth = coord.convert(t_depth, "depth_norm", "inv_depth_norm")
    t_inv_depth = t_inv_depth * t_mask

    # initialize a latent code
    with torch.no_grad():
        z_dim = G.mapping_network.in_ch
        z_samples = G.mapping_network(randn(num_z_samples, z_dim))
        z_avg = z_samples.mean(dim=0, keepdim=True)
        z_std = (((z_samples - z_avg) ** 2).sum() / num_z_samples).sqrt()
        if hypersphere_z:
            z_avg.div_(z_avg.pow(2).mean(dim=-1, keepdim=True).add(1e-9).sqrt())
    num_styles = G.synthesis_network.num_styles
    z_avg = z_avg.repeat_interleave(B, dim=0)
    if latent_type == "z":
        z = randn(B, z_dim)
    elif latent_type == "w":
        z = z_avg
    else:
        z = torch.stack([z_avg] * num_styles, dim=1)
    z = torch.nn.Parameter(z.contiguous()).requires_grad_()
    params_1st = [z]

    # the noise maps G holds (none for dusty_v2, which refuses use_noise)
    noises = []
    for m in G.modules():
        if isinstance(m, ops.NoiseInjection) and m.fixed_noise is not None:
            noise = randn(*m.fixed_noise.shape).float()
            m.fixed_noise = noise
            if len(noises) < 9:
                noise.requires_grad = True
                noises.append(noise)
    params_1st += noises

    phase = torch.nn.Parameter(torch.zeros((B, 2, 1, 1), device=dev)).requires_grad_()
    if optimize_phase:
        params_1st += [phase]

    criterion = MultiScaleMaskedLoss(loss_fn=F.l1_loss, level=2).to(dev)

    def forward(progress, perturb):
        if latent_type == "z":
            w = G.forward_mapping(z, None)
        elif latent_type == "w":
            w = torch.stack([z] * num_styles, dim=1)
        else:
            w = z
        if perturb:
            t = max(0.0, 1.0 - progress / noise_ratio)
            w = w + noise_coef * z_std * (t ** 2) * randn(*w.shape)
        imgs = G(w, angle=coord.angle + phase, input_w=True)
        g_inv_depth_orig = tanh_to_sigmoid(imgs["image_orig"])
        g_depth = coord.convert(g_inv_depth_orig, "inv_depth_norm", "depth_norm")
        loss = 0
        if latent_type == "w+":
            loss = loss + 5e-3 * geocross_loss(w)
        loss = loss + criterion(g_depth, t_depth, t_mask)
        loss = loss + criterion(g_inv_depth_orig, t_inv_depth, t_mask)
        return imgs, g_inv_depth_orig, loss

    losses = []

    def step(optim, progress, perturb):
        imgs, g_inv_depth_orig, loss = forward(progress, perturb)
        optim.zero_grad(set_to_none=True)
        loss.backward(gradient=torch.ones_like(loss))
        optim.step()
        losses.append(loss.detach())
        return imgs, g_inv_depth_orig

    imgs = g_inv_depth_orig = None
    # (1) gan inversion
    set_requires_grad(G, False)
    optim_cls = SphericalOptimizer if hypersphere_z else torch.optim.Adam
    optim_1st = optim_cls(params=params_1st, lr=lr_1st)
    scheduler = torch.optim.lr_scheduler.LambdaLR(
        optim_1st, lr_lambda=lambda it: lr_schedule(it, num_steps_1st, lr_1st_rampup_ratio, lr_1st_rampdown_ratio))
    for i in range(num_steps_1st):
        imgs, g_inv_depth_orig = step(optim_1st, i / num_steps_1st, perturb_z)
        scheduler.step()
        normalize_noise_(noises)

    # (2) pivotal tuning
    if num_steps_2nd > 0:
        set_requires_grad(G, True)
        optim_2nd = torch.optim.Adam(params=G.parameters(), lr=lr_2nd)
        for i in range(num_steps_2nd):
            imgs, g_inv_depth_orig = step(optim_2nd, i / num_steps_2nd, False)
            normalize_noise_(noises)

    out = {"latent": z.detach(), "phase": phase.detach(),
           "loss": torch.stack(losses) if losses else torch.zeros((0, B), device=dev)}
    if imgs is not None:
        out["inv_depth"] = tanh_to_sigmoid(imgs["image"]).detach()
        out["inv_depth_orig"] = g_inv_depth_orig.detach()
        out["raydrop_prob"] = torch.sigmoid(imgs["raydrop_logit"]).detach()
    return out
