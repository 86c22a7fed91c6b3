"""Sim2real ray-drop rendering: fit a trained generator to simulated scans and write one keep-probability map per scan,
the files semseg.datasets.GTALiDAR_GAN reads (the reference uses such maps -- "computed with DUSty v2" -- and has no
code that makes them; the arithmetic is stage 1 of demo_inversion.py:97-266).

LatentFitter is stage 1 of gans.inversion.invert as a dataset job: every buffer is allocated once, the average latent is
computed once (latent_prior), and everything after backward() -- the geocross term, the schedule, Adam, the hypersphere
projection, the loss row -- is ONE launch (native.latent_step) driven by device-resident step counters, so a whole step
(forward, backward, latent_step) can be replayed as a hipGraph.  render_raydrop_maps is the resumable walk over the
scans.  Out of scope, and refused rather than ignored: pivotal tuning (it would modify G per scan), latent perturbation,
noise-map optimisation."""
import gc
import inspect
import json
import os
import time
import warnings

import numpy as np
import torch

import dgv2_native as N

from .models import ops
from .models.ops import native
from .utils import tanh_to_sigmoid

__all__ = ["latent_prior", "LatentFitter", "render_raydrop_maps", "scan_list", "gan_path", "DEFAULT_GRAPH", "DEFAULT_BATCH_SIZE",
           "GEOCROSS_COEF"]

GEOCROSS_COEF = 5e-3       # demo_inversion.py:165, latent type "w+"
# both defaults are decisions of scripts/mb_sim2real.py (profiles/sim2real_mb.txt)
DEFAULT_GRAPH = True
DEFAULT_BATCH_SIZE = 32
_MSML_LEVELS = 2           # MultiScaleMaskedLoss(l1, level=2) of demo_inversion.py:139


def latent_prior(G, num_z_samples=10_000, generator=None):
    """(w_avg [1,D], w_std scalar tensor) of G's mapping network from `num_z_samples` draws, drawn exactly as
    gans.inversion.invert draws them (its first randn, on the generator's device): a fit that starts from this prior
    starts where invert starts."""
    dev = next(G.parameters()).device
    gdev = dev if generator is None else generator.device
    with torch.no_grad():
        z_dim = G.mapping_network.in_ch
        z_samples = G.mapping_network(torch.randn(num_z_samples, z_dim, generator=generator, device=gdev).to(dev))
        w_avg = z_samples.mean(dim=0, keepdim=True)
        w_std = (((z_samples - w_avg) ** 2).sum() / num_z_samples).sqrt()
    return w_avg, w_std


class LatentFitter:
    """Stage 1 of gans.inversion.invert for batch after batch of scans on one frozen generator.

    G: a generator in eval mode on the device of `coord`; its parameters are never modified (their requires_grad flags
    are cleared while a fit runs and restored afterwards).  prior: latent_prior(G, ...).  graph: capture one step as a
    hipGraph on its third call and replay it from then on (`captured` tells whether a graph is in use; a failed capture
    warns and the fitter goes on eagerly).  fit(depth, mask) -> {"latent", "phase" [B,2,1,1], "loss" [num_steps,B],
    "raydrop_prob", "inv_depth_orig" [B,1,H,W]} for up to batch_size scans."""

    def __init__(self, G, coord, batch_size, *, latent_type="w+", num_steps=500, lr=5e-2, rampup_ratio=0.05,
                 rampdown_ratio=0.25, optimize_phase=True, hypersphere=False, prior, graph=DEFAULT_GRAPH,
                 perturb_z=False, optimize_noise=False, num_steps_2nd=0, generator=None):
        if latent_type not in ("z", "w", "w+"):
            raise ValueError(f"{latent_type=}")
        if perturb_z:
            raise NotImplementedError("LatentFitter: latent perturbation (perturb_z) is not part of the dataset job")
        if optimize_noise or any(isinstance(m, ops.NoiseInjection) and m.fixed_noise is not None for m in G.modules()):
            raise NotImplementedError("LatentFitter: noise-map optimisation is not part of the dataset job (the "
                                      "generator holds fixed noise maps; use gans.inversion.invert)")
        if num_steps_2nd:
            raise NotImplementedError("LatentFitter: pivotal tuning would modify the generator per scan; use "
                                      "gans.inversion.invert")
        if int(batch_size) < 1 or int(num_steps) < 1:
            raise ValueError(f"LatentFitter: {batch_size=} and {num_steps=} must be positive")
        self.G, self.coord = G, coord
        self.B, self.num_steps = int(batch_size), int(num_steps)
        self.latent_type, self.lr = latent_type, float(lr)
        self.rampup_ratio, self.rampdown_ratio = float(rampup_ratio), float(rampdown_ratio)
        self.optimize_phase, self.hypersphere = bool(optimize_phase), bool(hypersphere)
        self.generator = generator
        self.graph = bool(graph)
        dev = self.device = coord.angle.device
        if dev.type != "cuda":
            raise RuntimeError("LatentFitter: the kernels have no CPU path")
        B, H, W = self.B, coord.H, coord.W
        self.num_styles = G.synthesis_network.num_styles
        D = self.D = G.synthesis_network.in_ch if latent_type != "z" else G.mapping_network.in_ch
        n = self.num_styles if latent_type == "w+" else 1
        self.geo_coef = GEOCROSS_COEF if latent_type == "w+" else 0.0

        w_avg, self.w_std = prior
        w_avg = w_avg.detach().to(dev).float().reshape(1, -1).clone()
        if hypersphere:
            w_avg.div_(w_avg.pow(2).mean(dim=-1, keepdim=True).add(1e-9).sqrt())
        self.w_avg = w_avg

        f = dict(device=dev, dtype=torch.float32)
        self.z = torch.zeros(B, n, D, **f).requires_grad_(True)
        self.m_z, self.v_z = torch.zeros(B, n, D, **f), torch.zeros(B, n, D, **f)
        self.phase = torch.zeros(B, 2, **f).requires_grad_(self.optimize_phase)
        self.m_p, self.v_p = torch.zeros(B, 2, **f), torch.zeros(B, 2, **f)
        self.step = torch.zeros(B, device=dev, dtype=torch.int32)
        self.loss_log = torch.zeros(self.num_steps, B, **f)
        self.geo = torch.zeros(B, **f)
        self._ones = torch.ones(B, **f)
        self.depth, self.mask = torch.zeros(B, 1, H, W, **f), torch.zeros(B, 1, H, W, **f)
        # the prepared targets the (captured) step reads: owned here, refreshed IN PLACE per batch.
        # MultiScaleMaskedLoss would cache a fresh MsmlTarget per tensor object and version, which a replayed graph
        # never sees.
        self._t_depth = native.msml_prepare(self.depth, self.mask, _MSML_LEVELS)
        self._t_inv = native.msml_prepare(self.depth, self.mask, _MSML_LEVELS)
        N.status_word(dev)   # must exist before a capture
        # the sampled image is not used (the objective reads image_orig, the result raydrop_logit): a constant Gumbel
        # uniform keeps the random generator out of the step
        self._g_kwargs = {}
        if "noise" in inspect.signature(G.forward).parameters:
            self._g_kwargs["noise"] = {"gumbel_u": torch.full((B, 1, H, W), 0.5, **f)}
        self._last = None    # (raydrop_logit, inv_depth_orig) of the latest forward
        self._graph, self._graph_tried, self._warm = None, False, 0
        self.steps_run = 0

    # ------------------------------------------------------------------ one batch
    @property
    def captured(self):
        return self._graph is not None

    @staticmethod
    def _refresh(owned, fresh):
        for name in ("refp", "maskp", "normp", "invm"):
            getattr(owned, name).copy_(getattr(fresh, name))

    @torch.no_grad()
    def _load(self, depth, mask):
        """Reset every buffer in place for a new batch of exactly B scans."""
        dev, coord = self.device, self.coord
        self.depth.copy_(depth.to(dev).float())
        self.mask.copy_(mask.to(dev).float())
        t_depth = coord.convert(self.depth, "depth", "depth_norm")
        t_inv = coord.convert(t_depth, "depth_norm", "inv_depth_norm") * self.mask
        self._refresh(self._t_depth, native.msml_prepare(t_depth, self.mask, _MSML_LEVELS))
        self._refresh(self._t_inv, native.msml_prepare(t_inv, self.mask, _MSML_LEVELS))
        if self.latent_type == "z":
            gdev = dev if self.generator is None else self.generator.device
            self.z.copy_(torch.randn(self.B, self.D, generator=self.generator, device=gdev).to(dev)[:, None])
        else:
            self.z.copy_(self.w_avg[:, None].expand_as(self.z))
        for t in (self.m_z, self.v_z, self.phase, self.m_p, self.v_p, self.step, self.loss_log, self.geo):
            t.zero_()

    def _step(self):
        """forward, backward, latent_step: no allocation that outlives the call except the images kept in _last, no
        host readback, no Python scalar that changes from step to step."""
        G, coord, z = self.G, self.coord, self.z
        if self.latent_type == "z":
            w = G.forward_mapping(z[:, 0], None)
        elif self.latent_type == "w":
            w = torch.stack([z[:, 0]] * self.num_styles, dim=1)
        else:
            w = z
        imgs = G(w, angle=coord.angle + self.phase[:, :, None, None], input_w=True, **self._g_kwargs)
        if "raydrop_logit" not in imgs:
            raise ValueError(f"LatentFitter: the output of {type(G).__name__} has no raydrop_logit (nothing to render)")
        inv = tanh_to_sigmoid(imgs["image_orig"])
        depth = coord.convert(inv, "inv_depth_norm", "depth_norm")
        loss = native.msml_loss(depth, self._t_depth, "l1", True) + native.msml_loss(inv, self._t_inv, "l1", True)
        params = [z, self.phase] if self.optimize_phase else [z]
        grads = torch.autograd.grad(loss, params, grad_outputs=self._ones)
        g_z = grads[0].contiguous()
        ph = dict(phase=self.phase.detach(), g_phase=grads[1].contiguous(), m_p=self.m_p, v_p=self.v_p) \
            if self.optimize_phase else {}
        native.latent_step(z.detach(), g_z, self.m_z, self.v_z, self.step, loss.detach(), self.loss_log, self.geo,
                           lr=self.lr, rampup_ratio=self.rampup_ratio, rampdown_ratio=self.rampdown_ratio,
                           geo_coef=self.geo_coef, hypersphere=self.hypersphere, **ph)
        self._last = (imgs["raydrop_logit"].detach(), inv.detach())

    def _capture(self):
        """Trainer._captured's recipe: a private pool, thread-local capture errors, no garbage collection meanwhile."""
        self._graph_tried = True
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        gc_was_enabled = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._step()
            self._graph = g
        except Exception as e:  # keep rendering: the step runs eagerly from now on
            torch.cuda.synchronize()
            warnings.warn(f"hipGraph capture of the latent-fitting step failed ({type(e).__name__}: {e}); running it "
                          f"eagerly")
            self._graph = None
        finally:
            if gc_was_enabled:
                gc.enable()

    def _advance(self):
        if self.graph and self._graph is None and not self._graph_tried:
            if self._warm < 2:
                self._warm += 1
            else:
                self._capture()   # records only: the replay below runs the step
        if self._graph is not None:
            self._graph.replay()
        else:
            self._step()
        self.steps_run += 1

    def fit(self, depth, mask):
        """depth, mask [b,1,H,W] (metric depth, validity), 1 <= b <= batch_size.  A short batch is padded by repeating
        its last scan; the padding is dropped from the result."""
        b = len(depth)
        if not 1 <= b <= self.B or tuple(depth.shape[1:]) != (1, self.coord.H, self.coord.W) \
                or tuple(mask.shape) != tuple(depth.shape):
            raise ValueError(f"LatentFitter.fit: depth / mask must be [b,1,{self.coord.H},{self.coord.W}] with b <= "
                             f"{self.B}, got {tuple(depth.shape)} / {tuple(mask.shape)}")
        if b < self.B:
            pad = [b - 1] * (self.B - b)
            depth, mask = torch.cat([depth, depth[pad]]), torch.cat([mask, mask[pad]])
        flags = [(p, p.requires_grad) for p in self.G.parameters()]
        for p, _ in flags:
            p.requires_grad_(False)
        try:
            self._load(depth, mask)
            for _ in range(self.num_steps):
                self._advance()
            logit, inv = self._last
            z = self.z.detach()
            out = {"latent": (z if self.latent_type == "w+" else z[:, 0])[:b].clone(),
                   "phase": self.phase.detach()[:b, :, None, None].clone(),
                   "loss": self.loss_log[:, :b].clone(),
                   "raydrop_prob": torch.sigmoid(logit[:b]),
                   "inv_depth_orig": inv[:b].clone()}
        finally:
            for p, flag in flags:
                p.requires_grad_(flag)
        return out


# ---------------------------------------------------------------------------------------
# the dataset walk
# ---------------------------------------------------------------------------------------
def scan_list(data_root, shard=(0, 1), limit=None, sim_dir="GTAV"):
    """The scans semseg.datasets.GTALiDAR lists (root/GTAV/*/*.npy, sorted), those whose index = shard[0] mod shard[1],
    the first `limit` of them."""
    from pathlib import Path
    i, n = (int(v) for v in shard)
    if not 0 <= i < n:
        raise ValueError(f"shard {i}/{n}: need 0 <= I < N")
    scans = sorted((Path(data_root) / sim_dir).glob("*/*.npy"))[i::n]
    return scans if limit is None else scans[:int(limit)]


def gan_path(scan, gan_dir, sim_dir="GTAV"):
    """The file GTALiDAR_GAN reads for `scan`: the same path with the simulation's directory name replaced."""
    return str(scan).replace(sim_dir, gan_dir)


def render_raydrop_maps(fitter, scans, out_paths, *, shape, min_depth, max_depth, batch_size, manifest=None,
                        depth_channel=3, log=None):
    """Fit every scan of `scans` ([H,W,5] .npy files, depth in channel 3) and write sigmoid(raydrop_logit) as float32
    [H,W] to the matching entry of `out_paths`.  A scan whose output exists is skipped; each file is written under a
    temporary name in its directory and renamed, so a killed run leaves no half-written map; one line per rendered scan
    (name, final loss, steps) is appended to `manifest`.  fitter: anything with fit(depth, mask) -> {"raydrop_prob"
    [b,1,H,W], "loss" [steps,b]}.  Returns {"rendered", "skipped", "mean_final_loss", "seconds", "scans_per_second"}."""
    from semseg.datasets.sqsg import _load_chw
    scans, out_paths = list(scans), [str(p) for p in out_paths]
    if len(scans) != len(out_paths):
        raise ValueError(f"render_raydrop_maps: {len(scans)} scans, {len(out_paths)} output paths")
    todo = [(s, o) for s, o in zip(scans, out_paths) if not os.path.exists(o)]
    skipped = len(scans) - len(todo)
    t0 = time.perf_counter()
    finals = []
    for start in range(0, len(todo), batch_size):
        chunk = todo[start:start + batch_size]
        depth = torch.stack([_load_chw(s, shape)[depth_channel] for s, _ in chunk])[:, None].float()
        mask = ((depth > min_depth) & (depth < max_depth)).float()
        out = fitter.fit(depth, mask)
        prob = out["raydrop_prob"].detach().float().cpu().numpy()
        loss = out["loss"].detach().float().cpu().numpy()
        if len(prob) != len(chunk):
            raise RuntimeError(f"render_raydrop_maps: the fitter returned {len(prob)} maps for {len(chunk)} scans")
        lines = []
        for i, (s, o) in enumerate(chunk):
            os.makedirs(os.path.dirname(o) or ".", exist_ok=True)
            tmp = f"{o}.tmp.{os.getpid()}"
            with open(tmp, "wb") as fh:
                np.save(fh, np.ascontiguousarray(prob[i, 0], dtype=np.float32))
            os.replace(tmp, o)
            final = float(loss[-1, i]) if len(loss) else float("nan")
            finals.append(final)
            lines.append(json.dumps({"name": os.path.relpath(o, os.path.dirname(manifest)) if manifest else o,
                                     "final_loss": final, "steps": int(len(loss))}))
        if manifest:
            os.makedirs(os.path.dirname(manifest) or ".", exist_ok=True)
            with open(manifest, "a") as fh:
                fh.write("".join(line + "\n" for line in lines))
        if log is not None:
            done = start + len(chunk)
            dt = time.perf_counter() - t0
            log(f"[{done}/{len(todo)}] final loss {np.mean(finals[-len(chunk):]):.5f}  {done / max(dt, 1e-9):.2f} scans/s")
    seconds = time.perf_counter() - t0
    return {"rendered": len(todo), "skipped": skipped,
            "mean_final_loss": float(np.mean(finals)) if finals and np.isfinite(finals).all() else None,
            "seconds": seconds, "scans_per_second": len(todo) / seconds if todo and seconds > 0 else 0.0}
