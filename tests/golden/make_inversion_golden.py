#!/usr/bin/env python3
"""Generate tests/golden/inversion.npz by running the REFERENCE's inversion code on CPU (build machine only).

    python tests/golden/make_inversion_golden.py

The reference tree is imported through _refshim, as make_golden.py does; what is written is data only: seeded inputs
and the reference's outputs / gradients, evaluated in float64 and in float32 (the per-case deviation between the two is
what the GPU tests derive their tolerance from).  The script ASSERTS that its inputs keep the reference itself
well-conditioned before it writes anything.
"""
import copy
import os
import pickle
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refshim  # noqa: E402

_refshim.install()

from gans.coords import CoordBridge  # noqa: E402
from gans.inversion import MultiScaleMaskedLoss, SphericalOptimizer, geocross_loss  # noqa: E402
from gans.models.builder import build_generator  # noqa: E402
from gans.utils import tanh_to_sigmoid  # noqa: E402

torch.set_num_threads(8)
F = torch.nn.functional
MIN_DEPTH, MAX_DEPTH = 1.45, 80.0


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ----------------------------------------------------------------------------
def msml_inputs(shape, seed, hole):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(B, 1, H, W, generator=g) < 0.85).float()
    if hole is not None:
        b, h0, h1, w0, w1 = hole
        mask[b, :, h0:h1, w0:w1] = 0.0          # large enough that a level-1 window sees no valid pixel
    mask[0, 0, 3, 5] = 1.0
    ref = (0.05 + 0.95 * torch.rand(B, C, H, W, generator=g)) * mask      # demo_inversion.py:95: zero outside the mask
    gen = ref * (1.0 + 0.2 * torch.randn(B, C, H, W, generator=g)) + 0.05 * torch.randn(B, C, H, W, generator=g)
    gen[0, 0, 3, 5] = ref[0, 0, 3, 5]           # the one planted tie (sign(0) = 0 for l1)
    # conditioning
    assert bool(((ref >= 0.05) | (mask.expand_as(ref) == 0)).all()) and bool((ref[mask.expand_as(ref) == 0] == 0).all())
    ties = ((gen == ref) & (mask.expand_as(ref) == 1)).sum()
    assert int(ties) == 1, int(ties)
    if hole is not None:
        crit = MultiScaleMaskedLoss(F.l1_loss, level=2)
        _, m1 = crit.update_mask(mask)
        assert bool((m1[hole[0]] == 0).any()), "no empty level-1 window"
    return gen, ref, mask


def msml_case(gen, ref, mask, loss_fn, level, relative, dtype):
    crit = MultiScaleMaskedLoss(loss_fn, level=level, relative=relative).to(dtype)
    x = gen.to(dtype).clone().requires_grad_(True)
    loss = crit(x, ref.to(dtype), mask.to(dtype))
    (g,) = torch.autograd.grad(loss.sum(), x)
    return loss.detach(), g


def golden_msml(out):
    names = []
    sets = {"a": msml_inputs((3, 1, 16, 64), 11, (1, 4, 11, 8, 26)), "b": msml_inputs((2, 2, 8, 32), 12, (0, 2, 7, 4, 14))}
    for s, (gen, ref, mask) in sets.items():
        out[f"msml.{s}.gen"], out[f"msml.{s}.ref"], out[f"msml.{s}.mask"] = gen, ref, mask
    cases = [("a", fn, rl, lv) for fn in ("l1", "mse") for rl in (1, 0) for lv in (1, 2, 0)] + [("b", "l1", 1, 0)]
    for s, fn, rl, lv in cases:
        gen, ref, mask = sets[s]
        loss_fn = {"l1": F.l1_loss, "mse": F.mse_loss}[fn]
        level = None if lv == 0 else lv
        l64, g64 = msml_case(gen, ref, mask, loss_fn, level, bool(rl), torch.float64)
        l32, g32 = msml_case(gen, ref, mask, loss_fn, level, bool(rl), torch.float32)
        name = f"{s}.{fn}.rel{rl}.level{lv}"
        dl, dg = rel(l32, l64), rel(g32, g64)
        assert dl < 1e-5, (name, dl)      # the inputs hide nothing: the reference agrees with itself
        names.append(name)
        out[f"msml.{name}.loss"] = l64
        out[f"msml.{name}.grad"] = g64.float()
        out[f"msml.{name}.dev"] = np.array([dl, dg])
        print(f"msml {name}: loss {l64.tolist()} ref fp32-vs-fp64 loss {dl:.2e} grad {dg:.2e}")
    out["msml.cases"] = np.array(names)
    crit = MultiScaleMaskedLoss(F.l1_loss, level=2)
    out["msml.state_dict_keys"] = np.array(list(crit.state_dict().keys()))
    out["msml.buffer_names"] = np.array([k for k, _ in crit.named_buffers()])
    for k, v in crit.state_dict().items():
        out[f"msml.state_dict.{k}"] = v


# ----------------------------------------------------------------------------
def golden_host(out):
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(2, 6, 32, generator=g).double().requires_grad_(True)
    v = geocross_loss(lat)
    (gl,) = torch.autograd.grad(v.sum(), lat)
    out["geocross.latents"], out["geocross.value"], out["geocross.grad"] = lat.detach().float(), v.detach(), gl
    # SphericalOptimizer: three steps with seeded gradients
    p = torch.nn.Parameter(torch.randn(2, 6, 32, generator=g))
    out["spherical.p0"] = p.detach().clone()
    opt = SphericalOptimizer([p], lr=0.05)
    grads = torch.randn(3, 2, 6, 32, generator=g)
    for i in range(3):
        p.grad = grads[i].clone()
        opt.step()
    out["spherical.grads"], out["spherical.p3"] = grads, p.detach().clone()
    # demo_inversion.py:147-152 through torch's LambdaLR, as the demo drives it
    for tag, n, up, down in (("a", 20, 0.05, 0.25), ("b", 500, 0.05, 0.25)):
        def lr_schedule(iteration, n=n, up=up, down=down):
            t = iteration / n
            gamma = min(1.0, (1.0 - t) / down)
            gamma = 0.5 - 0.5 * np.cos(gamma * np.pi)
            return gamma * min(1.0, t / up)
        q = torch.nn.Parameter(torch.zeros(1))
        o = torch.optim.Adam([q], lr=1.0)
        sch = torch.optim.lr_scheduler.LambdaLR(o, lr_lambda=lr_schedule)
        lrs = []
        for _ in range(n):
            lrs.append(o.param_groups[0]["lr"])
            o.step()
            sch.step()
        out[f"lr.{tag}"] = np.array([n, up, down])
        out[f"lr.{tag}.values"] = np.array(lrs)


# ----------------------------------------------------------------------------
PAIRS = [("depth", "inv_depth_norm"), ("depth", "inv_depth"), ("depth", "point_map"), ("depth_norm", "inv_depth_norm"),
         ("depth_norm", "point_map"), ("inv_depth_norm", "depth"), ("inv_depth_norm", "depth_norm"),
         ("inv_depth_norm", "point_map"), ("inv_depth", "depth"), ("inv_depth", "depth_norm")]


def small_angle_file():
    rng = np.random.RandomState(0)
    elev = np.linspace(0.035, -0.43, 16)[:, None] + rng.randn(16, 96) * 1e-3
    azim = np.linspace(np.pi, -np.pi, 96, endpoint=False)[None, :] + rng.randn(16, 96) * 1e-3
    return np.stack([elev, azim], axis=-1).astype(np.float32)


def coord_bridge(angle_file, H=16, W=64):
    tmp = "/tmp/_dgv2_inversion_angle.npy"
    np.save(tmp, angle_file)
    return CoordBridge(num_ring=H, num_points=W, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, angle_file=tmp)


def away_from(x, thresholds, margin):
    for t in thresholds:
        near = (x - t).abs() < margin
        x = torch.where(near, torch.full_like(x, t + 2 * margin), x)
    return x


def golden_coords(out, cb):
    g = torch.Generator().manual_seed(21)
    depth = torch.rand(2, 1, 16, 64, generator=g) * 95.0 - 2.0      # some below min_depth / 0, some beyond max_depth
    # every source at least 1e-3 (in its own units) away from every threshold of get_mask on its way
    ths = {"depth": (0.0, MIN_DEPTH, MAX_DEPTH), "depth_norm": (0.0, MIN_DEPTH / MAX_DEPTH, 1.0),
           "inv_depth_norm": (0.0, MIN_DEPTH / MAX_DEPTH, 1.0), "inv_depth": (0.0, 1.0 / MAX_DEPTH, 1.0 / MIN_DEPTH)}
    src = {"depth": depth, "depth_norm": depth / MAX_DEPTH,
           "inv_depth_norm": torch.rand(2, 1, 16, 64, generator=g) * 1.2 - 0.1,
           "inv_depth": torch.rand(2, 1, 16, 64, generator=g) * 0.8 - 0.05}
    for k in src:
        src[k] = away_from(src[k], ths[k], 1e-3)
        for t in ths[k]:
            assert float((src[k] - t).abs().min()) >= 1e-3, (k, t, float((src[k] - t).abs().min()))
        out[f"coords.src.{k}"] = src[k]
    out["coords.pairs"] = np.array([f"{a}>{b}" for a, b in PAIRS])
    for a, b in PAIRS:
        res = {}
        for dt in (torch.float64, torch.float32):
            c = copy.deepcopy(cb).to(dt)
            x = src[a].to(dt).clone().requires_grad_(True)
            y = c.convert(x, a, b)
            r = torch.randn(y.shape, generator=torch.Generator().manual_seed(31)).to(dt)
            (gx,) = torch.autograd.grad((y * r).sum(), x)
            res[dt] = (y.detach(), gx, r)
        (y64, g64, r), (y32, g32, _) = res[torch.float64], res[torch.float32]
        out[f"coords.{a}>{b}.cot"] = r.float()
        out[f"coords.{a}>{b}.value"] = y64.float()
        out[f"coords.{a}>{b}.grad"] = g64.float()
        out[f"coords.{a}>{b}.dev"] = np.array([rel(y32, y64), rel(g32, g64)])
        print(f"coords {a}>{b}: ref fp32-vs-fp64 value {rel(y32, y64):.2e} grad {rel(g32, g64):.2e}")


# ----------------------------------------------------------------------------
class _Node:
    def __setstate__(self, state):
        self.__dict__.update(state if isinstance(state, dict) else state[1] or {})


class _CfgUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module.startswith("omegaconf"):
            return type(name, (_Node,), {"__module__": module})
        return super().find_class(module, name)


class _CfgPickle:
    __name__ = "cfg_pickle"
    Unpickler = _CfgUnpickler
    load = staticmethod(lambda f, **kw: _CfgUnpickler(f, **kw).load())


def _plain(n):
    if isinstance(n, _Node):
        d = n.__dict__
        if "_content" in d:
            return _plain(d["_content"])
        return _plain(d.get("_val"))
    if isinstance(n, dict):
        return {(_plain(k) if not isinstance(k, str) else k): _plain(v) for k, v in n.items()}
    if isinstance(n, (list, tuple)):
        return [_plain(v) for v in n]
    return n


NUM_Z, STEPS_1, STEPS_2, LR_1, LR_2, SEED = 512, 20, 10, 5e-2, 5e-4, 77


def reference_invert(G, coord, depth, mask, dtype):
    """demo_inversion.py:84-266 for latent_type "w+", phase optimised, no perturb_z, no hypersphere, without display.
    dtype: of the latent, the phase, the targets, the conversion and the loss.  The reference's generator itself stays
    float32 (its synthesis network casts its output to float32 and RayDropModel lerps against it: float64 is refused)."""
    G = copy.deepcopy(G).eval()
    coord = copy.deepcopy(coord).to(dtype)
    t_depth, t_mask = depth.to(dtype), mask.to(dtype)
    B = len(t_depth)
    t_depth = coord.convert(t_depth, "depth", "depth_norm")
    t_inv_depth = coord.convert(t_depth, "depth_norm", "inv_depth_norm")
    t_inv_depth *= t_mask
    with torch.no_grad():
        z_samples = torch.randn(NUM_Z, 32, generator=torch.Generator().manual_seed(SEED))
        z_samples = G.mapping_network(z_samples).to(dtype)
        z_avg = z_samples.mean(dim=0, keepdim=True)
    z_avg = z_avg.repeat_interleave(B, dim=0)
    z = torch.stack([z_avg] * G.synthesis_network.num_styles, dim=1)
    z = torch.nn.Parameter(z).requires_grad_()
    phase = torch.nn.Parameter(torch.zeros((B, 2, 1, 1), dtype=dtype)).requires_grad_()
    criterion = MultiScaleMaskedLoss(loss_fn=F.l1_loss, level=2).to(dtype)

    def lr_schedule(iteration):
        t = iteration / STEPS_1
        gamma = min(1.0, (1.0 - t) / 0.25)
        gamma = 0.5 - 0.5 * np.cos(gamma * np.pi)
        return gamma * min(1.0, t / 0.05)

    def forward():
        imgs = G(z.float(), angle=(coord.angle + phase).float(), input_w=True)
        g_inv_depth_orig = tanh_to_sigmoid(imgs["image_orig"].to(dtype))
        g_depth = coord.convert(g_inv_depth_orig, "inv_depth_norm", "depth_norm")
        loss = 5e-3 * geocross_loss(z)
        loss += criterion(g_depth, t_depth, t_mask)
        loss += criterion(g_inv_depth_orig, t_inv_depth, t_mask)
        return loss

    losses = []
    for p in G.parameters():
        p.requires_grad = False
    optim_1st = torch.optim.Adam(params=[z, phase], lr=LR_1)
    scheduler = torch.optim.lr_scheduler.LambdaLR(optim_1st, lr_lambda=lr_schedule)
    for _ in range(STEPS_1):
        loss = forward()
        optim_1st.zero_grad(set_to_none=True)
        loss.backward(gradient=torch.ones_like(loss))
        optim_1st.step()
        scheduler.step()
        losses.append(loss.detach())
    for p in G.parameters():
        p.requires_grad = True
    optim_2nd = torch.optim.Adam(params=G.parameters(), lr=LR_2)
    for _ in range(STEPS_2):
        loss = forward()
        optim_2nd.zero_grad(set_to_none=True)
        loss.backward(gradient=torch.ones_like(loss))
        optim_2nd.step()
        losses.append(loss.detach())
    return torch.stack(losses), z.detach(), phase.detach()


def golden_invert(out, cb):
    ck = torch.load(os.path.join(HERE, "checkpoint_small.pth"), map_location="cpu", weights_only=False,
                    pickle_module=_CfgPickle)
    cfg = _refshim.to_attr(_plain(ck["cfg"]))
    G = build_generator(cfg.model.generator)
    G.load_state_dict(ck["G_ema"])
    G.eval()
    # targets: a smooth synthetic scene well inside the valid range, with dropped rays
    g = torch.Generator().manual_seed(41)
    H, W = 16, 64
    hh = torch.linspace(0, 1, H)[None, None, :, None]
    ww = torch.linspace(0, 2 * np.pi, W + 1)[None, None, None, :W]
    ph = torch.tensor([0.3, 1.7])[:, None, None, None]
    depth = 10.0 + 30.0 * hh + 6.0 * torch.sin(2 * ww + ph) * (1 - hh) + 0.5 * torch.rand(2, 1, H, W, generator=g)
    mask = (torch.rand(2, 1, H, W, generator=g) < 0.9).float()
    assert float(depth.min()) > MIN_DEPTH + 1 and float(depth.max()) < MAX_DEPTH - 1
    l64, z64, p64 = reference_invert(G, cb, depth, mask, torch.float64)
    l32, z32, p32 = reference_invert(G, cb, depth, mask, torch.float32)
    dev = ((l32.double() - l64).abs() / l64.abs()).max(dim=1).values
    print("invert: loss first", l64[0].tolist(), "last", l64[-1].tolist())
    print("invert: ref fp32-vs-fp64 per step", " ".join(f"{v:.1e}" for v in dev.tolist()))
    assert float(dev[0]) < 1e-5, float(dev[0])
    assert bool((l64[-1] < l64[0]).all())
    out.update({"invert.depth": depth, "invert.mask": mask, "invert.loss": l64, "invert.loss_dev": dev,
                "invert.latent": z64.float(), "invert.phase": p64.float(),
                "invert.cfg": np.array([NUM_Z, STEPS_1, STEPS_2, LR_1, LR_2, SEED])})


def main():
    out = {}
    angle_file = small_angle_file()
    cb = coord_bridge(angle_file)
    out["angle_file"] = angle_file
    golden_msml(out)
    golden_host(out)
    golden_coords(out, cb)
    golden_invert(out, cb)
    path = os.path.join(HERE, "inversion.npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                                 for k, v in out.items()})
    print(f"inversion.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
