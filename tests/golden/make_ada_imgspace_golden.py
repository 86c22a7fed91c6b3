#!/usr/bin/env python3
"""Generate tests/golden/ada_imgspace.npz by running the REFERENCE's AdaptiveAugment.forward on CPU (build machine only).

    python tests/golden/make_ada_imgspace_golden.py

The reference tree is imported through _refshim, as make_golden.py does; what is written is data only.  Per case the
reference's forward runs with all 13 multipliers positive and p = 0.9, once in float32 -- recording every random draw in
call order (sample_affine's G, sample_color's C, then each torch.randn / torch.rand / torch.randn_like of lines 547-621)
-- and once in float64 REPLAYING those draws, so both precisions see the same augmentation.  Stored: the input, the
draws (G, C, the final band gains g, sigma, cut, eps), the float64 output (rounded to float32 for the 64x512 case: the
file stays under 1 MiB) and the reference's own float32-vs-float64 deviation (what the GPU tests derive their tolerance
from); for the two small cases also the float64 output of the geometric + colour stages alone (y_geo: the input of lines
547-621), the linear part J x = forward(x) - forward(0) (what a double backward returns) and a cotangent with the
reference's input gradient.

The final g is not a tensor the reference exposes (it goes straight into `g @ Hz_fbank`); it is rebuilt from the recorded
selects and log2-gains by tests/ada_imgspace_ref.band_gains, and the script asserts that the float64 restatement fed
with it reproduces the reference's float64 output, which pins it.  The multipliers of the three image-space stages are
below 1 (0.4 / 0.6 / 0.6) so that a batch of two or three samples can hold a sample with the stage on AND one with it
off; the script ASSERTS that conditioning before it writes anything.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refshim  # noqa: E402

_refshim.install()

import gans.augment.adaptive_augment as ref_ada  # noqa: E402
from gans.augment.adaptive_augment import AdaptiveAugment  # noqa: E402

import ada_imgspace_ref as R  # noqa: E402

torch.set_num_threads(8)
P = 0.9
POLICY = dict(lr_flip=1, ud_flip=1, int_trans=1, iso_scale=1, frac_trans=1, brightness=1, contrast=1, luma_flip=1, hue=1,
              saturation=1, imgfilter=0.4, noise=0.6, cutout=0.6)
CASES = [("a", (3, 1, 24, 96), True), ("b", (2, 1, 26, 64), True), ("c", (2, 1, 64, 512), False)]   # (tag, shape, with gradient)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


class Tape:
    """Records (replay=None) or replays the draws of one forward: G, C and every rand / randn / randn_like after them."""

    def __init__(self, A, replay=None):
        self.A, self.replay, self.rec, self.live, self.pos = A, replay, [], False, 0

    def _draw(self, kind, fn, *a, **k):
        if not self.live and kind not in ("G", "C"):
            return fn(*a, **k)
        if self.replay is None:
            v = fn(*a, **k)
            self.rec.append((kind, v.clone()))
            return v
        rk, v = self.replay[self.pos]
        self.pos += 1
        assert rk == kind, (rk, kind)
        return v.to(torch.get_default_dtype()).clone()

    def __enter__(self):
        self.saved = (torch.rand, torch.randn, torch.randn_like, self.A.sample_affine, self.A.sample_color)
        rand, randn, randn_like, aff, col = self.saved
        torch.rand = lambda *a, **k: self._draw("rand", rand, *a, **k)
        torch.randn = lambda *a, **k: self._draw("randn", randn, *a, **k)
        torch.randn_like = lambda *a, **k: self._draw("randn_like", randn_like, *a, **k)

        def sample_affine(*a, **k):
            return self._draw("G", aff, *a, **k)

        def sample_color(*a, **k):
            out = self._draw("C", col, *a, **k)
            self.live = True    # from here on every generator call belongs to lines 547-621
            return out

        self.A.sample_affine, self.A.sample_color = sample_affine, sample_color
        return self

    def __exit__(self, *exc):
        torch.rand, torch.randn, torch.randn_like = self.saved[:3]
        del self.A.sample_affine, self.A.sample_color
        self.live = False


def _mat3(rows):
    return torch.tensor(rows, dtype=torch.get_default_dtype())


# the reference pins its two constant-matrix helpers to float32, which refuses a float64 run; the same matrices in the
# default dtype (the float32 run is untouched: its default dtype IS float32)
ref_ada.scale2d_single = lambda s_x, s_y, device="cpu": _mat3(((s_x, 0, 0), (0, s_y, 0), (0, 0, 1)))
ref_ada.translate2d_single = lambda t_x, t_y, device="cpu": _mat3(((1, 0, t_x), (0, 1, t_y), (0, 0, 1)))


def reference_forward(x, dtype, seed=None, replay=None):
    """(y, tape records) of the reference's forward on x in `dtype`; sampling with `seed` or replaying `replay`."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        A = AdaptiveAugment(p_init=P, **POLICY).to(dtype)
        if seed is not None:
            torch.manual_seed(seed)
        with Tape(A, replay) as tape:
            y = A(x.to(dtype))
        if replay is not None:
            assert tape.pos == len(replay)
        return y, tape.rec, A
    finally:
        torch.set_default_dtype(prev)


def parse(rec, B):
    """The recorded call order of lines 547-621 -> named draws."""
    kinds = [k for k, _ in rec]
    assert kinds == ["G", "C"] + ["randn", "rand"] * 4 + ["randn", "rand", "randn_like", "rand", "rand"], kinds
    v = [t for _, t in rec]
    d = {"G": v[0], "C": v[1]}
    d["log2_gain"] = torch.stack([v[2 + 2 * i] for i in range(4)], dim=1)                       # [B,4]
    d["band_select"] = torch.stack([v[3 + 2 * i] for i in range(4)], dim=1) < np.float32(0.4) * np.float32(P)
    sig, sig_u, eps, cut_u, centre = v[10:15]
    d["noise_select"] = sig_u.reshape(B) < np.float32(0.6) * np.float32(P)
    d["sigma"] = torch.where(d["noise_select"], sig.reshape(B).double().abs() * 0.1, torch.zeros(B, dtype=torch.float64))
    d["eps"] = eps * d["noise_select"].view(B, 1, 1, 1)      # a sample with sigma = 0 never sees its field: stored as zeros
    d["cut_select"] = cut_u.reshape(B) < np.float32(0.6) * np.float32(P)
    size = torch.where(d["cut_select"], torch.full((B,), 0.5), torch.zeros(B))
    d["cut"] = torch.stack([centre.reshape(B, 2)[:, 0], centre.reshape(B, 2)[:, 1], size, size], dim=1)
    d["g"] = R.band_gains(d["band_select"], d["log2_gain"])
    return d


def conditioned(d, shape):
    """The fixture's promises (module docstring of tests/test_gpu_ada_imgspace.py)."""
    B, _, H, W = shape
    filt = d["band_select"].any(dim=1)
    for sel in (filt, d["noise_select"], d["cut_select"]):
        if not (bool(sel.any()) and bool((~sel).any())):
            return False
    if not bool(((d["G"][:, 0, 0] < 0) & filt).any()):        # a flipped sample goes through the filter
        return False
    keep = R.cutout_mask(d["cut"], H, W)
    removed = 1 - keep.mean(dim=(1, 2, 3))
    for b in range(B):
        if d["cut_select"][b] and not 0.05 <= float(removed[b]) <= 0.5:
            return False
    cut = d["cut"].double()
    for b in range(B):
        if not d["cut_select"][b]:
            continue
        dx = (((torch.arange(W) + 0.5) / W - cut[b, 0]).abs() - cut[b, 2] / 2).abs().min()
        dy = (((torch.arange(H) + 0.5) / H - cut[b, 1]).abs() - cut[b, 3] / 2).abs().min()
        if float(dx) < 1e-4 or float(dy) < 1e-4:                # the `>=` tie of the mask
            return False
    return True


def make_input(shape, seed):
    B, _, H, W = shape
    g = torch.Generator().manual_seed(seed)
    hh = torch.linspace(0, 1, H)[None, None, :, None]
    ww = torch.linspace(0, 2 * np.pi, W + 1)[None, None, None, :W]
    ph = torch.rand(B, 1, 1, 1, generator=g) * 6.28
    return (0.6 * torch.sin(2 * ww + ph) * (1 - 0.5 * hh) + 0.3 * hh - 0.2 + 0.25 * torch.randn(B, 1, H, W, generator=g)).float()


def main():
    out = {"cases": np.array([t for t, _, _ in CASES]), "p": np.float64(P),
           "policy.keys": np.array(list(POLICY)), "policy.values": np.array(list(POLICY.values()), dtype=np.float64)}
    for n, (tag, shape, with_grad) in enumerate(CASES):
        B, _, H, W = shape
        x = make_input(shape, 100 + n)
        for seed in range(1000 * n, 1000 * n + 1000):
            y32, rec, A = reference_forward(x, torch.float32, seed=seed)
            d = parse(rec, B)
            if conditioned(d, shape):
                break
        else:
            raise AssertionError(f"case {tag}: no seed meets the conditioning")
        assert conditioned(d, shape)
        x64 = x.double().requires_grad_(True)
        y64, _, A64 = reference_forward(x64, torch.float64, replay=rec)
        y0, _, _ = reference_forward(torch.zeros_like(x), torch.float64, replay=rec)
        lin = (y64 - y0).detach()
        # the float64 restatement with the stored draws reproduces the reference: this is what pins `g`
        fb = A64.Hz_fbank
        geo = AdaptiveAugment(p_init=P, **{**POLICY, "imgfilter": 0, "noise": 0, "cutout": 0}).double()
        prev = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)
        with Tape(geo, rec[:2]):
            y_geo = geo(x.double())
        torch.set_default_dtype(prev)
        mine = R.image_space_f64(y_geo, fb, g=d["g"], sigma=d["sigma"], cut=d["cut"], eps=d["eps"])
        dev_mine = rel(mine, y64.detach())
        assert dev_mine < 1e-12, (tag, dev_mine)
        dev = [rel(y32, y64.detach())]
        pre = f"{tag}."
        out.update({pre + "x": x, pre + "G": d["G"], pre + "C": d["C"], pre + "g": d["g"], pre + "sigma": d["sigma"],
                    pre + "cut": d["cut"], pre + "eps": d["eps"], pre + "y": y64.detach() if with_grad else y64.detach().float(),
                    pre + "band_select": d["band_select"], pre + "log2_gain": d["log2_gain"], pre + "seed": np.int64(seed)})
        if with_grad:
            cot = torch.randn(shape, generator=torch.Generator().manual_seed(500 + n))
            (g64,) = torch.autograd.grad(y64, x64, cot.double())
            x32 = x.clone().requires_grad_(True)
            y32g, _, _ = reference_forward(x32, torch.float32, replay=rec)
            (g32,) = torch.autograd.grad(y32g, x32, cot)
            y0_32, _, _ = reference_forward(torch.zeros_like(x), torch.float32, replay=rec)
            dev += [rel(g32, g64), rel((y32g - y0_32).detach(), lin)]
            out.update({pre + "cot": cot, pre + "grad": g64.float(), pre + "lin": lin.float(), pre + "y_geo": y_geo})
        out[pre + "dev"] = np.array(dev)
        print(f"case {tag} {shape}: seed {seed}, filter on {d['band_select'].any(1).tolist()}, noise {d['noise_select'].tolist()}, "
              f"cutout {d['cut_select'].tolist()}, flipped {(d['G'][:, 0, 0] < 0).tolist()}; restatement vs reference {dev_mine:.1e}; "
              f"reference fp32-vs-fp64 " + " ".join(f"{v:.2e}" for v in dev))
    out["Hz_fbank"] = fb.float()
    path = os.path.join(HERE, "ada_imgspace.npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()})
    size = os.path.getsize(path)
    assert size < 1024 * 1024, size
    print(f"ada_imgspace.npz: {size / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
