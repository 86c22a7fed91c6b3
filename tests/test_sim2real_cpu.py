"""CPU checks of sim2real ray-drop rendering (gans/sim2real.py, render_gan_noise.py, csrc/latent.hip's contract).
Needs the built library (the package imports dgv2_native), no GPU.

1. tests/sim2real_ref.latent_step_ref -- the float64 restatement the GPU test holds the kernel to -- against what it
   replaces: torch.optim.Adam (SphericalOptimizer) + LambdaLR + autograd through gans.inversion.geocross_loss, float64,
   six steps that cover lr = 0, ramp-up, the plateau and the ramp-down.  Bound 1e-12 relative to the largest magnitude:
   both sides are float64 evaluations of the same formulae in another order (rounding 1.1e-16 per operation, a few
   hundred operations per value, conditioning of the update <= 1e2).
2. the dataset walk with a stub fitter.
3. the ABI checks of test_abi.py with the new entry."""
import json
import os

import numpy as np
import pytest
import torch

import sim2real_ref as R
from conftest import ROOT

STEPS = 6
UP, DOWN = 0.34, 0.34   # of 6 steps: k = 0 (lr 0), 1-2 ramp-up, 3 plateau, 4-5 ramp-down


def _styles(kind, B, n, D, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        return torch.randn(B, n, D, generator=g, dtype=torch.float64)
    base = torch.randn(B, 1, D, generator=g, dtype=torch.float64)
    if kind == "identical":            # the start of every "w+" fit: N copies of the average latent
        return base.repeat(1, n, 1)
    raise ValueError(kind)


def _data_loss(z, phase, c, q):
    """A stand-in for the data terms: smooth, couples the styles, the samples and the phase.  -> [B]"""
    loss = ((z * c).sum(-1)).pow(2).sum(-1) + (z - 0.3).abs().mean((1, 2))
    if phase is not None:
        loss = loss + ((phase - q).pow(2) * (1 + z.mean((1, 2))[:, None].detach())).sum(-1)
    return loss


@pytest.mark.parametrize("kind", ["random", "identical"])
@pytest.mark.parametrize("with_phase,hypersphere", [(False, False), (True, False), (False, True)])
def test_ref_matches_adam_lambdalr_geocross(kind, with_phase, hypersphere):
    """(phase with the hypersphere has no reference: SphericalOptimizer also projects the phase, a row of one element,
    onto +-1; the kernel projects the rows of z only, include/dgv2.h.)"""
    from gans.inversion import SphericalOptimizer, geocross_loss, lr_schedule
    B, n, D = 2, 5, 24
    lr0, b1, b2, eps, coef = (R.f32(v) for v in (5e-2, 0.9, 0.999, 1e-8, 5e-3))
    z0 = _styles(kind, B, n, D, 5)
    if hypersphere:
        z0 = z0 / (z0.pow(2).mean(-1, keepdim=True) + 1e-9).sqrt()
    g = torch.Generator().manual_seed(11)
    c = torch.randn(B, n, D, generator=g, dtype=torch.float64) * 0.1
    q = torch.randn(B, 2, generator=g, dtype=torch.float64)

    # what the kernel replaces
    z = torch.nn.Parameter(z0.clone())
    phase = torch.nn.Parameter(torch.zeros(B, 2, dtype=torch.float64)) if with_phase else None
    params = [z] + ([phase] if with_phase else [])
    opt = (SphericalOptimizer if hypersphere else torch.optim.Adam)(params, lr=lr0, betas=(b1, b2), eps=eps)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda it: lr_schedule(it, STEPS, R.f32(UP), R.f32(DOWN)))

    # the restatement, fed the data gradient autograd produced
    st = {"z": z0.clone(), "m_z": torch.zeros_like(z0), "v_z": torch.zeros_like(z0),
          "step": torch.zeros(B, dtype=torch.int32), "loss_log": torch.zeros(STEPS, B, dtype=torch.float64),
          "geo": torch.zeros(B, dtype=torch.float64)}
    if with_phase:
        st.update(phase=torch.zeros(B, 2, dtype=torch.float64), m_p=torch.zeros(B, 2, dtype=torch.float64),
                  v_p=torch.zeros(B, 2, dtype=torch.float64))
    worst = 0.0

    def rel(a, b):
        return float((a - b).abs().max() / (b.abs().max() + 1e-300))

    for k in range(STEPS):
        total = coef * geocross_loss(z) + _data_loss(z, phase, c, q)
        opt.zero_grad(set_to_none=True)
        total.backward(gradient=torch.ones_like(total))
        zr = st["z"].clone().requires_grad_(True)
        pr = st["phase"].clone().requires_grad_(True) if with_phase else None
        data = _data_loss(zr, pr, c, q)
        grads = torch.autograd.grad(data.sum(), [zr] + ([pr] if with_phase else []))
        before = st["z"].clone()
        new = R.latent_step_ref(st["z"], grads[0], st["m_z"], st["v_z"], st["step"], data.detach(), st["loss_log"],
                                st["geo"], lr0=lr0, num_steps=STEPS, rampup_ratio=UP, rampdown_ratio=DOWN, beta1=b1,
                                beta2=b2, eps=eps, geo_coef=coef, hypersphere=hypersphere,
                                phase=st.get("phase"), g_phase=grads[1] if with_phase else None, m_p=st.get("m_p"),
                                v_p=st.get("v_p"))
        assert rel(new["g_z"], z.grad) <= 1e-12, (k, rel(new["g_z"], z.grad))
        opt.step()
        sched.step()
        st.update({key: new[key] for key in st})
        if k == 0 and not hypersphere:
            assert torch.equal(st["z"], before) and torch.equal(z.detach(), before)   # lr_schedule(0) = 0
            assert float(st["m_z"].abs().max()) > 0
        errs = {"z": rel(st["z"], z.detach()), "m": rel(st["m_z"], opt.state[z]["exp_avg"]),
                "v": rel(st["v_z"], opt.state[z]["exp_avg_sq"]), "loss": rel(st["loss_log"][k], total.detach()),
                "geo": rel(st["geo"], geocross_loss(before))}
        if with_phase:
            errs["phase"] = rel(st["phase"], phase.detach())
        worst = max(worst, *errs.values())
        assert all(e <= 1e-12 for e in errs.values()), (k, errs)
    assert st["step"].tolist() == [STEPS] * B
    again = R.latent_step_ref(st["z"], torch.ones_like(z0), st["m_z"], st["v_z"], st["step"], torch.ones(B),
                              st["loss_log"], st["geo"], lr0=lr0, num_steps=STEPS, geo_coef=coef)
    assert all(torch.equal(again[key], st[key]) for key in ("z", "m_z", "v_z", "step", "loss_log", "geo"))
    print(f"{kind} phase={with_phase} hypersphere={hypersphere}: worst relative deviation {worst:.2e}")


def test_identical_styles_have_the_exact_floor():
    """N equal styles: |x_i - x_j|^2 summed from the differences is exactly 0, so A = sqrt(1e-9) as in the reference."""
    from gans.inversion import geocross_loss
    x = _styles("identical", 1, 6, 32, 3)
    geo, grad = R.geocross_ref(x[0])
    assert abs(float(geo) - float(geocross_loss(x))) <= 1e-12 * float(geo)
    B2 = 4 * float(x[0, 0].pow(2).sum()) + 1e-9
    assert float(geo) == pytest.approx(float(torch.atan2(torch.tensor(1e-9).double().sqrt(), torch.tensor(B2).sqrt())) ** 3,
                                       rel=1e-12)


# ---------------------------------------------------------------------------------------
# the dataset walk
# ---------------------------------------------------------------------------------------
H, W = 8, 16
MIN_D, MAX_D = 1.45, 80.0


class StubFitter:
    """fit() -> a map that encodes the scan (its mean depth) and the mask it was given."""

    def __init__(self, batch_size):
        self.B, self.calls, self.masks, self.depths = batch_size, [], [], []

    def fit(self, depth, mask):
        assert 1 <= len(depth) <= self.B and tuple(depth.shape[1:]) == (1, H, W)
        self.calls.append(len(depth))
        self.masks.append(mask.clone())
        self.depths.append(depth.clone())
        prob = torch.sigmoid(depth.mean((1, 2, 3), keepdim=True) / 100).expand(-1, 1, H, W).clone()
        return {"raydrop_prob": prob, "loss": torch.full((3, len(depth)), 0.25)}


def _make_tree(root, n=5):
    rng = np.random.default_rng(0)
    paths = []
    for i in range(n):
        d = root / "GTAV" / f"seq{i % 2}"
        d.mkdir(parents=True, exist_ok=True)
        scan = rng.uniform(2, 60, size=(H, W, 5)).astype(np.float32)
        scan[0, 0, 3], scan[0, 1, 3], scan[0, 2, 3], scan[0, 3, 3] = MIN_D, MAX_D, 0.0, 95.0
        scan[0, 4, 3], scan[0, 5, 3] = np.nextafter(np.float32(MIN_D), np.float32(2)), np.nextafter(np.float32(MAX_D), np.float32(0))
        np.save(d / f"{i:04d}.npy", scan)
        paths.append(d / f"{i:04d}.npy")
    return sorted(paths)


def _walk(root, fitter, scans, batch_size=2, gan_dir="GTAV_noise_v2"):
    from gans.sim2real import gan_path, render_raydrop_maps
    outs = [gan_path(s, gan_dir) for s in scans]
    stats = render_raydrop_maps(fitter, scans, outs, shape=(H, W), min_depth=MIN_D, max_depth=MAX_D,
                                batch_size=batch_size, manifest=str(root / gan_dir / "manifest.jsonl"))
    return outs, stats


def _all_files(root):
    return sorted(str(p.relative_to(root)) for p in root.rglob("*") if p.is_file())


def test_walk_mirrors_paths_masks_pads_and_resumes(tmp_path):
    from gans.sim2real import scan_list
    paths = _make_tree(tmp_path)
    scans = scan_list(tmp_path)
    assert scans == paths
    fitter = StubFitter(2)
    outs, stats = _walk(tmp_path, fitter, scans)
    # path mirroring: the very file GTALiDAR_GAN opens
    for s, o in zip(scans, outs):
        assert o == str(s).replace("GTAV", "GTAV_noise_v2") and os.path.exists(o)
        m = np.load(o)
        assert m.dtype == np.float32 and m.shape == (H, W)
        want = torch.sigmoid(torch.from_numpy(np.load(s)[..., 3]).mean() / 100)
        assert np.allclose(m, float(want), atol=1e-6)      # each map belongs to its own scan
    # the last short batch: one scan goes in (the fitter pads), one map comes out
    assert fitter.calls == [2, 2, 1] and stats["rendered"] == 5 and stats["skipped"] == 0
    # the mask rule: min_depth < depth < max_depth, strict at both ends
    assert fitter.masks[0][0, 0, 0, :6].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0]
    assert float(fitter.depths[0][0, 0, 0, 3]) == 95.0        # the depth itself is handed over unmasked
    # no temporary file is left, the manifest has one line per rendered scan
    files = _all_files(tmp_path / "GTAV_noise_v2")
    assert len(files) == 6 and not [f for f in files if ".tmp" in f]
    lines = [json.loads(line) for line in open(tmp_path / "GTAV_noise_v2" / "manifest.jsonl")]
    assert len(lines) == 5 and {ln["name"] for ln in lines} == {os.path.relpath(o, tmp_path / "GTAV_noise_v2") for o in outs}
    assert all(ln["final_loss"] == 0.25 and ln["steps"] == 3 for ln in lines)
    json.dumps(stats, allow_nan=False)

    # a second run skips everything and touches nothing
    mtimes = {o: os.stat(o).st_mtime_ns for o in outs}
    fitter2 = StubFitter(2)
    _, stats2 = _walk(tmp_path, fitter2, scans)
    assert stats2["rendered"] == 0 and stats2["skipped"] == 5 and fitter2.calls == []
    assert {o: os.stat(o).st_mtime_ns for o in outs} == mtimes
    assert len(open(tmp_path / "GTAV_noise_v2" / "manifest.jsonl").readlines()) == 5

    # after deleting one map exactly that one is rendered
    os.remove(outs[3])
    fitter3 = StubFitter(2)
    _, stats3 = _walk(tmp_path, fitter3, scans)
    assert stats3["rendered"] == 1 and stats3["skipped"] == 4 and fitter3.calls == [1]
    assert {o: os.stat(o).st_mtime_ns for o in outs if o != outs[3]} == {o: t for o, t in mtimes.items() if o != outs[3]}
    assert len(open(tmp_path / "GTAV_noise_v2" / "manifest.jsonl").readlines()) == 6


def test_shards_partition_the_list(tmp_path):
    import render_gan_noise
    from gans.sim2real import scan_list
    _make_tree(tmp_path)
    every = scan_list(tmp_path)
    parts = []
    for text in ("0/2", "1/2"):
        args = render_gan_noise.parse(["--ckpt_path", "x", "--shard", text])
        parts.append(scan_list(tmp_path, args.shard))
    assert parts[0] == every[0::2] and parts[1] == every[1::2]
    assert sorted(parts[0] + parts[1]) == every and not set(parts[0]) & set(parts[1])
    assert scan_list(tmp_path, (0, 1), limit=3) == every[:3]
    for bad in ("2/2", "-1/2", "1", "a/b"):
        with pytest.raises(SystemExit):
            render_gan_noise.parse(["--ckpt_path", "x", "--shard", bad])
    # both shards through the walk: together they render every scan once
    for part in parts:
        _walk(tmp_path, StubFitter(2), part)
    assert len([f for f in _all_files(tmp_path / "GTAV_noise_v2") if f.endswith(".npy")]) == 5


def test_walk_refuses_a_fitter_that_returns_the_padding(tmp_path):
    scans = _make_tree(tmp_path, 1)

    class Padded(StubFitter):
        def fit(self, depth, mask):
            out = super().fit(depth, mask)
            return {k: torch.cat([v, v], dim=0 if k == "raydrop_prob" else 1) for k, v in out.items()}
    with pytest.raises(RuntimeError):
        _walk(tmp_path, Padded(2), scans)
    assert not [f for f in _all_files(tmp_path) if "noise" in f and f.endswith(".npy")]


def test_frontal_angle_grid_is_the_simulators():
    from gans.coords import CoordBridge, frontal_angle_grid
    from semseg.datasets.sqsg import SyntheticFrontal
    grid = frontal_angle_grid(8, 32)
    assert grid.shape == (8, 32, 2) and grid.dtype == np.float32
    dirs = SyntheticFrontal(length=1, shape=(8, 32))._dirs
    e, a = grid[..., 0].astype(np.float64), grid[..., 1].astype(np.float64)
    assert np.allclose(np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)]), dirs, atol=1e-6)
    coord = CoordBridge(8, 32, MIN_D, MAX_D, angle_array=grid)        # same size: the bridge keeps the grid as it is
    assert np.allclose(coord.angle[0].permute(1, 2, 0).numpy(), grid, atol=1e-6)


def test_fitter_refuses_what_it_does_not_do():
    from gans.sim2real import LatentFitter
    for kw in ({"perturb_z": True}, {"optimize_noise": True}, {"num_steps_2nd": 10}):
        with pytest.raises(NotImplementedError):
            LatentFitter(torch.nn.Linear(1, 1), None, 2, prior=None, **kw)
    with pytest.raises(ValueError):
        LatentFitter(torch.nn.Linear(1, 1), None, 2, prior=None, latent_type="x")


# ---------------------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------------------
def test_abi_checks_hold_with_the_new_entry():
    import dgv2_native as N
    import test_abi
    protos = test_abi.parse_header()
    assert "dgv2_latent_step" in protos and "dgv2_latent_step" in N.SIGNATURES
    assert "dgv2_latent_step_scratch" not in protos and N.ABI_VERSION == 60
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_binding_matches_header()
    test_abi.test_header_cites_reference_interfaces()
    src = open(os.path.join(ROOT, "include", "dgv2.h")).read()
    assert "inversion.py:10-20,81-90" in src and "demo_inversion.py:147-152" in src


def test_wrapper_is_part_of_the_package_and_checks_its_arguments():
    from gans.models.ops import native
    assert native.latent_step is native.latent.latent_step
    z = torch.zeros(2, 1, 8)
    i32 = torch.zeros(2, dtype=torch.int32)
    v, log = torch.zeros(2), torch.zeros(4, 2)
    with pytest.raises(RuntimeError):      # CPU tensors: no fallback
        native.latent_step(z, z.clone(), z.clone(), z.clone(), i32, v, log, v.clone(), lr=0.1)
    with pytest.raises(ValueError):        # geocross needs two styles
        native.latent_step(z, z.clone(), z.clone(), z.clone(), i32, v, log, v.clone(), lr=0.1, geo_coef=5e-3)
    with pytest.raises(ValueError):        # phase buffers go together
        native.latent_step(z, z.clone(), z.clone(), z.clone(), i32, v, log, v.clone(), lr=0.1, phase=torch.zeros(2, 2))
    with pytest.raises(ValueError):        # int64 counters
        native.latent_step(z, z.clone(), z.clone(), z.clone(), i32.long(), v, log, v.clone(), lr=0.1)
    with pytest.raises(ValueError):        # more than the LDS holds
        big = torch.zeros(1, 2, 8193)
        native.latent_step(big, big, big, big, i32[:1], v[:1], log[:, :1], v[:1], lr=0.1)
