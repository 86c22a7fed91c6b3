"""Sim2real ray-drop rendering on the GPU: dgv2_latent_step (csrc/latent.hip) against tests/sim2real_ref.py, the fitter
(gans/sim2real.py) against the reference trajectory of tests/golden/inversion.npz, graph replay against eager runs, and
render_gan_noise.py end to end.

Tolerance rule of the kernel test (the one of tests/test_gpu_inversion.py): a result may differ from the float64
restatement by 1e-5 relative to the largest expected magnitude plus twice the deviation of the FLOAT32 torch restatement
of the same case from float64, which the test measures.

Measured on an MI355X: kernel, 102 cases, worst error / bound 0.038; first five losses of the
fitter 4.6e-8 .. 1.4e-7 from the reference's float64 trajectory, 1.30 % at step 19; eager fits differ by 2e-6 .. 3e-6
from run to run after 8 steps and graph replay agrees within twice that; a stage-1 step is 458 device launches in
invert and 389 in the fitter at 16 x 64.  The file runs in about 8 s, 5 s of it the profiler's first use."""
import json
import os

import numpy as np
import pytest
import torch

import sim2real_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
NUM_STEPS = 40                      # rampup 0.05: k = 1 ramps up; rampdown 0.25: k >= 31 ramps down
COUNTERS = (0, 1, 20, 35, NUM_STEPS - 1, NUM_STEPS)
SHAPES = ((3, 10, 512), (1, 1, 512), (2, 2, 64), (2, 10, 500))
STYLES = ("random", "identical", "near", "antipodal")
OUT_KEYS = ("z", "g_z", "m_z", "v_z", "phase", "m_p", "v_p", "loss_log", "geo")
SENTINEL = 7.0


def make_case(B, n, D, style, with_phase, counters, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, n, D, generator=g)
    if style != "random" and n > 1:
        z = z[:, :1].repeat(1, n, 1)
        if style == "near":
            z = z * (1 + 1e-4 * torch.randn(B, n, D, generator=g))
        elif style == "antipodal":
            z = torch.randn(B, n, D, generator=g)
            z[:, 1] = -z[:, 0]
    c = {"z": z.contiguous(), "g_z": torch.randn(B, n, D, generator=g) * 0.1,
         "m_z": torch.randn(B, n, D, generator=g) * 0.05, "v_z": torch.rand(B, n, D, generator=g) * 0.01,
         "step": torch.tensor([counters[i % len(counters)] for i in range(B)], dtype=torch.int32),
         "loss_terms": torch.rand(B, generator=g) * 10, "loss_log": torch.full((NUM_STEPS, B), SENTINEL),
         "geo": torch.full((B,), SENTINEL)}
    if with_phase:
        c.update(phase=torch.randn(B, 2, generator=g) * 0.01, g_phase=torch.randn(B, 2, generator=g),
                 m_p=torch.randn(B, 2, generator=g) * 0.1, v_p=torch.rand(B, 2, generator=g))
    return c


def run_ref(c, dtype, **kw):
    return R.latent_step_ref(c["z"], c["g_z"], c["m_z"], c["v_z"], c["step"], c["loss_terms"], c["loss_log"], c["geo"],
                             num_steps=NUM_STEPS, phase=c.get("phase"), g_phase=c.get("g_phase"), m_p=c.get("m_p"),
                             v_p=c.get("v_p"), dtype=dtype, **kw)


def run_kernel(c, lr0=5e-2, geo_coef=0.0, hypersphere=False, rampup_ratio=0.05, rampdown_ratio=0.25):
    from gans.models.ops import native
    d = {k: v.to(DEV).clone() for k, v in c.items()}
    ph = {k: d[k] for k in ("phase", "g_phase", "m_p", "v_p") if k in d}
    native.latent_step(d["z"], d["g_z"], d["m_z"], d["v_z"], d["step"], d["loss_terms"], d["loss_log"], d["geo"],
                       lr=lr0, rampup_ratio=rampup_ratio, rampdown_ratio=rampdown_ratio, geo_coef=geo_coef,
                       hypersphere=hypersphere, **ph)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


# ---------------------------------------------------------------------------------------
# 1. the kernel against the float64 restatement
# ---------------------------------------------------------------------------------------
def test_latent_step_matches_reference():
    worst, bad, ncases = (0.0, None), [], 0
    for si, (B, n, D) in enumerate(SHAPES):
        for style in (STYLES if n > 1 else STYLES[:1]):
            for with_phase in (False, True):
                for hypersphere in (False, True):
                    for geo_coef in ((0.0, 5e-3) if n > 1 else (0.0,)):
                        # every case is a batch of mixed counters; the rotation walks all six through every position
                        rot = ncases % len(COUNTERS)
                        counters = COUNTERS[rot:] + COUNTERS[:rot]
                        if (B, n, D) == SHAPES[0] and style == "random" and with_phase and not hypersphere:
                            lists = [COUNTERS[:3], COUNTERS[3:]]      # all six counters on the flagship case
                        else:
                            lists = [counters]
                        for cl in lists:
                            ncases += 1
                            c = make_case(B, n, D, style, with_phase, cl, 1000 + ncases)
                            kw = dict(lr0=5e-2, geo_coef=geo_coef, hypersphere=hypersphere)
                            want, f32r, got = run_ref(c, torch.float64, **kw), run_ref(c, torch.float32, **kw), run_kernel(c, **kw)
                            name = f"{(B, n, D)} {style} phase={int(with_phase)} hs={int(hypersphere)} geo={geo_coef} k={list(cl)[:B]}"
                            assert torch.equal(got["step"], want["step"]), name
                            for key in OUT_KEYS:
                                if want[key] is None:
                                    continue
                                w = want[key]
                                dev = float((f32r[key].double() - w).abs().max())
                                err = float((got[key].double() - w).abs().max())
                                tol = 1e-5 * float(w.abs().max()) + 2 * dev
                                ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
                                if ratio > worst[0]:
                                    worst = (ratio, f"{name} {key}: err {err:.3e} tol {tol:.3e} (fp32 restatement {dev:.3e})")
                                if not err <= tol:
                                    bad.append((name, key, err, tol))
                            for b in range(B):
                                k = int(c["step"][b])
                                if k == 0 and not hypersphere:   # lr_schedule(0) = 0: parameters bit-unchanged, moments moved
                                    assert torch.equal(got["z"][b], c["z"][b]), name
                                    assert not torch.equal(got["m_z"][b], c["m_z"][b]) and not torch.equal(got["v_z"][b], c["v_z"][b])
                                    if with_phase:
                                        assert torch.equal(got["phase"][b], c["phase"][b]) and not torch.equal(got["m_p"][b], c["m_p"][b])
                                    assert float(got["loss_log"][0, b]) != SENTINEL
                                if k == NUM_STEPS:               # finished: nothing of the sample changes
                                    for key in ("z", "g_z", "m_z", "v_z", "geo") + (("phase", "m_p", "v_p") if with_phase else ()):
                                        assert torch.equal(got[key][b], c[key][b]), (name, key)
                                    assert torch.equal(got["loss_log"][:, b], c["loss_log"][:, b]), name
                                if geo_coef == 0.0:
                                    assert torch.equal(got["g_z"][b], c["g_z"][b]), name
    print(f"{ncases} cases; worst error / bound = {worst[0]:.3f}: {worst[1]}")
    assert not bad, bad[:8]


def test_equal_styles_get_the_exact_floor():
    """All N styles equal: |x_i - x_j|^2 is exactly 0 (summed from the differences), so geo = atan2(sqrt(1e-9), B)^3 as
    in the reference -- not rounding noise of a Gram form, a thousand times the 1e-9."""
    c = make_case(1, 10, 512, "identical", False, (5,), 3)
    got = run_kernel(c, geo_coef=5e-3)
    Bq = (4 * c["z"][0, 0].double().pow(2).sum() + 1e-9).sqrt()
    want = float(torch.atan2(torch.tensor(1e-9, dtype=torch.float64).sqrt(), Bq) ** 3)
    assert abs(float(got["geo"][0]) - want) <= 1e-5 * want, (float(got["geo"][0]), want)


def test_the_largest_sample_the_lds_holds():
    """N * D = 16384 (the dynamic LDS request goes through the attribute path above 48 KiB), against the restatement."""
    for (B, n, D), kw in (((2, 32, 512), dict(geo_coef=5e-3)), ((1, 1, 16384), dict(hypersphere=True))):
        c = make_case(B, n, D, "random", True, (20, 1), 77)
        want, f32r, got = run_ref(c, torch.float64, lr0=5e-2, **kw), run_ref(c, torch.float32, lr0=5e-2, **kw), run_kernel(c, **kw)
        for key in OUT_KEYS:
            dev = float((f32r[key].double() - want[key]).abs().max())
            err = float((got[key].double() - want[key]).abs().max())
            assert err <= 1e-5 * float(want[key].abs().max()) + 2 * dev, (key, err, dev)


# ---------------------------------------------------------------------------------------
# 2. repeatability, independence of the batch
# ---------------------------------------------------------------------------------------
def test_bits_repeat_and_do_not_depend_on_the_batch():
    for hypersphere in (False, True):
        c = make_case(3, 10, 512, "random", True, (20, 35, 1), 5)
        kw = dict(geo_coef=5e-3, hypersphere=hypersphere)
        a, b = run_kernel(c, **kw), run_kernel(c, **kw)
        for key in OUT_KEYS + ("step",):
            assert torch.equal(a[key], b[key]), key
        one = {k: (v[:, 1:2] if k == "loss_log" else v[1:2]).contiguous() for k, v in c.items()}
        s = run_kernel(one, **kw)
        for key in OUT_KEYS + ("step",):
            assert torch.equal(s[key], a[key][:, 1:2] if key == "loss_log" else a[key][1:2]), key


# ---------------------------------------------------------------------------------------
# 3. rejections
# ---------------------------------------------------------------------------------------
def test_rejections_launch_nothing():
    import dgv2_native as N
    c = make_case(2, 4, 64, "random", True, (3, 4), 9)
    d = {k: v.to(DEV).clone() for k, v in c.items()}
    order = ("z", "g_z", "m_z", "v_z", "phase", "g_phase", "m_p", "v_p", "step", "loss_terms", "loss_log", "geo")

    def call(ptrs=None, B=2, n=4, D=64, num_steps=NUM_STEPS, geo_coef=5e-3):
        p = {k: d[k].data_ptr() for k in order}
        p.update(ptrs or {})
        return N.lib.dgv2_latent_step(*[p[k] for k in order], B, n, D, num_steps, 5e-2, 0.05, 0.25, 0.9, 0.999, 1e-8,
                                      geo_coef, 0, N.stream())
    rcs = {}
    for k in ("z", "g_z", "m_z", "v_z", "step", "loss_terms", "loss_log", "geo"):
        rcs[f"null {k}"] = call({k: None})
    rcs["B=0"], rcs["N=0"], rcs["D=0"], rcs["num_steps=0"] = call(B=0), call(n=0), call(D=0), call(num_steps=0)
    rcs["N*D>16384"] = call(n=4, D=4097)
    rcs["geo with N=1"] = call(n=1)
    for k in ("phase", "g_phase", "m_p", "v_p"):
        rcs[f"only {k} null"] = call({k: None})
        rcs[f"only {k} set"] = call({j: None for j in ("phase", "g_phase", "m_p", "v_p") if j != k})
    torch.cuda.synchronize()
    assert all(rc == N.EINVAL for rc in rcs.values()), {k: rc for k, rc in rcs.items() if rc != N.EINVAL}
    for k in order:
        assert torch.equal(d[k].cpu(), c[k]), k
    assert call({k: None for k in ("phase", "g_phase", "m_p", "v_p")}) == 0      # all four null is a valid call
    torch.cuda.synchronize()
    assert d["step"].tolist() == [4, 5]


# ---------------------------------------------------------------------------------------
# fixtures of the fitter tests
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "inversion.npz"))
    return {k: d[k] for k in d.files if k.startswith("invert.") or k == "angle_file"}


@pytest.fixture(scope="module")
def coord(gold):
    from gans.coords import CoordBridge
    return CoordBridge(16, 64, 1.45, 80.0, angle_array=gold["angle_file"]).to(DEV)


@pytest.fixture(scope="module")
def G():
    from gans.models.builder import build_generator
    from gans.pretrained import autoload_ckpt
    ck = autoload_ckpt(os.path.join(GOLDEN, "checkpoint_small.pth"))
    cfg = ck["cfg"].model.generator
    cfg.synthesis_kwargs.num_fp16_layers = 0
    G = build_generator(cfg)
    G.load_state_dict(ck["G_ema"])
    return G.eval().to(DEV)


def make_fitter(G, coord, gold, num_steps, graph, batch_size=2):
    from gans.sim2real import LatentFitter, latent_prior
    num_z, _, _, lr1, _, seed = gold["invert.cfg"]
    prior = latent_prior(G, int(num_z), torch.Generator().manual_seed(int(seed)))
    return LatentFitter(G, coord, batch_size, latent_type="w+", num_steps=num_steps, lr=float(lr1), optimize_phase=True,
                        prior=prior, graph=graph)


def targets(gold):
    return torch.from_numpy(gold["invert.depth"]), torch.from_numpy(gold["invert.mask"])


# ---------------------------------------------------------------------------------------
# 4. launch accounting
# ---------------------------------------------------------------------------------------
def _count(fn):
    """(C-ABI entry names, device launches) of fn()."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from test_gpu_inversion import CallLog
    torch.cuda.synchronize()
    with CallLog() as log, profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return list(log.names), sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)


def test_one_latent_step_launch_per_step_and_fewer_launches_than_invert(G, coord, gold):
    from gans.inversion import invert
    depth, mask = targets(gold)
    num_z, _, _, lr1, _, seed = gold["invert.cfg"]

    def run_invert(steps):
        invert(G, coord, depth, mask, latent_type="w+", num_steps_1st=steps, num_steps_2nd=0, lr_1st=float(lr1),
               optimize_phase=True, generator=torch.Generator().manual_seed(int(seed)), num_z_samples=64)
    fitters = {s: make_fitter(G, coord, gold, s, False) for s in (3, 5)}
    for s in (3, 5):   # warm both paths (allocator, lazy module state)
        run_invert(s)
        fitters[s].fit(depth, mask)
    per_step = {}
    for name, run in (("invert", run_invert), ("fitter", lambda s: fitters[s].fit(depth, mask))):
        (c3, k3), (c5, k5) = _count(lambda: run(3)), _count(lambda: run(5))
        per_step[name] = ((len(c5) - len(c3)) / 2, (k5 - k3) / 2)
        if name == "fitter":
            assert c3.count("dgv2_latent_step") == 3 and c5.count("dgv2_latent_step") == 5
        else:
            assert "dgv2_latent_step" not in c5      # invert's launch sequence is the parent's
    print(f"per stage-1 step: invert {per_step['invert'][0]} C-ABI calls, {per_step['invert'][1]} device launches "
          f"(C-ABI kernels + every torch launch, the optimizer's included); fitter {per_step['fitter'][0]} C-ABI "
          f"calls, {per_step['fitter'][1]} device launches")
    assert per_step["fitter"][1] < per_step["invert"][1]
    # C-ABI calls plus the torch launches beside them: the fitter adds one entry and drops the optimizer's launches
    assert per_step["fitter"][0] <= per_step["invert"][0] + 1


# ---------------------------------------------------------------------------------------
# 5. the reference trajectory
# ---------------------------------------------------------------------------------------
def test_fitter_follows_the_reference_trajectory(G, coord, gold):
    s1 = int(gold["invert.cfg"][1])
    depth, mask = targets(gold)
    before = {k: v.clone() for k, v in G.state_dict().items()}
    flags = [p.requires_grad for p in G.parameters()]
    out = make_fitter(G, coord, gold, s1, False).fit(depth, mask)
    assert all(torch.equal(v, before[k]) for k, v in G.state_dict().items())     # G is frozen
    assert [p.requires_grad for p in G.parameters()] == flags
    loss, want, dev = out["loss"].double().cpu(), torch.from_numpy(gold["invert.loss"])[:s1], gold["invert.loss_dev"]
    assert tuple(loss.shape) == (s1, 2) and bool(torch.isfinite(loss).all())
    err = ((loss - want).abs() / want.abs()).max(dim=1).values
    print("per-step loss error  ", " ".join(f"{float(e):.1e}" for e in err))
    print("reference fp32-vs-fp64", " ".join(f"{float(e):.1e}" for e in dev[:s1]))
    gap = float(((loss[-1] - want[-1]).abs() / want[-1]).max())
    rel_latent = float((out["latent"].double().cpu() - torch.from_numpy(gold["invert.latent"]).double()).abs().max()
                       / np.abs(gold["invert.latent"]).max())
    print(f"loss at step {s1 - 1}: {loss[-1].tolist()} reference {want[-1].tolist()} gap {gap:.2%}; latent relative "
          f"distance to the reference's (which went on through pivotal tuning's steps unchanged) {rel_latent:.2e}")
    for i in range(5):
        assert float(err[i]) <= 1e-5 + 2 * float(dev[i]), (i, float(err[i]), float(dev[i]))
    assert gap <= 0.10, gap
    assert bool((loss[-1] < loss[0]).all())
    assert tuple(out["latent"].shape) == tuple(gold["invert.latent"].shape)
    assert tuple(out["phase"].shape) == (2, 2, 1, 1) and float(out["phase"].abs().max()) > 0
    p = out["raydrop_prob"]
    assert tuple(p.shape) == (2, 1, 16, 64) and not p.requires_grad and float(p.min()) >= 0 and float(p.max()) <= 1
    assert tuple(out["inv_depth_orig"].shape) == (2, 1, 16, 64) and not out["inv_depth_orig"].requires_grad


def test_fitter_refuses_a_generator_without_raydrop(G, coord, gold):
    class NoDrop(torch.nn.Module):
        def __init__(self, G):
            super().__init__()
            self.G, self.mapping_network, self.synthesis_network = G, G.mapping_network, G.synthesis_network

        def forward(self, w, angle=None, input_w=False):
            out = self.G(w, angle=angle, input_w=input_w)
            return {k: v for k, v in out.items() if k != "raydrop_logit"}
    from gans.sim2real import LatentFitter, latent_prior
    fitter = LatentFitter(NoDrop(G), coord, 2, num_steps=2, prior=latent_prior(G, 16), graph=False)
    with pytest.raises(ValueError):
        fitter.fit(*targets(gold))


# ---------------------------------------------------------------------------------------
# 6. graph replay
# ---------------------------------------------------------------------------------------
KEYS = ("latent", "phase", "loss", "raydrop_prob", "inv_depth_orig")


def _agree(got, want, scale, what):
    """bit-equal when the eager runs were (scale = 0); else within twice the eager run-to-run difference, taken
    relative to each result's magnitude."""
    for k in KEYS:
        if scale == 0.0:
            assert torch.equal(got[k], want[k]), (what, k, float((got[k] - want[k]).abs().max()))
        else:
            tol = 2 * scale * float(want[k].abs().max())
            assert float((got[k] - want[k]).abs().max()) <= tol, (what, k, float((got[k] - want[k]).abs().max()), tol)


def _eager_runs(G, coord, gold, depth, mask, what):
    """Three fresh eager fits of one batch -> (the first, their run-to-run difference: the largest over the three pairs
    and the result keys, relative to each result's magnitude; 0.0 = bit-equal).  The difference is a property of the
    batch (the optimisation amplifies the last bits of the generator's backward), so every batch gets its own."""
    runs = [make_fitter(G, coord, gold, 8, False).fit(depth, mask) for _ in range(3)]
    scale = max(float((a[k] - b[k]).abs().max()) / float(a[k].abs().max())
                for a, b in ((runs[0], runs[1]), (runs[0], runs[2]), (runs[1], runs[2])) for k in KEYS)
    print(f"eager run-to-run relative difference over 8 steps, {what}: {scale:.2e} "
          f"({'bit-equal' if scale == 0 else 'not bit-equal'})")
    return runs[0], scale


def test_graph_replay_matches_eager_and_sees_every_new_batch(G, coord, gold):
    depth, mask = targets(gold)
    depth_b = depth.flip(0).roll(5, dims=-1).contiguous()      # batch B: other scans
    mask_b = mask.flip(0).roll(5, dims=-1).contiguous()
    e1, scale = _eager_runs(G, coord, gold, depth, mask, "batch A")
    fitter = make_fitter(G, coord, gold, 8, True)
    ga = fitter.fit(depth, mask)
    assert fitter.captured, "the capture fell back to eager steps"
    assert fitter.steps_run == 8
    _agree(ga, e1, scale, "graph vs eager, batch A")
    gb = fitter.fit(depth_b, mask_b)                            # replay only, on batch B
    assert fitter.captured and fitter.steps_run == 16
    fresh, scale_b = _eager_runs(G, coord, gold, depth_b, mask_b, "batch B")
    assert not torch.equal(fresh["loss"], e1["loss"])           # B is another problem than A
    _agree(gb, fresh, scale_b, "batch B after batch A through the same captured fitter (stale prepared target?)")
    # an eager fitter is reusable in the same way
    eager = make_fitter(G, coord, gold, 8, False)
    eager.fit(depth, mask)
    _agree(eager.fit(depth_b, mask_b), fresh, scale_b, "batch B after batch A through one eager fitter")
    # a short batch: padded by repeating its last scan, the padding dropped
    short = fitter.fit(depth_b[:1], mask_b[:1])
    assert all(len(short[k]) == 1 for k in KEYS if k != "loss") and tuple(short["loss"].shape) == (8, 1)
    twice, scale_s = _eager_runs(G, coord, gold, depth_b[[0, 0]], mask_b[[0, 0]], "the padded short batch")
    _agree(short, {k: (twice[k][:, :1] if k == "loss" else twice[k][:1]) for k in KEYS}, scale_s, "short batch")


# ---------------------------------------------------------------------------------------
# 7. end to end
# ---------------------------------------------------------------------------------------
def _make_tree(root, n=5, H=16, W=64, max_depth=80.0):
    from gans.coords import frontal_angle_grid
    from semseg.datasets.sqsg import _hash_unit
    grid = frontal_angle_grid(H, W).astype(np.float64)
    e, a = grid[..., 0], grid[..., 1]
    dirs = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=-1)
    paths = []
    for i in range(n):
        depth = 2.0 + 58.0 * _hash_unit(0, i, 0, H * W).reshape(H, W) ** 2
        u = _hash_unit(0, i, 1, H * W).reshape(H, W)
        depth[u < 0.10] = 0.0                   # no return
        depth[u > 0.95] = max_depth + 15.0      # beyond the sensor's range
        label = (_hash_unit(0, i, 2, H * W).reshape(H, W) * 3).astype(np.int64)
        scan = np.concatenate([dirs * depth[..., None], depth[..., None], label[..., None]], axis=-1).astype(np.float32)
        d = root / "GTAV" / f"seq{i % 2}"
        d.mkdir(parents=True, exist_ok=True)
        np.save(d / f"{i:06d}.npy", scan)
        paths.append(d / f"{i:06d}.npy")
    return sorted(paths)


def test_render_gan_noise_end_to_end(tmp_path, capsys):
    import render_gan_noise
    from semseg.datasets import GTALiDAR_GAN
    scans = _make_tree(tmp_path)
    argv = ["--ckpt_path", os.path.join(GOLDEN, "checkpoint_small.pth"), "--data_root", str(tmp_path),
            "--batch_size", "2", "--num_steps", "8"]

    def run():
        render_gan_noise.main(argv)
        lines = capsys.readouterr().out.strip().splitlines()
        return (json.loads(lines[-1], parse_constant=lambda s: pytest.fail(f"not strict JSON: {s}")),
                [ln for ln in lines[:-1] if ln.startswith("[")])
    stats, progress = run()
    assert stats["rendered"] == 5 and stats["skipped"] == 0 and len(progress) == 3
    assert stats["mean_final_loss"] > 0 and stats["seconds"] > 0 and stats["scans_per_second"] > 0
    outs = [str(s).replace("GTAV", "GTAV_noise_v2") for s in scans]
    for o in outs:
        m = np.load(o)
        assert m.dtype == np.float32 and m.shape == (16, 64) and m.min() >= 0 and m.max() <= 1
    assert len(open(tmp_path / "GTAV_noise_v2" / "manifest.jsonl").readlines()) == 5
    ds = GTALiDAR_GAN(str(tmp_path), shape=(16, 64), gan_dir="GTAV_noise_v2")
    assert len(ds) == 5
    for i in range(len(ds)):
        item = ds[i]
        hit = torch.from_numpy(np.load(scans[i])[..., 3] > 0).float()
        assert tuple(item["mask"].shape) == (16, 64) and bool((item["mask"] <= hit).all())
    mtimes = {o: os.stat(o).st_mtime_ns for o in outs}
    stats2, _ = run()
    assert stats2["rendered"] == 0 and stats2["skipped"] == 5
    assert {o: os.stat(o).st_mtime_ns for o in outs} == mtimes
    os.remove(outs[2])
    stats3, _ = run()
    assert stats3["rendered"] == 1 and stats3["skipped"] == 4 and os.path.exists(outs[2])
    assert all(os.stat(o).st_mtime_ns == mtimes[o] for o in outs if o != outs[2])
    assert not [p for p in (tmp_path / "GTAV_noise_v2").rglob("*") if ".tmp" in p.name]
