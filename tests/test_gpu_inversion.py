"""GAN inversion on the GPU (csrc/inversion.hip, gans/inversion.py) against tests/golden/inversion.npz, which the
reference wrote on CPU in float64 and float32 (tests/golden/make_inversion_golden.py).

Tolerance rule (the one of tests/test_gpu_full.py): a result may differ from the reference's float64 evaluation by
1e-5 relative plus twice the reference's OWN float32-vs-float64 deviation for that case, which the fixture stores.

Measured on an MI355X (worst case; every bound is 1e-5 + 2 x 1e-7 .. 7e-7): loss 1.9e-7, loss gradient 6.8e-7,
conversion values 2.5e-7 and gradients 1.7e-7; inversion trajectory: first five steps 4.6e-8 .. 1.4e-7 (the reference's
own float32-vs-float64 figures, step for step), final loss 1.1 % from the reference's (whose own two precisions end
0.35 % apart).  The file runs in about 5 s."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_FN = {"l1": F.l1_loss, "mse": F.mse_loss}


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "inversion.npz"))
    return {k: d[k] for k in d.files}


def rel(got, want):
    got, want = got.detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-300))


def t(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


def parse_case(name):
    s, fn, rl, lv = name.split(".")
    level = int(lv[len("level"):])
    return s, fn, bool(int(rl[len("rel"):])), (None if level == 0 else level)


def criterion_for(name):
    from gans.inversion import MultiScaleMaskedLoss
    s, fn, relative, level = parse_case(name)
    return s, MultiScaleMaskedLoss(LOSS_FN[fn], level=level, relative=relative).to(DEV)


class CallLog:
    """Names of the C-ABI entries called while active (the machinery of scripts/count_calls.py)."""

    def __enter__(self):
        import dgv2_native as N
        self.N, self.names, self.orig = N, [], (N.call, N.try_call)

        def call(name, *a):
            self.names.append(name)
            return self.orig[0](name, *a)

        def try_call(name, *a):
            self.names.append(name)
            return self.orig[1](name, *a)
        N.call, N.try_call = call, try_call
        return self

    def __exit__(self, *exc):
        self.N.call, self.N.try_call = self.orig


# ---------------------------------------------------------------------------------------
# 1. value and gradient, every stored case
# ---------------------------------------------------------------------------------------
def test_multiscale_masked_loss_matches_reference(gold):
    worst = [0.0, 0.0]
    bad = []
    for name in gold["msml.cases"]:
        s, crit = criterion_for(name)
        gen = t(gold[f"msml.{s}.gen"]).requires_grad_(True)
        ref, mask = t(gold[f"msml.{s}.ref"]), t(gold[f"msml.{s}.mask"])
        loss = crit(gen, ref, mask)
        (g,) = torch.autograd.grad(loss.sum(), gen)
        dl, dg = gold[f"msml.{name}.dev"]
        el, eg = rel(loss, gold[f"msml.{name}.loss"]), rel(g, gold[f"msml.{name}.grad"])
        print(f"{name}: loss err {el:.2e} (bound {1e-5 + 2 * dl:.2e}), grad err {eg:.2e} (bound {1e-5 + 2 * dg:.2e})")
        worst = [max(worst[0], el), max(worst[1], eg)]
        if el > 1e-5 + 2 * dl or eg > 1e-5 + 2 * dg:
            bad.append((name, el, eg))
    print("worst", worst)
    assert not bad, bad


def test_planted_tie_has_zero_l1_gradient(gold):
    """sign(0) = 0: the pixel where gen == ref gets no gradient from its own level (level=1: no other term reaches it)."""
    s, crit = criterion_for("a.l1.rel0.level1")
    gen = t(gold["msml.a.gen"]).requires_grad_(True)
    (g,) = torch.autograd.grad(crit(gen, t(gold["msml.a.ref"]), t(gold["msml.a.mask"])).sum(), gen)
    assert float(g[0, 0, 3, 5]) == 0.0
    assert float(g[0, 0, 3, 6]) != 0.0 or float(gold["msml.a.mask"][0, 0, 3, 6]) == 0.0


# ---------------------------------------------------------------------------------------
# 2. the prepared target is cached on (tensor objects, versions)
# ---------------------------------------------------------------------------------------
def test_target_is_prepared_once_per_target(gold):
    s, crit = criterion_for("a.l1.rel1.level2")
    gen, ref, mask = t(gold["msml.a.gen"]), t(gold["msml.a.ref"]), t(gold["msml.a.mask"])
    with CallLog() as log:
        l0 = crit(gen, ref, mask)
    assert log.names.count("dgv2_msml_prepare") == 1
    with CallLog() as log:
        l1 = crit(gen, ref, mask)
    assert "dgv2_msml_prepare" not in log.names and log.names == ["dgv2_msml_fwd"]
    assert torch.equal(l0, l1)
    mask[0, 0, 3, 7:9] = 0.0      # in place: same object, new version
    with CallLog() as log:
        l2 = crit(gen, ref, mask)
    assert log.names.count("dgv2_msml_prepare") == 1
    assert not torch.equal(l0, l2)
    with CallLog() as log:        # an equal tensor that is another object prepares again
        crit(gen, ref.clone(), mask)
    assert log.names.count("dgv2_msml_prepare") == 1


# ---------------------------------------------------------------------------------------
# 3. launch budget: at most L launches each way per call once the target is prepared, none of them ATen
# ---------------------------------------------------------------------------------------
def _kernels(prof):
    from torch.autograd import DeviceType
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]


@pytest.mark.parametrize("name", ["a.l1.rel1.level1", "a.l1.rel1.level2", "a.mse.rel0.level0"])
def test_launch_budget(gold, name):
    from torch.profiler import ProfilerActivity, profile
    s, crit = criterion_for(name)
    gen = t(gold[f"msml.{s}.gen"]).requires_grad_(True)
    ref, mask = t(gold[f"msml.{s}.ref"]), t(gold[f"msml.{s}.mask"])
    L = crit.num_levels(gen.shape[2])
    ones = torch.ones(gen.shape[0], device=DEV)
    for _ in range(2):            # prepares the target; warms the allocator
        torch.autograd.grad(crit(gen, ref, mask), gen, grad_outputs=ones)
    torch.cuda.synchronize()
    with CallLog() as log, profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as pf:
        loss = crit(gen, ref, mask)
        torch.cuda.synchronize()
    fwd_calls, fwd_kernels = list(log.names), _kernels(pf)
    with CallLog() as log, profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as pb:
        torch.autograd.grad(loss, gen, grad_outputs=ones)
        torch.cuda.synchronize()
    bwd_calls, bwd_kernels = list(log.names), _kernels(pb)
    print(f"{name}: L = {L}; forward {fwd_kernels}; backward {bwd_kernels}")
    assert fwd_calls == ["dgv2_msml_fwd"] and bwd_calls == ["dgv2_msml_bwd"]
    assert 1 <= len(fwd_kernels) <= L and 1 <= len(bwd_kernels) <= L
    for k in fwd_kernels + bwd_kernels:
        assert "msml" in k and "at::" not in k, k
    if L <= 2:   # the demo's setting: one launch each way
        assert len(fwd_kernels) == 1 and len(bwd_kernels) == 1


# ---------------------------------------------------------------------------------------
# 4. the range conversion is differentiable
# ---------------------------------------------------------------------------------------
@pytest.fixture()
def coord(gold):
    from gans.coords import CoordBridge
    return CoordBridge(16, 64, 1.45, 80.0, angle_array=gold["angle_file"]).to(DEV)


def test_convert_records_a_gradient(coord, gold):
    """The regression behind the item: demo_inversion.py:169's depth term must not silently drop out of the objective."""
    x = t(gold["coords.src.inv_depth_norm"]).requires_grad_()
    y = coord.convert(x, "inv_depth_norm", "depth_norm")
    assert y.requires_grad
    assert not coord.convert(x.detach(), "inv_depth_norm", "depth_norm").requires_grad


def test_convert_gradients_match_reference(coord, gold):
    bad = []
    for pair in gold["coords.pairs"]:
        a, b = pair.split(">")
        x = t(gold[f"coords.src.{a}"]).requires_grad_()
        y = coord.convert(x, a, b)
        (g,) = torch.autograd.grad((y * t(gold[f"coords.{pair}.cot"])).sum(), x)
        dv, dg = gold[f"coords.{pair}.dev"]
        ev, eg = rel(y, gold[f"coords.{pair}.value"]), rel(g, gold[f"coords.{pair}.grad"])
        print(f"{pair}: value err {ev:.2e} (bound {1e-5 + 2 * dv:.2e}), grad err {eg:.2e} (bound {1e-5 + 2 * dg:.2e})")
        if ev > 1e-5 + 2 * dv or eg > 1e-5 + 2 * dg:
            bad.append((pair, ev, eg))
    assert not bad, bad


def test_fetch_reals_form_gradient(coord):
    """Mode 0 with the mask blend (*2-1, ray-drop constant): gradient 2 * mask * d(inv_depth_norm) against tensor ops."""
    from gans.models.ops import native
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(2, 1, 16, 64, generator=g) * 70 + 2).to(DEV).requires_grad_()
    m = (torch.rand(2, 1, 16, 64, generator=g) < 0.8).float().to(DEV)
    y = native.coords_convert_diff(x, 0, 1.45, 80.0, coord.angle.contiguous(), m, -1.0)
    r = torch.randn(2, 1, 16, 64, generator=g).to(DEV)
    (got,) = torch.autograd.grad((y * r).sum(), x)
    xd = x.detach().double()
    want = r.double() * 2 * m.double() * (-1.45 / (xd + 1e-11) ** 2)
    # fp32 evaluation of -min_d / (x + tol)^2: a reciprocal, a square and two products, 1 ulp each at most
    assert rel(got, want) < 8 * 2.0 ** -24


# ---------------------------------------------------------------------------------------
# 5. angle gradient of the positional encoding
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("c0", [0, 64])
def test_fourier_feature_angle_gradient(dtype, B, c0):
    """Against float64 tensor ops.  Bound, per pixel and angle: the kernel recomputes c_f = f_e e + f_a a + p_f in fp32
    (three roundings of numbers up to max|c|, then sincos: <= 4 * 2^-24 * max|c| + 4 * 2^-24 in each sin / cos) and
    accumulates F products in fp32 (<= (F + 4) * 2^-24 relative to the sum of magnitudes), so
    |error| <= sum_f |freq| (|g_sin| + |g_cos|) * (4 * 2^-24 * (max|c| + 1) + (F + 4) * 2^-24).
    The bf16 rows are rounded BEFORE both evaluations: the kernel reads them exactly."""
    from gans.models.ops import native
    nf, H, W = 40, 8, 32
    g = torch.Generator().manual_seed(100 + B + c0)
    freqs2 = torch.cat([torch.empty(nf, 1).uniform_(-16, 16, generator=g),
                        torch.randint(-32, 33, (nf, 1), generator=g).float()], dim=1)
    phase = torch.rand(nf, generator=g) * 2 * np.pi
    angle = torch.stack([torch.empty(B, H, W).uniform_(-0.45, 0.05, generator=g),
                         torch.empty(B, H, W).uniform_(-np.pi, np.pi, generator=g)], dim=1)
    ld = c0 + 2 * nf
    grad = torch.randn(B, H, W, ld, generator=g).to(dtype)
    got = native.fourier_feature_bwd(grad.to(DEV), c0, angle.to(DEV), None, freqs2.to(DEV).contiguous(), phase.to(DEV))
    a64 = angle.double().requires_grad_(True)
    c = torch.einsum("bahw,fa->bhwf", a64, freqs2.double()) + phase.double()
    pe = torch.cat([c.sin(), c.cos()], dim=3)
    g64 = grad.double()[..., c0:c0 + 2 * nf]
    (want,) = torch.autograd.grad((pe * g64).sum(), a64)
    mag = g64[..., :nf].abs() + g64[..., nf:].abs()                          # [B,H,W,F]
    terms = torch.einsum("bhwf,fa->bahw", mag, freqs2.double().abs())
    u = 2.0 ** -24
    bound = terms * (4 * u * (float(c.detach().abs().max()) + 1) + (nf + 4) * u)
    err = (got.double().cpu() - want).abs()
    print(f"{dtype} B={B} c0={c0}: max err {float(err.max()):.2e}, max |want| {float(want.abs().max()):.2e}, "
          f"worst err/bound {float((err / bound).max()):.3f}")
    assert got.shape == want.shape and got.dtype == torch.float32
    assert bool((err <= bound).all()), float((err / bound).max())


def test_up_cat_pe_returns_both_gradients():
    """The level input of the generator (FIR up-2 of h beside the encoding): h and the angles both get their gradient
    from the native node; the angle gradient equals the stand-alone kernel's on that channel slice."""
    from gans.models.ops import native
    nf, H, W, B = 16, 8, 32, 2
    g = torch.Generator().manual_seed(9)
    freqs2 = torch.randint(-8, 9, (nf, 2), generator=g).float().to(DEV)
    phase = (torch.rand(nf, generator=g) * 6).to(DEV)
    angle = (torch.rand(B, 2, H, W, generator=g) - 0.5).to(DEV).requires_grad_(True)
    x = native.up_cat_pe(None, None, angle, None, freqs2, phase, torch.float32, B)
    assert x.requires_grad and tuple(x.shape) == (B, H, W, 2 * nf)
    r = torch.randn(B, H, W, 2 * nf, generator=g).to(DEV)
    (ga,) = torch.autograd.grad((x * r).sum(), angle)
    assert torch.equal(ga, native.fourier_feature_bwd(r, 0, angle.detach(), None, freqs2, phase))
    y = native.fourier_feature(angle, None, freqs2, phase)
    assert torch.equal(y, x)
    (gb,) = torch.autograd.grad((y * r).sum(), angle)
    assert torch.equal(ga, gb)


# ---------------------------------------------------------------------------------------
# 6. the driver
# ---------------------------------------------------------------------------------------
def test_invert_follows_the_reference_trajectory(coord, gold):
    from gans.inversion import invert
    from gans.models.builder import build_generator
    from gans.pretrained import autoload_ckpt
    ck = autoload_ckpt(os.path.join(GOLDEN, "checkpoint_small.pth"))
    cfg = ck["cfg"].model.generator
    cfg.synthesis_kwargs.num_fp16_layers = 0
    G = build_generator(cfg)
    G.load_state_dict(ck["G_ema"])
    G.eval().to(DEV)
    num_z, s1, s2, lr1, lr2, seed = gold["invert.cfg"]
    out = invert(G, coord, torch.from_numpy(gold["invert.depth"]), torch.from_numpy(gold["invert.mask"]),
                 latent_type="w+", num_steps_1st=int(s1), num_steps_2nd=int(s2), lr_1st=float(lr1), lr_2nd=float(lr2),
                 optimize_phase=True, perturb_z=False, hypersphere_z=False,
                 generator=torch.Generator().manual_seed(int(seed)), num_z_samples=int(num_z))
    loss, want, dev = out["loss"].double().cpu(), torch.from_numpy(gold["invert.loss"]), gold["invert.loss_dev"]
    assert tuple(loss.shape) == (int(s1) + int(s2), 2) and bool(torch.isfinite(loss).all())
    err = ((loss - want).abs() / want.abs()).max(dim=1).values
    print("per-step loss error  ", " ".join(f"{float(e):.1e}" for e in err))
    print("reference fp32-vs-fp64", " ".join(f"{float(e):.1e}" for e in dev))
    gap = float(((loss[-1] - want[-1]).abs() / want[-1]).max())
    print(f"final loss {loss[-1].tolist()} reference {want[-1].tolist()} gap {gap:.2%}; "
          f"latent rel diff {rel(out['latent'], gold['invert.latent']):.2e}")
    for i in range(5):
        assert float(err[i]) <= 1e-5 + 2 * float(dev[i]), (i, float(err[i]), float(dev[i]))
    assert bool((loss[-1] < loss[0]).all())
    assert gap <= 0.10, gap
    assert tuple(out["latent"].shape) == tuple(gold["invert.latent"].shape)
    assert tuple(out["phase"].shape) == (2, 2, 1, 1) and float(out["phase"].abs().max()) > 0
    for k in ("inv_depth", "inv_depth_orig", "raydrop_prob"):
        assert tuple(out[k].shape) == (2, 1, 16, 64) and not out[k].requires_grad


# ---------------------------------------------------------------------------------------
# 7. run to run
# ---------------------------------------------------------------------------------------
def test_loss_is_bit_identical_run_to_run(gold):
    for name in ("a.l1.rel1.level2", "a.mse.rel1.level0", "b.l1.rel1.level0"):
        res = []
        for _ in range(2):
            s, crit = criterion_for(name)
            gen = t(gold[f"msml.{s}.gen"]).requires_grad_(True)
            loss = crit(gen, t(gold[f"msml.{s}.ref"]), t(gold[f"msml.{s}.mask"]))
            (g,) = torch.autograd.grad(loss.sum(), gen)
            res.append((loss.detach().clone(), g.clone()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), name
