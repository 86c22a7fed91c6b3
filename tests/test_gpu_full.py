"""Full-size parity on the GPU (64x512, channel widths 512..32): the HIP modules in fp32 parity mode against the
fixture the REFERENCE produced at that size (tests/golden/model_full.npz: G step, D step, lazy R1, eval forwards of
BASELINE configs[0] / [1]).  These shapes take kernels the reduced configuration never reaches (dgv2_modconv_pe_fwd_sq and
its slabs, streaming weight gradients, weight bank, fused stem, one-launch data gradients).  Tolerance: 1e-3 relative
(north_star).  Then the bf16 throughput mode against the same fixture with a stated bf16 tolerance."""
import pytest
import torch

from conftest import sub_dict
from helpers import ada_from_cfg, build_models, full_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = torch.nn.functional


def rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-30))


def full_models(d, low_precision=False, gbuf=False):
    import recipe
    cfg = full_cfg(low_precision)
    G, D = build_models(cfg, "cpu")
    sdG = recipe.fill_state_dict({k: v.clone() for k, v in G.state_dict().items()}, 1234)
    sdD = recipe.fill_state_dict({k: v.clone() for k, v in D.state_dict().items()}, 4321)
    sdG.update(sub_dict(d, "G."))            # PE frequencies / phases of the reference ctor
    if gbuf:
        sdG.update(sub_dict(d, "G1buf."))    # ema_var / w_avg the fixture's G step left
    G.load_state_dict(sdG)
    D.load_state_dict(sdD)
    return cfg, G.to(DEV), D.to(DEV), ada_from_cfg(cfg, 0.6, DEV)


def tensor_err(got, want):
    """max |got - want| relative to max |want| (per-tensor relative error)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-300))


def check_vs_f64(named_grads, truth, tol, floor=0.0):
    """Every gradient tensor, WHOLE, against the fp64 evaluation: max abs error <= tol * max|truth| (+ floor)."""
    assert set(named_grads) == set(truth), set(named_grads) ^ set(truth)
    bad, worst = [], (0.0, "")
    for k, t in truth.items():
        g = named_grads[k].detach().double().cpu().reshape(t.shape)
        e = float((g - t).abs().max() / (t.abs().max() + floor / tol + 1e-300))
        worst = max(worst, (e, k))
        if e > tol:
            bad.append((k, e))
    assert not bad, (tol, bad)
    return worst


def check_vs_fixture(named_grads, d, prefix, truth, tol, n=32, floor=0.0):
    """Against the reference's fp32 numbers (norm and leading slice of every gradient): within tol plus the reference's
    OWN deviation from the fp64 evaluation for that tensor (triangle inequality; ~1e-6 for most tensors, up to 5e-3
    for sums that cancel over 65 k pixels)."""
    bad = []
    for k, g in named_grads.items():
        if f"{prefix}gradnorm.{k}" not in d:
            continue
        t = truth[k]
        want_norm, sl = float(d[f"{prefix}gradnorm.{k}"]), d[f"{prefix}gradslice.{k}"].double()
        scale = float(t.abs().max()) + floor / tol
        ref_dev_norm = abs(float(t.norm()) - want_norm) / (want_norm + floor / tol)
        ref_dev_sl = float((t.flatten()[:n] - sl).abs().max()) / scale
        e_norm = abs(float(g.double().norm()) - want_norm) / (want_norm + floor / tol)
        e_sl = float((g.flatten()[:n].double().cpu() - sl).abs().max()) / scale
        if e_norm > tol + 1.5 * ref_dev_norm:
            bad.append((k, "norm", e_norm, ref_dev_norm))
        if e_sl > tol + 1.5 * ref_dev_sl:
            bad.append((k, "slice", e_sl, ref_dev_sl))
    assert not bad, (prefix, tol, bad)


@pytest.fixture(scope="module")
def angle(g_coords):
    return g_coords["angle_64x512"].to(DEV)


@pytest.fixture(scope="module")
def truth(g_full, g_coords):
    from helpers import oracle_f64_full
    return oracle_f64_full(g_full, g_coords["angle_64x512"])


def test_fp32_g_step_matches_reference(g_full, angle, truth):
    d = g_full
    cfg, G, D, A = full_models(d)
    G.train().requires_grad_(True)
    D.requires_grad_(False)
    noise = {"shifts": d["gs_shifts"].to(DEV), "gumbel_u": d["gs_u"].to(DEV)}
    o = G(d["z"].to(DEV), angle=angle, noise=noise)
    assert rel(o["image_orig"], d["gs_image_orig"].float()) < 1e-3     # fixture stores fp16 (5e-4)
    assert rel(o["raydrop_logit"], d["gs_raydrop_logit"].float()) < 1e-3
    x_aug = A(o["image"], draws={"G": d["gs_adaG"], "C": d["gs_adaC"]})
    assert rel(x_aug[:, :, 31], d["gs_x_aug_row"]) < 1e-3
    # the ray-drop mask is a hard threshold: a pixel whose perturbed logit is ~0 may flip, everything else agrees
    assert float(((x_aug.double().cpu() - truth["x_aug"]).abs() > 1e-3).double().mean()) < 1e-4
    y_fake = D(x_aug)
    loss = F.softplus(-y_fake).mean()
    assert rel(y_fake, d["gs_y_fake"]) < 1e-3 and rel(y_fake, truth["y_fake"]) < 1e-3
    assert rel(loss, d["gs_loss"]) < 1e-4
    params = dict(G.named_parameters())
    grads = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
    got = {k: g for k, g in zip(params, grads) if g is not None}
    assert set(got) == {k[len("gs_gradnorm."):] for k in d if k.startswith("gs_gradnorm.")}
    check_vs_f64(got, truth["grads_g"], 1e-3)               # whole tensors, north_star tolerance
    check_vs_fixture(got, d, "gs_", truth["grads_g"], 1e-3)   # the reference's own fp32 numbers
    sd = G.state_dict()
    for k, v in sub_dict(d, "G1buf.").items():
        assert rel(sd[k], v) < 1e-5, k


def test_fp32_d_step_and_r1_match_reference(g_full, angle, truth):
    d = g_full
    cfg, G, D, A = full_models(d)
    G.train().requires_grad_(False)
    D.requires_grad_(True)
    B = d["z"].shape[0]
    with torch.no_grad():
        o = G(d["z"].to(DEV), angle=angle, noise={"shifts": d["gs_shifts"].to(DEV), "gumbel_u": d["gs_u"].to(DEV)})
        xf = A(o["image"], draws={"G": d["gs_adaG"], "C": d["gs_adaC"]})
        xr = A(d["x_real"].to(DEV), draws={"G": d["ds_adaG_real"], "C": d["ds_adaC_real"]})
    params = dict(D.named_parameters())
    # the trainer's one-pass form (both halves stacked) == the reference's two calls
    y = D(torch.cat([xr, xf]), splits=2)
    y_real, y_fake = y[:B], y[B:]
    assert rel(y_real, d["ds_y_real"]) < 1e-3 and rel(y_fake, d["gs_y_fake"]) < 1e-3
    loss = F.softplus(-y_real).mean() + F.softplus(y_fake).mean()
    assert rel(loss, d["ds_loss"]) < 1e-4
    grads = dict(zip(params, torch.autograd.grad(loss, list(params.values()))))
    check_vs_f64(grads, truth["grads_d"], 1e-3)
    check_vs_fixture(grads, d, "ds_", truth["grads_d"], 1e-3)

    # lazy R1 (trainer.py:419-451): double backward through D and ADA at full size
    xin = d["x_real"].to(DEV).clone().requires_grad_(True)
    yr = D(A(xin, draws={"G": d["r1_adaG"], "C": d["r1_adaC"]}), double_backward=True)
    (gx,) = torch.autograd.grad(yr.sum(), xin, create_graph=True)
    assert rel(gx[:, :, 31], d["r1_gradx_row"]) < 1e-3
    # whole input gradient vs fp64: a unit next to a leaky-ReLU kink may land on the other side and moves the patch
    # of pixels below it (a dozen of 65 k here); all others agree to 1e-3 of the maximum
    egx = (gx.double().cpu() - truth["grad_x"]).abs() / truth["grad_x"].abs().max()
    assert float((egx > 1e-3).double().mean()) < 1e-3 and float(egx.max()) < 1e-2
    assert abs(float(gx.double().norm()) - float(d["r1_gradx_norm"])) < 1e-3 * float(d["r1_gradx_norm"])
    r1 = (gx ** 2).sum(dim=[1, 2, 3]).mean()
    assert rel(r1, d["r1_penalty"]) < 1e-3
    rgrads = torch.autograd.grad((16.0 / 2) * r1 + 0.0 * yr.squeeze()[0], list(params.values()), allow_unused=True)
    got = {k: g for k, g in zip(params, rgrads) if g is not None and k in truth["grads_r1"]}
    # weights: 2e-3 of each tensor's maximum.  The bias gradients of R1 are pure second-order terms, sums that cancel
    # over every pixel and sit five orders below the weight gradients: the reference's own fp32 run deviates 3-5e-3 from
    # the fp64 value on them, and so may ours (5e-3), with an absolute floor tied to the largest gradient of the step
    top = max(float(v.abs().max()) for v in truth["grads_r1"].values())
    isb = lambda k: truth["grads_r1"][k].ndim == 1
    check_vs_f64({k: g for k, g in got.items() if not isb(k)}, {k: truth["grads_r1"][k] for k in got if not isb(k)}, 2e-3)
    check_vs_f64({k: g for k, g in got.items() if isb(k)}, {k: truth["grads_r1"][k] for k in got if isb(k)}, 5e-3,
                 floor=5e-3 * 1e-4 * top)
    topn = max(float(v) for k, v in d.items() if k.startswith("r1_gradnorm."))
    check_vs_fixture(got, d, "r1_", truth["grads_r1"], 2e-3, floor=2e-3 * 1e-4 * topn)


def test_fp32_discriminator_at_batch_4_matches_reference():
    """The HIP discriminator (fp32 parity mode) on tests/golden/model_full_b4.npz: full width, B = 4, so the minibatch
    standard deviation runs with its configured group of 4 (dgv2_mbstd_cat_fwd_x/_bwd_x): logits, loss and every parameter
    gradient (norm and leading slice) within 1e-3 of the reference's CPU run."""
    from conftest import load_golden
    from helpers import build_models, full_cfg
    import recipe
    d = load_golden("model_full_b4.npz")
    _, D = build_models(full_cfg(), DEV)
    D.load_state_dict(recipe.fill_state_dict({k: v.clone().cpu() for k, v in D.state_dict().items()}, 4321))
    D.requires_grad_(True)
    y = D(d["x"].to(DEV))
    want = d["y"]
    assert float((y.cpu() - want).abs().max()) <= 1e-3 * float(want.abs().max())
    loss = torch.nn.functional.softplus(-y).mean()
    assert abs(float(loss) - float(d["loss"])) <= 1e-4 * abs(float(d["loss"]))
    params = dict(D.named_parameters())
    grads = dict(zip(params, torch.autograd.grad(loss, list(params.values()))))
    for k, g in grads.items():
        wn, sl = float(d[f"gradnorm.{k}"]), d[f"gradslice.{k}"]
        assert abs(float(g.double().norm()) - wn) <= 2e-3 * wn, (k, float(g.double().norm()), wn)
        assert float((g.flatten()[:32].cpu() - sl).abs().max()) <= 2e-3 * float(sl.abs().max()) + 2e-3 * wn / max(1.0, g.numel() ** 0.5), k


@pytest.mark.parametrize("low", [False, True])
def test_eval_forwards_match_reference(g_full, angle, low):
    """BASELINE configs[0] (quick_demo.py: eval, B = 1, truncation_psi = 0.7) and the configs[1] shape (B = 32, which is
    bf16 in the benchmark: low=True, stated tolerance 3e-2 of the output range)."""
    d = g_full
    cfg, G, D, A = full_models(d, low_precision=low, gbuf=True)
    G.eval()
    tol = 3e-2 if low else 1e-3
    z32 = torch.randn(32, 512, generator=torch.Generator().manual_seed(10)).to(DEV)
    with torch.no_grad():
        o = G(z32[:1], angle=angle, truncation_psi=0.7, noise={"gumbel_u": d["ev1_u"].to(DEV)})
        assert rel(o["image_orig"], d["ev1_image_orig"]) < tol
        assert rel(o["raydrop_logit"], d["ev1_raydrop_logit"]) < tol
        if not low:
            assert float(((o["image"].cpu() - d["ev1_image"]).abs() > 1e-3).float().mean()) < 1e-3
        o = G(z32, angle=angle, truncation_psi=0.7)
    for name in ("image_orig", "raydrop_logit"):
        v = o[name].float().cpu()
        assert rel(v[:, 0, 31], d[f"ev32_{name}_row"]) < tol, name
        nrm = v.double().flatten(1).norm(dim=1)
        assert float(((nrm - d[f"ev32_{name}_norm"]).abs() / d[f"ev32_{name}_norm"]).max()) < tol, name


def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300))


def _l2(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def test_bf16_outputs_track_reference(g_full, angle, truth):
    """Throughput mode (bf16 storage, fp32 accumulation; D epilogue in fp32 like the reference) against the reference's
    fp32 fixture: generator outputs and discriminator logits within 2e-2 of their range."""
    d = g_full
    cfg, G, D, A = full_models(d, low_precision=True)
    G.train()
    B = d["z"].shape[0]
    with torch.no_grad():
        o = G(d["z"].to(DEV), angle=angle, noise={"shifts": d["gs_shifts"].to(DEV), "gumbel_u": d["gs_u"].to(DEV)})
        assert rel(o["image_orig"], d["gs_image_orig"].float()) < 2e-2
        assert rel(o["raydrop_logit"], d["gs_raydrop_logit"].float()) < 2e-2
        xr = A(d["x_real"].to(DEV), draws={"G": d["ds_adaG_real"], "C": d["ds_adaC_real"]})
        y = D(torch.cat([xr, truth["x_aug"].float().to(DEV)]), splits=2)   # the fixture's own D inputs
    assert rel(y[B:], d["gs_y_fake"]) < 2e-2
    # D(real) on white-noise reals is a near-cancelling sum (|y| ~ 0.05): judged against the logit range of the step
    assert float((y[:B].double().cpu() - truth["y_real"]).abs().max()) < 2e-2 * float(truth["y_fake"].abs().max())


def test_bf16_gradients_track_fp32_per_tensor():
    """Per-tensor agreement of the bf16 backward kernels with the fp32 parity mode (itself pinned to the reference at
    1e-3 above), same weights and inputs, B = 8.  Losses are LINEAR functionals of the generator outputs / of the
    discriminator trunk's features, so that what is compared is kernel precision and not the discrete events a
    reduced-precision run flips downstream (the hard ray-drop threshold; the 512-unit leaky-ReLU bottleneck of D's fp32
    epilogue, where one flipped unit moves the input gradient by several percent in ANY implementation).  Every tensor:
    cosine >= 0.998 and relative L2 error <= 6e-2.  End to end through the real losses only the direction is asserted:
    cosine of all gradients together >= 0.99 (G) / 0.98 (D)."""
    import recipe
    from oracle import coords as o_coords
    from gans.coords import synthetic_angle_grid
    B, H, W = 8, 64, 512
    g = torch.Generator().manual_seed(3)
    z = torch.randn(B, 512, generator=g).to(DEV)
    noise = {"shifts": (torch.rand(B, generator=g) * 6.28).to(DEV),
             "gumbel_u": torch.rand(B, 1, H, W, generator=g).clamp(1e-6, 1 - 1e-6).to(DEV)}
    r1, r2 = torch.randn(B, 1, H, W, generator=g).to(DEV), torch.randn(B, 1, H, W, generator=g).to(DEV)
    t = torch.linspace(0, 6.28, W)[None, None, None, :] * torch.arange(1, 2 * B + 1)[:, None, None, None]
    xin = (torch.sin(t + torch.linspace(0, 3, H)[None, None, :, None]) * 0.8).to(DEV)
    rf = None
    ang = torch.from_numpy(o_coords.resample_angle_grid(synthetic_angle_grid(64), H, W)).to(DEV)
    d = {}
    res = {}
    G0, D0 = build_models(full_cfg(), "cpu")
    sdG = recipe.fill_state_dict({k: v.clone() for k, v in G0.state_dict().items()}, 1234)
    sdD = recipe.fill_state_dict({k: v.clone() for k, v in D0.state_dict().items()}, 4321)
    for low in (False, True):
        G, D = build_models(full_cfg(low), "cpu")
        G.load_state_dict(sdG)
        D.load_state_dict(sdD)
        G, D = G.to(DEV).train().requires_grad_(True), D.to(DEV).train().requires_grad_(True)
        o = G(z, angle=ang, noise=noise)
        gp, dp = dict(G.named_parameters()), dict(D.named_parameters())
        lin = (o["image_orig"] * r1).mean() + (o["raydrop_logit"] * r2).mean() * 0.1
        gg = {k: v for k, v in zip(gp, torch.autograd.grad(lin, list(gp.values()), allow_unused=True, retain_graph=True))
              if v is not None}
        feats = D(xin, splits=2, features_only=True).float()
        if rf is None:
            rf = torch.randn(feats.shape, generator=g).to(DEV)
        trunk = {k: v for k, v in zip(dp, torch.autograd.grad((feats * rf).mean(), list(dp.values()), allow_unused=True))
                 if v is not None}
        # end to end through the real losses
        y_fake = D(o["image"])
        ge = {k: v for k, v in zip(gp, torch.autograd.grad(F.softplus(-y_fake).mean(), list(gp.values()), allow_unused=True))
              if v is not None}
        y = D(xin, splits=2)
        de = dict(zip(dp, torch.autograd.grad(F.softplus(-y[:B]).mean() + F.softplus(y[B:]).mean(), list(dp.values()))))
        res[low] = (gg, trunk, ge, de)
    report = {}
    for idx, name in ((0, "G"), (1, "D trunk")):
        ref, got = res[False][idx], res[True][idx]
        assert set(ref) == set(got)
        rows = sorted(((_l2(got[k], t), _cos(got[k], t), k) for k, t in ref.items()), reverse=True)
        report[name] = rows[:3]
        bad = [(k, e, c) for e, c, k in rows if e > 6e-2 or c < 0.998]
        assert not bad, (name, bad)
    flat = lambda gs: torch.cat([gs[k].double().flatten().cpu() for k in sorted(gs)])
    assert _cos(flat(res[True][2]), flat(res[False][2])) > 0.99
    assert _cos(flat(res[True][3]), flat(res[False][3])) > 0.98


def test_training_forward_of_the_generator_is_reproducible():
    """The timed configuration's generator forward (bf16 trunks, B = 64, training mode: every ModConv2d updates its
    input-magnitude EMA from statistic partials the producing kernels leave, style.py:98-103) run 150 times from the same
    state on the same inputs: images, ray-drop logits and every ema_var must come out with the same bits -- the forward
    has no float atomics, so any difference is a race.  (It was one: a hand-issued load left in flight past the sample
    loop of modconv_pe overwrote a partial sum about once in 20 forwards)"""
    import recipe
    from oracle import coords as o_coords
    from gans.coords import synthetic_angle_grid
    B, H, W = 64, 64, 512
    g = torch.Generator().manual_seed(7)
    G, _ = build_models(full_cfg(True), "cpu")
    G.load_state_dict(recipe.fill_state_dict({k: v.clone() for k, v in G.state_dict().items()}, 99))
    G = G.to(DEV).train()
    z = torch.randn(B, 512, generator=g).to(DEV)
    noise = {"shifts": (torch.rand(B, generator=g) * 6.28).to(DEV),
             "gumbel_u": torch.rand(B, 1, H, W, generator=g).clamp(1e-6, 1 - 1e-6).to(DEV)}
    ang = torch.from_numpy(o_coords.resample_angle_grid(synthetic_angle_grid(64), H, W)).to(DEV)
    state0 = {k: v.clone() for k, v in G.state_dict().items()}

    def run():
        G.load_state_dict(state0)
        with torch.no_grad():
            o = G(z, angle=ang, noise=noise)
        bufs = {k: v.clone() for k, v in G.state_dict().items() if k.endswith("ema_var") or k.endswith("w_avg")}
        return o["image_orig"].clone(), o["raydrop_logit"].clone(), bufs

    img0, logit0, b0 = run()
    assert len(b0) > 10
    bad = []
    for i in range(150):
        img, logit, b = run()
        diff = [k for k in b0 if not torch.equal(b0[k], b[k])]
        if diff or not torch.equal(img, img0) or not torch.equal(logit, logit0):
            bad.append((i, diff[:4]))
    assert not bad, f"{len(bad)} of 150 forwards differ from the first: {bad[:3]}"


def test_forward_of_the_discriminator_is_reproducible():
    """The same for the discriminator's forward at the D step's size (2B = 128 images, bf16 trunks, fp32 epilogue): 100
    runs, same logits bit for bit (strip-streaming and halo-tile convs, MFMA blurs, decimating FIRs, minibatch-stddev
    statistic, the three-plane Linear)."""
    import recipe
    B, H, W = 64, 64, 512
    _, D = build_models(full_cfg(True), "cpu")
    D.load_state_dict(recipe.fill_state_dict({k: v.clone() for k, v in D.state_dict().items()}, 98))
    D = D.to(DEV).train()
    t = torch.linspace(0, 6.28, W)[None, None, None, :] * torch.arange(1, 2 * B + 1)[:, None, None, None]
    xin = (torch.sin(t + torch.linspace(0, 3, H)[None, None, :, None]) * 0.8).to(DEV)
    with torch.no_grad():
        y0 = D(xin, splits=2).clone()
        assert torch.isfinite(y0).all()
        bad = sum(int(not torch.equal(D(xin, splits=2), y0)) for _ in range(100))
    assert bad == 0, f"{bad} of 100 forwards differ from the first"


@pytest.mark.parametrize("low", [False, True])
def test_r1_pass_with_the_epilogue_conv_on_the_matrix_cores_matches_the_exact_fp32_conv(low):
    """R1 (reference: trainer.py:419-451) through the discriminator, once with its fp32 epilogue conv on the bf16 matrix
    cores (native.x3_auto: plane images built per call -- the pass has no weight bank --, the 15 padding channels told apart
    by the `live` map; bf16 trunk: the zero planes of its features skipped) and once on the exact fp32 MFMA kernels;
    everything else in the two passes is the same launch.  fp32 trunk: the penalty agrees to 1e-5, every weight gradient
    to the fp32 accumulation noise both kernels carry (< 5e-4 of the tensor's norm; see below).  bf16 trunk: the 1e-6 differences of the
    epilogue's results flip bf16 roundings of the trunk's first- and second-order gradients behind it, every tensor --
    the epilogue's own second-order terms included -- then agrees to a few 1e-3.  In-situ check of what
    tests/test_gpu_ops.py::test_conv_x3_is_fp32_equivalent holds per call."""
    import dgv2_native as N
    from gans.models.ops import native as nat
    torch.manual_seed(3)
    _, D = build_models(full_cfg(low), DEV)
    D.requires_grad_(True)
    xr = (torch.rand(8, 1, 64, 512, device=DEV) * 2 - 1)
    conv = D.epilogue[1]
    live = {(conv.in_ch + 15) // 16 * 16: conv.in_ch}

    def run(on):
        for p in D.parameters():
            p.grad = None
        x = xr.clone().requires_grad_(True)
        with nat.x3_auto(on, live):
            y = D(x, double_backward=True)
            (g,) = torch.autograd.grad(y.sum(), [x], create_graph=True)
            r1 = (g.float() ** 2).sum(dim=[1, 2, 3]).mean()
            r1.backward()
        return float(r1.detach()), {k: p.grad.detach().float().clone() for k, p in D.named_parameters() if p.grad is not None}

    r_off, g_off = run(False)
    r_on, g_on = run(True)
    assert N.status_read() == 0
    assert set(g_on) == set(g_off) and len(g_on) >= 20
    assert abs(r_on - r_off) <= 1e-4 * abs(r_off), (r_on, r_off)
    rel = sorted(((float((g_on[k] - g_off[k]).norm() / (g_off[k].norm() + 1e-30)), k) for k in g_off), reverse=True)
    print(f"low={low}: r1 {r_on:.6e} vs {r_off:.6e};", ", ".join(f"{k} {v:.1e}" for v, k in rel))
    if low:
        assert rel[0][0] < 2e-2, rel[:4]
    else:
        # both convs carry fp32 accumulation noise of ~3e-6 of sum |g||w| over 4 608 terms of random sign, i.e. ~2e-4 of the
        # RESULT, in different realisations: every weight gradient behind them differs by about that (measured 1.3-1.9e-4,
        # uniformly over the layers); the bias gradients of R1 are small sums through the minibatch-stddev path only (a
        # piecewise-linear network has no other second-order dependence on its biases) and amplify it ten-fold
        assert all(v < 5e-4 for v, k in rel if k.endswith("weight")), [r for r in rel if r[1].endswith("weight")][:4]
        assert rel[0][0] < 5e-3, rel[:4]


def test_fp32_epilogue_on_bf16_features_keeps_its_x_exact_promise_at_b64():
    """The timed configuration's discriminator epilogue (dusty_v2.py:376-379 in the fp32 island of :394-395) at B = 64 behind
    the bf16 trunk: minibatch-stddev -> 3x3 513 -> 512 conv -> bias + leaky ReLU on conv_x3.hip with the `x_exact = 512`
    promise Discriminator.forward makes for the trunk's features (three of six plane products skipped) against the ORACLE's
    float64 epilogue evaluated on the same bf16 features: fp32-equivalent (the exact-fp32 kernel's own distance from
    float64 is the yardstick), and the kernels' status word stays clear (no value broke the promise)."""
    import math
    import recipe
    import dgv2_native as N
    from gans.models.ops import native
    from oracle import ops as o_ops
    B, H, W = 64, 64, 512
    _, D = build_models(full_cfg(True), "cpu")
    sd = recipe.fill_state_dict({k: v.clone() for k, v in D.state_dict().items()}, 4321)
    D.load_state_dict(sd)
    D = D.to(DEV).train()
    t = torch.linspace(0, 6.28, W)[None, None, None, :] * torch.arange(1, B + 1)[:, None, None, None]
    xin = (torch.sin(t + torch.linspace(0, 3, H)[None, None, :, None]) * 0.8).to(DEV)
    N.status_read()
    with torch.no_grad():
        feats = D(xin, features_only=True)                              # bf16 [B, 4, 32, 512], channels-last
        assert feats.dtype == torch.bfloat16
        mb, conv, act1 = D.epilogue[0], D.epilogue[1], D.epilogue[2]
        cin = feats.shape[3] + mb.features
        cpad = (cin + 15) // 16 * 16
        bank = D._weight_bank()

        def epilogue(promise):
            x = native.mbstd_cat(feats, mb.group, 1, cpad, out_dtype=torch.float32)
            if promise:
                x._dgv2_exact = int(feats.shape[3])
            return conv.forward_cl(x, pad_in_to=cpad, act=act1, bank=bank)
        got = epilogue(True)
        full = epilogue(False)
        assert N.status_read() == 0, "a trunk feature was not bf16-representable: the x_exact promise is broken"
        assert torch.equal(got, full)                                    # the skipped products are products with zero
        # the same epilogue on the exact-fp32 MFMA kernel (no plane images): the yardstick
        from gans.models.ops.native import conv as cv
        old = cv._CONV_X3
        cv._CONV_X3 = False
        try:
            exact32 = epilogue(False)
        finally:
            cv._CONV_X3 = old
    # float64 oracle on the same features
    f64 = feats.float().permute(0, 3, 1, 2).double().cpu()
    h = o_ops.minibatch_stddev(f64, mb.group, mb.features)
    h = o_ops.equal_lr_conv2d(h, sd["epilogue.1.1.module.weight"].double(), 1, 1, True)
    want = o_ops.fused_leaky_relu(h, sd["epilogue.2.bias"].double())
    g = got.permute(0, 3, 1, 2).double().cpu()
    e32 = exact32.permute(0, 3, 1, 2).double().cpu()
    scale = float(want.abs().max())
    err_x3 = float((g - want).abs().max()) / scale
    err_32 = float((e32 - want).abs().max()) / scale
    assert err_x3 <= max(2 * err_32, 2e-6), (err_x3, err_32)
    assert err_x3 < 1e-5, err_x3


# ---------------------------------------------------------------------------- the timed mode against float64, per tensor
def bf16_vs_f64_rows(d, angle, B=4):
    """Per-tensor relative L2 error (and cosine) of the bf16 THROUGHPUT mode's parameter gradients against the ORACLE in
    float64, through the real objectives, at full size: G step (generator forward, ADA, discriminator, non-saturating
    loss), D step (on the oracle's own augmented reals / fakes as inputs, so that the discriminator's backward is what
    is measured and not the generator's forward on top of it), lazy R1 (double backward).  Weights by recipe, draws by
    seed, ADA draws of the fixture tiled to B.  -> {"G step": [(rel_l2, cos, name, numel)], "D step": [...], "R1": [...]}
    and the scalar rows [(what, bf16 value, float64 value)]."""
    import recipe
    from conftest import sub_dict
    from gans.models.ops import native as nat
    from oracle import augment, model, step
    H, W = 64, 512
    g = torch.Generator().manual_seed(41)
    z = torch.randn(B, 512, generator=g)
    shifts = torch.rand(B, generator=g) * 6.2831853
    u = torch.rand(B, 1, H, W, generator=g).clamp(1e-6, 1 - 1e-6)
    x_real = torch.rand(B, 1, H, W, generator=g) * 2 - 1
    tile = lambda t: torch.cat([t] * ((B + t.shape[0] - 1) // t.shape[0]))[:B]
    ada = {k: {"G": tile(d[f"{k}_adaG{s}"]), "C": tile(d[f"{k}_adaC{s}"])} for k, s in (("gs", ""), ("ds", "_real"), ("r1", ""))}
    G0, D0 = build_models(full_cfg(), "cpu")
    sdG = recipe.fill_state_dict({k: v.clone() for k, v in G0.state_dict().items()}, 1234)
    sdD = recipe.fill_state_dict({k: v.clone() for k, v in D0.state_dict().items()}, 4321)
    sdG.update(sub_dict(d, "G."))
    # ---- float64 oracle
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        f64 = lambda t: t.double() if torch.is_tensor(t) and t.is_floating_point() else t
        f64d = lambda m: {k: f64(v) for k, v in m.items()}
        sG, sD = f64d(sdG), f64d(sdD)
        ang = f64(angle.cpu()).repeat_interleave(B, 0)
        loss_g, grads_g, _, ex = step.g_step(sG, sD, f64(z), ang, f64(shifts), f64(u), ada=f64d(ada["gs"]))
        Dg = step.with_grad(sD, step.D_BUFFER_SUFFIXES)
        xr64 = augment.ada_forward(f64(x_real), f64(ada["ds"]["G"]), f64(ada["ds"]["C"]))
        y_r, y_f = model.discriminator(Dg, xr64), model.discriminator(Dg, ex["x_aug"])
        loss_d = model.loss_d_nsgan(y_r, y_f)
        keys = [k for k, v in Dg.items() if v.requires_grad]
        grads_d = dict(zip(keys, torch.autograd.grad(loss_d, [Dg[k] for k in keys])))
        r1_64, grads_r1, _ = step.r1_step(sD, f64(x_real), 16.0, ada=f64d(ada["r1"]))
    finally:
        torch.set_default_dtype(old)
    # ---- the timed mode: bf16 trunks, fp32 epilogue of D (its 3x3 conv on the bf16 matrix cores, fp32-equivalent)
    cfg = full_cfg(True)
    G, D = build_models(cfg, "cpu")
    G.load_state_dict(sdG)
    D.load_state_dict(sdD)
    G, D = G.to(DEV).train().requires_grad_(True), D.to(DEV).train().requires_grad_(False)
    A = ada_from_cfg(cfg, 0.6, DEV)
    o = G(z.to(DEV), angle=angle.to(DEV), noise={"shifts": shifts.to(DEV), "gumbel_u": u.to(DEV)})
    y_fake = D(A(o["image"], draws=ada["gs"]))
    lg = F.softplus(-y_fake).mean()
    gp = dict(G.named_parameters())
    got_g = {k: v for k, v in zip(gp, torch.autograd.grad(lg, list(gp.values()), allow_unused=True)) if v is not None}
    D.requires_grad_(True)
    y = D(torch.cat([xr64.float(), ex["x_aug"].float()]).to(DEV), splits=2)
    ld = F.softplus(-y[:B]).mean() + F.softplus(y[B:]).mean()
    dp = dict(D.named_parameters())
    got_d = dict(zip(dp, torch.autograd.grad(ld, list(dp.values()))))
    conv = D.epilogue[1]
    xin = x_real.to(DEV).clone().requires_grad_(True)
    with nat.x3_auto(True, {(conv.in_ch + 15) // 16 * 16: conv.in_ch}):
        yr = D(A(xin, draws=ada["r1"]), double_backward=True)
        (gx,) = torch.autograd.grad(yr.sum(), xin, create_graph=True)
        r1 = (gx.float() ** 2).sum(dim=[1, 2, 3]).mean()
        got_r1 = {k: v for k, v in zip(dp, torch.autograd.grad((16.0 / 2) * r1, list(dp.values()), allow_unused=True))
                  if v is not None}
    table = {}
    for name, got, want in (("G step", got_g, {k: v for k, v in grads_g.items() if v is not None}), ("D step", got_d, grads_d),
                            ("R1", got_r1, {k: v for k, v in grads_r1.items() if v is not None and k in got_r1})):
        assert set(got) >= set(want), (name, set(want) - set(got))
        table[name] = sorted(((_l2(got[k].reshape(want[k].shape), want[k]), _cos(got[k], want[k]), k, want[k].numel())
                              for k in want), reverse=True)
    scalars = [("loss_G", float(lg), float(loss_g)), ("loss_D", float(ld), float(loss_d)), ("R1 penalty", float(r1), float(r1_64)),
               ("y_fake max |err|", float((y_fake.double().cpu() - ex["y_fake"]).abs().max()), float(ex["y_fake"].abs().max()))]
    return table, scalars


def format_bf16_table(table, scalars):
    out = ["bf16 throughput mode against the oracle in float64, through the real objectives, 64x512 full widths, B = 4",
           "(tests/test_gpu_full.py::bf16_vs_f64_rows; relative L2 error and cosine per parameter-gradient tensor)", ""]
    for what, a, b in scalars:
        out.append(f"  {what:22s} bf16 mode {a: .6e}   float64 {b: .6e}")
    for name, rows in table.items():
        errs = sorted(r[0] for r in rows)
        flat = lambda i: None
        out.append("")
        out.append(f"== {name}: {len(rows)} tensors, rel-L2 median {errs[len(errs) // 2]:.2e}, 90th percentile "
                   f"{errs[int(0.9 * (len(errs) - 1))]:.2e}, worst {errs[-1]:.2e}; lowest cosine {min(r[1] for r in rows):.5f}")
        for e, c, k, n in rows:
            out.append(f"   {k:64s} {n:9d}  rel-L2 {e:.3e}  cos {c:.5f}")
    return "\n".join(out)


def test_bf16_gradients_against_the_float64_oracle_per_tensor(g_full, angle):
    """The timed mode held DIRECTLY to the float64 oracle, per tensor, through the real losses (beside the fp32-mode
    comparison above, which is transitive).  The committed table profiles/round6_bf16_vs_f64_table.txt is this function's
    output on the GPU box (scripts/bf16_grad_table.py); the bounds sit at about twice its worst row per class, "small" =
    biases and tensors of <= 4096 elements (sums over the whole map that nearly cancel):
      class     measured worst (rel-L2 / cosine)         bound
      G step    large 0.134 / 0.9919, small 0.175 / 0.991   large 0.25 / 0.98, small 0.35 / 0.97
      D step    large 0.053 / 0.9986, small 0.063 / 0.998   all 0.12 / 0.995
      R1        large 0.066 / 0.9978, small 0.257 / 0.969   large 0.15 / 0.99, small 0.5 / 0.93
    (the G step runs through the hard ray-drop threshold and the whole discriminator: its figures are end-to-end, not
    per-kernel; R1 differentiates every bf16 rounding of the first pass again, and its bias gradients are pure
    second-order terms); the losses within 5e-3, the penalty within 2e-2."""
    table, scalars = bf16_vs_f64_rows(g_full, angle, B=4)
    print(format_bf16_table(table, scalars))
    small = lambda k, n: k.endswith("bias") or n <= 4096
    bounds = {"G step": ((0.25, 0.98), (0.35, 0.97)), "D step": ((0.12, 0.995), (0.12, 0.995)), "R1": ((0.15, 0.99), (0.5, 0.93))}
    for name, (big, sm) in bounds.items():
        bad = [(k, e, c) for e, c, k, n in table[name]
               if e > (sm if small(k, n) else big)[0] or c < (sm if small(k, n) else big)[1]]
        assert not bad, (name, bad)
    for what, a, b in scalars[:2]:
        assert abs(a - b) <= 5e-3 * abs(b), (what, a, b)
    assert abs(scalars[2][1] - scalars[2][2]) <= 2e-2 * abs(scalars[2][2]), scalars[2]
