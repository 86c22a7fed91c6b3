"""ADA's image-space stages (band filter, additive noise, cutout; reference adaptive_augment.py:547-621) on the GPU:
the fold of the filter into the separable operators and the one-launch apply, through AdaptiveAugment's public
interface, against tests/golden/ada_imgspace.npz -- the reference's own float64 forward with every draw recorded
(tests/golden/make_ada_imgspace_golden.py, which asserts the conditioning the cases rely on: per case a sample with each
stage on and one with it off, a flipped sample under the filter, boxes that remove 5-50 % and no pixel centre on a box
edge).  Shapes: a [3,1,24,96] LDS kernel, two column tiles, ring seam; b [2,1,26,64] generic kernel (H % 4 != 0) with
W < K' = 74; c [2,1,64,512] the model's shape.

Tolerance per case and quantity: 4 x the reference's own float32-vs-float64 deviation recorded in the fixture, floor
5e-5 relative (the existing ADA parity bound), error measured as max |got - want| / max |want|.
"""
import math
import os

import numpy as np
import pytest
import torch

import ada_imgspace_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEO = dict(lr_flip=1, ud_flip=1, int_trans=1, iso_scale=1, frac_trans=1, brightness=1, contrast=1, luma_flip=1, hue=1,
           saturation=1)


def rel_err(got, want):
    return float((got.detach().double().cpu() - want.double()).abs().max() / (want.double().abs().max() + 1e-30))


@pytest.fixture(scope="module")
def fx():
    d = np.load(os.path.join(GOLDEN, "ada_imgspace.npz"))
    return {k: (d[k] if d[k].dtype.kind in "US" else torch.from_numpy(d[k])) for k in d.files}


def policy(fx):
    return dict(zip([str(k) for k in fx["policy.keys"]], [float(v) for v in fx["policy.values"]]))


def draws_of(fx, tag):
    return {k: fx[f"{tag}.{k}"] for k in ("G", "C", "g", "sigma", "cut", "eps")}


def augment(fx, **over):
    from gans.augment.adaptive_augment import AdaptiveAugment
    return AdaptiveAugment(p_init=float(fx["p"]), **{**policy(fx), **over}).to(DEV)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_forward_gradient_and_double_backward_match_the_reference(fx, tag):
    A = augment(fx)
    dev = [float(v) for v in fx[f"{tag}.dev"]]
    tol = [max(4 * v, 5e-5) for v in dev]
    xd = fx[f"{tag}.x"].to(DEV).requires_grad_(True)
    y = A(xd, draws=draws_of(fx, tag))
    e = rel_err(y, fx[f"{tag}.y"])
    print(f"case {tag}: forward rel err {e:.3e} (reference fp32-vs-fp64 {dev[0]:.2e}, bound {tol[0]:.1e})")
    assert e <= tol[0]
    if f"{tag}.cot" not in fx:
        return
    gyd = fx[f"{tag}.cot"].to(DEV).requires_grad_(True)
    (gx,) = torch.autograd.grad(y, xd, gyd, create_graph=True)
    e = rel_err(gx, fx[f"{tag}.grad"])
    print(f"case {tag}: gradient rel err {e:.3e} (reference {dev[1]:.2e}, bound {tol[1]:.1e})")
    assert e <= tol[1]
    (ggy,) = torch.autograd.grad(gx, gyd, xd.detach())     # = J x: the forward without the offset and the noise
    e = rel_err(ggy, fx[f"{tag}.lin"])
    print(f"case {tag}: double backward rel err {e:.3e} (reference {dev[2]:.2e}, bound {tol[2]:.1e})")
    assert e <= tol[2]


@pytest.mark.parametrize("stage", ["imgfilter", "noise", "cutout"])
def test_each_stage_alone(fx, stage):
    """One multiplier positive, the other two zero, at [3,1,24,96]: the reference's float64 output of the stages before
    (fixture) through the float64 restatement of that one stage."""
    off = {k: 0.0 for k in ("imgfilter", "noise", "cutout") if k != stage}
    A = augment(fx, **off)
    d = draws_of(fx, "a")
    kw = {"imgfilter": dict(g=d["g"]), "noise": dict(sigma=d["sigma"], eps=d["eps"]), "cutout": dict(cut=d["cut"])}[stage]
    want = R.image_space_f64(fx["a.y_geo"], fx["Hz_fbank"], **kw)
    assert rel_err(want, fx["a.y_geo"]) > 1e-2              # the stage does something in this case
    xd = fx["a.x"].to(DEV).requires_grad_(True)
    y = A(xd, draws=d)
    e = rel_err(y, want)
    print(f"{stage} alone: rel err {e:.3e}")
    assert e <= max(4 * float(fx["a.dev"][0]), 5e-5)
    # the adjoint of that stage alone: <A'(x) v, w> = <v, A'(x)^T w>
    gen = torch.Generator().manual_seed(3)
    v, w = torch.randn(xd.shape, generator=gen).to(DEV), torch.randn(xd.shape, generator=gen).to(DEV).requires_grad_(True)
    (gx,) = torch.autograd.grad(y, xd, w, create_graph=True)
    (jv,) = torch.autograd.grad(gx, w, v)
    lhs, rhs = float((jv.double() * w.detach().double()).sum()), float((v.double() * gx.detach().double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), abs(rhs))


def test_all_selects_off_is_the_plain_path(fx):
    """All three multipliers positive, no select drawn (raw uniforms above p x mul): unit gains fold to a delta, sigma and
    the box size are 0 -- the geometric + colour path to 1e-5 relative, through the 74-tap kernels."""
    A, plain = augment(fx), augment(fx, imgfilter=0.0, noise=0.0, cutout=0.0)
    x = fx["a.x"].to(DEV)
    B = x.shape[0]
    gen = torch.Generator().manual_seed(4)
    u2 = torch.full((B, 8), 0.95)
    u2[:, 6:] = torch.rand(B, 2, generator=gen)
    d = {"G": fx["a.G"], "C": fx["a.C"], "u2": u2.to(DEV), "n2": torch.randn(B, 8, generator=gen).to(DEV),
         "eps": torch.randn(x.shape, generator=gen).to(DEV)}
    want = plain(x, draws={"G": fx["a.G"], "C": fx["a.C"]})
    got = A(x, draws=d)
    e = rel_err(got, want.cpu())
    print(f"selects off vs plain path: rel err {e:.3e}")
    assert e <= 1e-5


def test_out_argument_and_raw_draws_agree_with_the_parity_form(fx):
    """The raw form {u2, n2, eps} goes through dgv2_ada_sample_img; feeding its (g, sigma, cut) back as the parity form
    gives the same bits, also when written through `out`."""
    from gans.augment.adaptive_augment import AdaptiveAugment
    A = AdaptiveAugment(p_init=0.9, imgfilter=1, noise=1, cutout=1, **GEO).to(DEV)
    x = fx["a.x"].to(DEV)
    B = x.shape[0]
    gen = torch.Generator(device=DEV).manual_seed(6)
    u2, n2 = torch.rand(B, 8, device=DEV, generator=gen), torch.randn(B, 8, device=DEV, generator=gen)
    eps = torch.randn(x.shape, device=DEV, generator=gen)
    from gans.models.ops import native
    g, sigma, cut = native.ada_sample_img(B, A.p.reshape(1), A.image_policy_vector(), DEV, u2=u2, n2=n2)
    raw = A(x, draws={"G": fx["a.G"], "C": fx["a.C"], "u2": u2, "n2": n2, "eps": eps})
    out = torch.empty_like(x)
    with torch.no_grad():
        A(x, draws={"G": fx["a.G"], "C": fx["a.C"], "g": g, "sigma": sigma, "cut": cut, "eps": eps}, out=out)
    assert torch.equal(raw, out)


def test_image_space_sampling_statistics():
    """20 000 draws of the fused sampler.  Exactness first: for raw draws we make ourselves, g is the sequential
    normalisation of tests/ada_imgspace_ref.band_gains.  Then the distributions of the path forward() samples from."""
    from gans.augment.adaptive_augment import AdaptiveAugment
    from gans.models.ops import native
    torch.manual_seed(0)
    n, p, mul = 20000, 0.5, dict(imgfilter=0.6, noise=0.8, cutout=1.0)
    A = AdaptiveAugment(p_init=p, **mul).to(DEV)
    u2, n2 = torch.rand(n, 8, device=DEV), torch.randn(n, 8, device=DEV)
    g, sigma, cut = native.ada_sample_img(n, A.p.reshape(1), A.image_policy_vector(), DEV, u2=u2, n2=n2)
    sel = (u2[:, :4] < np.float32(mul["imgfilter"]) * np.float32(p)).cpu()
    want = R.band_gains(sel, n2[:, :4].cpu())
    assert float(((g.cpu().double() - want).abs() / want).max()) <= 1e-5
    on = ((g.cpu().double() - 1).abs() > 1e-6).any(1)             # some band selected: 1 - (1 - p x mul)^4 within 0.02
    assert abs(float(on.float().mean()) - (1 - (1 - p * mul["imgfilter"]) ** 4)) < 0.02
    # the sampling path of forward(): its own generator calls
    g, sigma, cut = (t.cpu().double() for t in A.sample_image_params(n, DEV))
    assert abs(float((sigma > 0).float().mean()) - p * mul["noise"]) < 0.02
    assert abs(float((cut[:, 2] > 0).float().mean()) - p * mul["cutout"]) < 0.02
    assert torch.equal(cut[:, 2], cut[:, 3]) and set(cut[:, 2].unique().tolist()) == {0.0, 0.5}
    none = (g - 1).abs().max(dim=1).values < 1e-6
    assert abs(float(none.float().mean()) - (1 - p * mul["imgfilter"]) ** 4) < 0.02
    # a single selected band i: the other three share 1/den, so t = g_i / g_other; its log2 is N(0, imgfilter_std = 1)
    # BEFORE normalisation, and g_i is the closed form t / sqrt(1 - e_i + e_i t^2)
    logs = []
    for i in range(4):
        others = [k for k in range(4) if k != i]
        same = (g[:, others].max(dim=1).values - g[:, others].min(dim=1).values) < 1e-6
        single = same & ((g[:, i] - g[:, others[0]]).abs() > 1e-6)
        lt = torch.log2(g[single, i] / g[single, others[0]])
        assert float(((g[single, i] - R.single_band_gain(i, lt)).abs() / g[single, i]).max()) <= 1e-5
        assert abs(float(single.float().mean()) - p * mul["imgfilter"] * (1 - p * mul["imgfilter"]) ** 3) < 0.02
        logs.append(lt)
    logs = torch.cat(logs)
    assert logs.numel() > 5000 and abs(float(logs.std()) - 1.0) < 0.05 and abs(float(logs.mean())) < 0.05
    s = sigma[sigma > 0] / 0.1                                     # half-normal: mean sqrt(2 / pi)
    assert abs(float(s.mean()) / math.sqrt(2 / math.pi) - 1) < 0.03
    for k in (0, 1):                                               # centres: uniform on [0, 1)
        c = cut[:, k]
        assert float(c.min()) >= 0 and float(c.max()) < 1
        assert abs(float(c.mean()) - 0.5) < 0.01 and abs(float(c.std()) / math.sqrt(1 / 12) - 1) < 0.03
        assert abs(float((c < 0.25).float().mean()) - 0.25) < 0.02 and abs(float((c > 0.9).float().mean()) - 0.1) < 0.02


# ---------------------------------------------------------------------------- trainer
def _trainer(hip_graph):
    from gans.trainer import Trainer
    from helpers import small_cfg
    cfg = small_cfg()
    # the small configuration at 32 rows: the band filter's reflect padding of 21 needs H >= 22
    cfg.model.generator.synthesis_kwargs.update(resolution=[32, 64])
    cfg.model.discriminator.layer_kwargs.update(resolution=[32, 64])
    cfg.dataset.name = "synthetic"
    cfg.training.update(rank=0, num_gpus=1, batch_size=8, batch_size_per_gpu=8, resume=None, hip_graph=hip_graph)
    cfg.training.lazy.update(gp=2, ada=2)
    cfg.training.augment.update(p_init=0.6, kimg=1)
    cfg.training.augment.policy.update(imgfilter=1, noise=1, cutout=1)
    cfg.training.warmup.fade_kimg = 0
    torch.manual_seed(0)
    np.random.seed(0)
    return Trainer(cfg, sync_scalars=False)


def test_trainer_iteration_replays_with_injected_image_space_draws():
    """One iteration (G, D) and the next (+ R1) of the small configuration with the three multipliers on, every draw
    injected through set_draws (raw u2 / n2 / eps next to the parity G / C): eagerly and as hipGraph replays from the same
    state.  Iteration 1 starts from identical weights and must agree to the bound of
    test_full_size_bf16_graph_replay_equals_eager for that iteration (1e-6 relative).  A further replay with another eps
    must move the output: the graph reads the static buffers set_draws fills."""
    import copy
    eager, graph = _trainer(False), _trainer(True)
    B, (H, W) = eager.B, eager.resolution
    assert (H, W) == (32, 64) and eager.A.image_space_on()
    init = {n: copy.deepcopy(m.state_dict()) for n, m in (("G", eager.G), ("D", eager.D), ("Gema", eager.G_ema))}
    gen = torch.Generator(device=DEV).manual_seed(5)
    rnd = lambda *s: torch.rand(*s, device=DEV, generator=gen)
    randn = lambda *s: torch.randn(*s, device=DEV, generator=gen)
    nz = int(eager.cfg.model.generator.mapping_kwargs.in_ch)

    def make_draws():
        dr = {"g.z": randn(B, nz), "d.z": randn(B, nz)}
        for s in ("g", "d"):
            dr[s + ".shifts"] = rnd(B) * 6.2831853
            dr[s + ".u"] = rnd(B, 1, H, W).clamp(1e-6, 1 - 1e-6)
        for s in ("g.ada", "d.ada_real", "d.ada_fake", "r1.ada"):
            dr[s + ".G"] = eager.A.sample_affine(B, H, W, device=DEV)
            dr[s + ".C"] = eager.A.sample_color(B, device=DEV)
            dr[s + ".u2"], dr[s + ".n2"], dr[s + ".eps"] = rnd(B, 8), randn(B, 8), randn(B, 1, H, W)
        return dr

    draws = [make_draws(), make_draws()]
    reals = [{"depth": rnd(B, 1, H, W) * 78.55 + 1.45, "mask": (rnd(B, 1, H, W) < 0.85).float()} for _ in range(2)]

    def reset(tr):
        tr.G.load_state_dict(init["G"])
        tr.D.load_state_dict(init["D"])
        tr.G_ema.load_state_dict(init["Gema"])
        with torch.no_grad():
            tr.A.p.fill_(0.6)
            tr.A.sign_cum.zero_()
            tr.A.n_pred_cum.zero_()
            for opt in (tr.optim_G, tr.optim_D):
                for st in opt.state.values():
                    for v in st.values():
                        if torch.is_tensor(v):
                            v.zero_()
                if getattr(opt, "_dgv2_step", None) is not None:
                    opt._dgv2_step.zero_()

    def run(tr, its, dr=draws):
        outs = []
        for it in its:
            k = (it - 1) % 2
            tr.iter_train_loader = iter([reals[k]])
            tr.set_draws(dr[k])
            outs.append({n: float(v) for n, v in tr.step(it).items()})
        return outs

    run(graph, range(1, 7))          # two eager warm runs + the captures
    assert len(graph._graphs) == 3 and all(v is not None for v in graph._graphs.values()), graph._graphs.keys()
    reset(eager)
    e = run(eager, (1, 2))
    reset(graph)
    r = run(graph, (1, 2))
    assert set(e[0]) == set(r[0]) and set(e[1]) == set(r[1]) and "loss/D/gradient_penalty" in r[1]
    assert all(math.isfinite(v) for o in e + r for v in o.values())
    for k in ("loss/G/adversarial", "loss/D/output/real"):
        assert abs(e[0][k] - r[0][k]) <= 1e-6 * abs(e[0][k]), ("iteration 1", k, e[0][k], r[0][k])
    # another eps, everything else the same: the replayed bodies must see it
    other = [dict(d) for d in draws]
    for s in ("g.ada", "d.ada_real", "d.ada_fake", "r1.ada"):
        other[0][s + ".eps"] = randn(B, 1, H, W)
    reset(graph)
    r2 = run(graph, (1,), other)
    assert r2[0]["loss/D/output/real"] != r[0]["loss/D/output/real"]
    assert r2[0]["loss/G/adversarial"] != r[0]["loss/G/adversarial"]
