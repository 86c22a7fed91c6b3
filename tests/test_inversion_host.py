"""Host side of GAN inversion (gans/inversion.py, demo_inversion.py) against tests/golden/inversion.npz, which the
reference wrote (tests/golden/make_inversion_golden.py).  CPU only: nothing here reaches a kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, PKG, ROOT


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "inversion.npz"))
    return {k: d[k] for k in d.files}


def test_exports():
    import gans.inversion as inv
    for name in ("MultiScaleMaskedLoss", "SphericalOptimizer", "geocross_loss", "normalize_noise_", "invert"):
        assert callable(getattr(inv, name)), name


def test_state_dict_layout_matches_reference(gold):
    from gans.inversion import MultiScaleMaskedLoss
    crit = MultiScaleMaskedLoss(F.l1_loss, level=2)
    assert list(crit.state_dict().keys()) == list(gold["msml.state_dict_keys"])
    assert [k for k, _ in crit.named_buffers()] == list(gold["msml.buffer_names"])
    for k, v in crit.state_dict().items():
        want = torch.from_numpy(gold[f"msml.state_dict.{k}"])
        assert v.shape == want.shape and v.dtype == want.dtype and torch.equal(v, want), k


def test_unsupported_loss_fn_is_refused():
    from gans.inversion import MultiScaleMaskedLoss
    with pytest.raises(NotImplementedError) as e:
        MultiScaleMaskedLoss(F.smooth_l1_loss)
    assert "l1_loss" in str(e.value) and "mse_loss" in str(e.value)
    MultiScaleMaskedLoss(F.l1_loss)
    MultiScaleMaskedLoss(F.mse_loss, level=3, relative=False)


def test_loss_fails_loudly_on_cpu_tensors():
    from gans.inversion import MultiScaleMaskedLoss
    crit = MultiScaleMaskedLoss(F.l1_loss, level=2)
    x = torch.rand(1, 1, 8, 16)
    with pytest.raises(RuntimeError):
        crit(x, x.clone(), torch.ones(1, 1, 8, 16))


def test_lr_schedule(gold):
    from gans.inversion import lr_schedule
    for tag in ("a", "b"):
        n, up, down = gold[f"lr.{tag}"]
        want = gold[f"lr.{tag}.values"]
        got = np.array([lr_schedule(i, int(n), up, down) for i in range(int(n))])
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
    assert lr_schedule(0, 500) == 0.0


def test_spherical_optimizer(gold):
    from gans.inversion import SphericalOptimizer
    p = torch.nn.Parameter(torch.from_numpy(gold["spherical.p0"]).clone())
    opt = SphericalOptimizer([p], lr=0.05)
    for g in torch.from_numpy(gold["spherical.grads"]):
        p.grad = g.clone()
        opt.step()
    want = torch.from_numpy(gold["spherical.p3"])
    assert float((p.detach() - want).abs().max()) < 1e-6
    assert torch.allclose(p.detach().pow(2).mean(-1), torch.ones(2, 6), atol=1e-5)


def test_geocross_loss(gold):
    from gans.inversion import geocross_loss
    lat = torch.from_numpy(gold["geocross.latents"]).double().requires_grad_(True)
    v = geocross_loss(lat)
    (g,) = torch.autograd.grad(v.sum(), lat)
    assert float((v.detach() - torch.from_numpy(gold["geocross.value"])).abs().max()) < 1e-12
    assert float((g - torch.from_numpy(gold["geocross.grad"])).abs().max()) < 1e-12


def test_normalize_noise():
    from gans.inversion import normalize_noise_
    n = [torch.randn(1, 1, 8, 16, generator=torch.Generator().manual_seed(1)) * 3 + 2]
    normalize_noise_(n)
    assert abs(float(n[0].mean())) < 1e-6 and abs(float(n[0].std()) - 1) < 1e-6
    normalize_noise_([])


def test_cli_help_parses():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo_inversion.py"), "--help"], capture_output=True,
                       text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--ckpt_path", "--sample_id", "--latent_type", "--num_steps_1st", "--num_steps_2nd", "--lr_1st",
                "--lr_1st_rampup_ratio", "--lr_1st_rampdown_ratio", "--lr_2nd", "--noise_ratio", "--noise_coef",
                "--optimize_phase", "--perturb_z", "--hypersphere_z", "--device", "--seed", "--synthetic"):
        assert opt in r.stdout, opt
    assert "--visualize" not in r.stdout


def test_cli_imports_no_display_packages():
    src = open(os.path.join(ROOT, "demo_inversion.py")).read()
    for mod in ("cv2", "rich", "tqdm", "torchvision"):
        assert f"import {mod}" not in src and f"from {mod}" not in src, mod
