"""CPU checks of the CRF-RNN layer (semseg/models/crf_as_rnn.py): the float64 restatement tests/crf_ref.py against the
reference's own float64 results in tests/golden/crf_rnn.npz (tests/golden/make_crf_golden.py), and the module's
state-dict layout, buffers and argument checks.  No kernel runs here."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from crf_ref import from_state_dict

RESULTS = ("out", "g_unary", "g_weight_smoothness", "g_weight_appearance", "g_label_compatibility.weight")


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "crf_rnn.npz"))
    return {k: d[k] for k in d.files}


def case_of(gold, name):
    B, C, H, W, kh, kw, iters = (int(v) for v in gold[f"{name}.shape"])
    sd = {k[len(name) + 4:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(f"{name}.sd.")}
    return (B, C, H, W), (kh, kw), iters, sd


def module_for(gold, name):
    from semseg.models.crf_as_rnn import CRFRNN
    (B, C, H, W), ks, iters, sd = case_of(gold, name)
    return CRFRNN(C, kernel_size=ks, theta_gamma=sd["theta_gamma"].tolist(), theta_alpha=sd["theta_alpha"].tolist(),
                  theta_beta=sd["theta_beta"].tolist(), num_iters=iters), sd


def test_fixture_holds_the_seven_cases(gold):
    shapes = [tuple(int(v) for v in gold[f"{n}.shape"]) for n in gold["cases"]]
    assert shapes == [(2, 3, 5, 9, 3, 5, 3), (1, 4, 3, 5, 3, 5, 3), (1, 2, 1, 7, 3, 5, 3), (1, 3, 4, 6, 1, 3, 1),
                      (1, 2, 6, 7, 5, 3, 3), (1, 3, 33, 130, 3, 5, 3), (1, 8, 4, 6, 3, 5, 3)]


def test_crf_ref_matches_the_reference_in_float64(gold):
    bad = []
    for name in gold["cases"]:
        _, _, iters, sd = case_of(gold, name)
        sd = {k: v.double() for k, v in sd.items()}
        leaves = [sd[k].requires_grad_(True) for k in ("weight_smoothness", "weight_appearance", "label_compatibility.weight")]
        unary = torch.from_numpy(gold[f"{name}.unary"]).double().requires_grad_(True)
        out = from_state_dict(sd, unary, torch.from_numpy(gold[f"{name}.xyz"]).double(),
                              torch.from_numpy(gold[f"{name}.mask"]).double(), iters)
        grads = torch.autograd.grad((out * torch.from_numpy(gold[f"{name}.cot"]).double()).sum(), [unary] + leaves)
        for key, got in zip(RESULTS, (out.detach(),) + grads):
            err = float((got - torch.from_numpy(gold[f"{name}.{key}.f64"])).abs().max())
            print(f"{name} {key}: max abs deviation {err:.2e}")
            if not err <= 1e-12:
                bad.append((name, key, err))
    assert not bad, bad


def test_state_dict_keys_and_shapes(gold):
    for name in gold["cases"]:
        crf, _ = module_for(gold, name)
        sd = crf.state_dict()
        want = dict(zip(gold["sd_keys"].tolist(), gold[f"{name}.sd_shapes"].tolist()))
        assert {k: ",".join(map(str, v.shape)) for k, v in sd.items()} == want
        assert all(v.dtype == torch.float32 for v in sd.values())


def test_reference_state_dict_loads_strictly(gold):
    for name in gold["cases"]:
        crf, sd = module_for(gold, name)
        crf.load_state_dict(sd, strict=True)
        for k, v in crf.state_dict().items():
            assert torch.equal(v, sd[k]), k
        assert {k for k, _ in crf.named_parameters()} == {"weight_appearance", "weight_smoothness",
                                                          "label_compatibility.weight"}


def test_gaussian_buffers_equal_the_reference(gold):
    for name in gold["cases"]:
        crf, sd = module_for(gold, name)
        for k in ("kernel_gamma", "kernel_alpha", "theta_gamma", "theta_alpha", "theta_beta"):
            err = float((getattr(crf, k) - sd[k]).abs().max())
            assert err <= 1e-7, (name, k, err)
        kh, kw = crf.kernel_size
        assert float(crf.kernel_gamma[:, :, kh // 2, kw // 2].abs().max()) == 0.0


def test_defaults_are_the_reference_defaults():
    from semseg.models import CRFRNN
    crf = CRFRNN(4)
    assert crf.kernel_size == (3, 5) and crf.padding == (1, 2) and crf.num_iters == 3 and crf.num_classes == 4
    assert torch.equal(crf.weight_smoothness, torch.full((1, 4, 1, 1), 0.02))
    assert torch.equal(crf.weight_appearance, torch.full((1, 4, 1, 1), 0.1))
    assert torch.equal(crf.label_compatibility.weight[:, :, 0, 0], 1 - torch.eye(4))
    assert torch.equal(crf.theta_beta, torch.full((4,), 0.015)) and torch.equal(crf.theta_gamma, torch.full((4,), 0.9))
    assert CRFRNN(2, kernel_size=3).kernel_size == (3, 3)


def test_apply_returns_the_module_untouched():
    from semseg.models import CRFRNN
    crf = CRFRNN(3)
    before = {k: v.clone() for k, v in crf.state_dict().items()}
    calls = []

    def init(m):
        calls.append(m)
        if hasattr(m, "weight"):
            torch.nn.init.zeros_(m.weight)
    assert crf.apply(init) is crf and not calls
    assert all(torch.equal(v, before[k]) for k, v in crf.state_dict().items())
    # inside a backbone the shield holds too
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 3, 1), crf)
    net.apply(init)
    assert len(calls) == 2 and crf not in calls and float(net[0].weight.detach().abs().max()) == 0.0
    assert all(torch.equal(v, before[k]) for k, v in crf.state_dict().items())


def test_argument_checks():
    from gans.models.ops.native.crf import C_MAX
    from semseg.models import CRFRNN
    assert C_MAX >= 8
    for ks in ((2, 5), (3, 4), 4):
        with pytest.raises(ValueError):
            CRFRNN(3, kernel_size=ks)
    with pytest.raises(ValueError):
        CRFRNN(C_MAX + 1)
    with pytest.raises(ValueError):
        CRFRNN(3, kernel_size=(7, 5))
    with pytest.raises(ValueError):
        CRFRNN(3, kernel_size=(3, 11))
    crf = CRFRNN(3)
    u, xyz, m = torch.zeros(1, 3, 4, 6), torch.zeros(1, 3, 4, 6), torch.ones(1, 4, 6)
    with pytest.raises(RuntimeError):       # CPU tensors: there is no CPU path
        crf(u, xyz, m)
    with pytest.raises(ValueError):
        crf(u, torch.zeros(1, 3, 4, 7), m)
    with pytest.raises(ValueError):
        crf(u, xyz, torch.ones(1, 2, 4, 6))
    with pytest.raises(ValueError):
        crf(torch.zeros(1, 4, 4, 6), xyz, m)
    crf.num_iters = 0
    assert crf(u, xyz, m) is u
