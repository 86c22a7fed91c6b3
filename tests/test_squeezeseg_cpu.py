"""CPU checks of the SqueezeSeg trunks (semseg/models/squeezeseg_v1.py, squeezeseg_v2.py, common.py): the plain-torch
restatement of the Fire forward against the reference's fixture, the state-dict layout, the modules' composition path
in float64 against the reference's float64 logits, the initialisers, the local-only SqueezeNet loading and the native
wrapper's argument checks.  Needs the built library (the package imports dgv2_native), no GPU."""
import inspect
import os

import numpy as np
import pytest
import torch

import squeezeseg_ref as R
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fx():
    d = np.load(os.path.join(GOLDEN, "squeezeseg.npz"))
    return {k: d[k] for k in d.files}


def _our_fire(i):
    from semseg.models import squeezeseg_v1, squeezeseg_v2
    ver, B, Cin, Cs, E, H, W, up = R.FIRE_CASES[i]
    fire = squeezeseg_v1.Fire(Cin, Cs, E, E, up=up) if ver == 1 else squeezeseg_v2.Fire(Cin, Cs, E, E, 0.001, up=up)
    sd = R.hash_fill_state_dict(fire.state_dict(), salt=R.fire_case_name(i) + "/")
    fire.load_state_dict(sd, strict=True)
    return fire.eval(), sd


def _our_model(i):
    from semseg.models import SqueezeSegV1, SqueezeSegV2
    ver, B, H, W, crf = R.MODEL_CASES[i]
    if ver == 1:
        model = SqueezeSegV1(R.MODEL_INPUTS, R.MODEL_CLASSES, use_crf=crf)
    else:
        model = SqueezeSegV2(R.MODEL_INPUTS, R.MODEL_CLASSES, use_crf=crf, pretrained_weights=False)
    model.load_state_dict(R.hash_fill_state_dict(model.state_dict(), salt=f"v{ver}/"), strict=True)
    return model.eval()


def test_hash_fill_is_pinned():
    """The fill is part of the fixture: three values written down when it was generated."""
    v = R.hash_uniform("pin", 3)
    assert v.dtype == np.float64 and np.all((v >= 0) & (v < 1))
    assert [float(t).hex() for t in v] == ["0x1.e416ae004e230p-1", "0x1.08b69d0b7c140p-7", "0x1.618eaee360628p-2"]
    assert np.array_equal(v, R.hash_uniform("pin", 5)[:3])
    assert not np.array_equal(R.hash_uniform("pin", 3), R.hash_uniform("pim", 3))


@pytest.mark.parametrize("i", range(len(R.FIRE_CASES)))
def test_restatement_matches_fixture(fx, i):
    name = R.fire_case_name(i)
    fire, sd = _our_fire(i)
    y = R.fire_ref(sd, R.fire_case_input(i))
    idx = R.sample_index(name, y.numel())
    ref64 = torch.from_numpy(fx[name + "/ref64"])
    dev = float((y.flatten()[idx] - ref64).abs().max())
    print(f"{name}: restatement deviation {dev:.2e}, max|ref64| {float(fx[name + '/max64']):.3f}")
    assert dev <= 1e-12 * float(fx[name + "/max64"])
    assert abs(float(y.abs().max()) - float(fx[name + "/max64"])) <= 1e-12 * float(fx[name + "/max64"])


@pytest.mark.parametrize("i", range(len(R.FIRE_CASES)))
def test_fire_module_composition_float64(fx, i):
    name = R.fire_case_name(i)
    fire, sd = _our_fire(i)
    with torch.no_grad():
        y = fire.double()(R.fire_case_input(i).double())
    idx = R.sample_index(name, y.numel())
    dev = float((y.flatten()[idx] - torch.from_numpy(fx[name + "/ref64"])).abs().max())
    assert dev <= 1e-12 * float(fx[name + "/max64"])


@pytest.mark.parametrize("ver,crf", [(1, False), (1, True), (2, False), (2, True)])
def test_state_dict_listing(fx, ver, crf):
    from semseg.models import SqueezeSegV1, SqueezeSegV2
    if ver == 1:
        model = SqueezeSegV1(R.MODEL_INPUTS, R.MODEL_CLASSES, use_crf=crf)
    else:
        model = SqueezeSegV2(R.MODEL_INPUTS, R.MODEL_CLASSES, use_crf=crf, pretrained_weights=False)
    want = [str(s) for s in fx[f"listing_v{ver}{'_crf' if crf else ''}"]]
    assert R.listing(model.state_dict()) == want


@pytest.mark.parametrize("i", [i for i, c in enumerate(R.MODEL_CASES) if not c[4]])
def test_model_composition_float64(fx, i):
    name = R.model_case_name(i)
    model = _our_model(i).double()
    img = torch.from_numpy(fx[name + "/img"])
    assert torch.equal(img, R.model_case_inputs(i)[0])
    with torch.no_grad():
        logit = model(img.double())
    ref64 = torch.from_numpy(fx[name + "/logit64"])
    dev = float((logit - ref64).abs().max())
    print(f"{name}: deviation {dev:.2e}, max|ref64| {float(ref64.abs().max()):.3f}")
    assert logit.shape == ref64.shape and dev <= 1e-12 * float(ref64.abs().max())


def test_constructor_defaults_and_initialisation():
    from semseg.models import SqueezeSegV1, SqueezeSegV2
    sig = inspect.signature(SqueezeSegV2.__init__).parameters
    assert sig["bn_momentum"].default == 0.001 and sig["head_dropout_p"].default == 0.5
    assert sig["pretrained_weights"].default is True and sig["crf_kernel_size"].default == (3, 5)
    assert "bn_momentum" not in inspect.signature(SqueezeSegV1.__init__).parameters
    torch.manual_seed(0)
    m2 = SqueezeSegV2(["xyz", "depth"], 4, pretrained_weights=None)
    w_enc = m2.encoder["fire_6_9"][4].expand3x3[0].weight.detach()
    w_dec = m2.decoder["fire_10"].expand3x3[0].weight.detach()
    assert 0.0005 < float(w_enc.std()) < 0.0015
    assert 0.05 < float(w_dec.std()) < 0.15
    assert float(m2.encoder["fire_2_3"][2].attn[1].weight.detach().abs().max()) > 0.05                    # CAM: xavier, not 0.001
    assert all(float(m.bias.detach().abs().max()) == 0 for m in m2.modules() if isinstance(m, torch.nn.Conv2d) and m.bias is not None)
    assert m2.encoder["conv_1a"][0][2].momentum == 0.001 and m2.decoder["head"][0].p == 0.5
    m1 = SqueezeSegV1(["xyz", "depth"], 4)
    assert 0.0005 < float(m1.fire10.expand3x3[0].weight.detach().std()) < 0.0015


def test_deconv_keeps_bilinear_kernel():
    from semseg.models import SqueezeSegV1
    from semseg.models.common import DeconvReLU, init_weights_trunc_normal
    want = torch.tensor([1.0, 3.0, 3.0, 1.0]) / 4

    def check(deconv):
        w = deconv[0].weight
        C = w.shape[0]
        assert tuple(w.shape) == (C, C, 1, 4)
        for c in range(C):
            assert torch.equal(w[c, c, 0], want)
        off = w.detach().clone()
        off[torch.arange(C), torch.arange(C)] = 0
        assert float(off.abs().max()) == 0 and float(deconv[0].bias.detach().abs().max()) == 0

    d = DeconvReLU(16, 16, (1, 4), (1, 2), (0, 1))
    check(d)
    assert d.apply(init_weights_trunc_normal) is d
    check(d)
    model = SqueezeSegV1(["xyz", "depth"], 4)
    model.apply(lambda m: torch.nn.init.constant_(m.weight, 7.0) if isinstance(m, torch.nn.ConvTranspose2d) else None)
    for fire in (model.fire10, model.fire11, model.fire12, model.fire13):
        check(fire.upsample)
    # the bilinear kernel doubles the width exactly on a constant row
    x = torch.ones(1, 16, 1, 5)
    with torch.no_grad():
        assert torch.allclose(d(x)[..., 1:-1], torch.ones(1, 16, 1, 8))


def test_pretrained_is_local_only(tmp_path):
    import joblib

    from semseg.models import SqueezeSegV2, squeezeseg_v2
    src = inspect.getsource(squeezeseg_v2)
    for needle in ("http", "torch.hub", "download", "urllib", "www."):
        assert needle not in src, needle
    assert not squeezeseg_v2.SQUEEZENET_FILE.exists(), "the repository ships no SqueezeNet pickle"
    with pytest.raises(FileNotFoundError, match="squeezenet_v1.1.pkl"):
        SqueezeSegV2(["xyz", "depth"], 4, pretrained_weights=True)
    with pytest.raises(FileNotFoundError):
        SqueezeSegV2(["xyz", "depth"], 4, pretrained_weights=str(tmp_path / "missing.pkl"))
    # a path loads that pickle into the eight encoder Fires (and nothing else)
    plain = SqueezeSegV2(["xyz", "depth"], 4, pretrained_weights=False)
    table = {}
    for name, module in plain.encoder.named_modules():
        if isinstance(module, squeezeseg_v2.Fire):
            for layer in ("squeeze1x1", "expand1x1", "expand3x3"):
                conv = getattr(module, layer)[0]
                key = f"{squeezeseg_v2._SQUEEZENET_NAMES[name]}/{layer}"
                table[key] = (R.hash_tensor(key + "/w", conv.weight.shape, -1, 1).numpy(),
                              R.hash_tensor(key + "/b", conv.bias.shape, -1, 1).numpy())
    assert len(table) == 24
    path = tmp_path / "sq.pkl"
    joblib.dump(table, path)
    model = SqueezeSegV2(["xyz", "depth"], 4, pretrained_weights=str(path))
    conv = model.encoder["fire_6_9"][3].expand3x3[0]
    assert np.array_equal(conv.weight.detach().numpy(), table["fire8/expand3x3"][0])
    assert np.array_equal(conv.bias.detach().numpy(), table["fire8/expand3x3"][1])


def test_wrapper_rejects_out_of_range():
    from gans.models.ops import native
    from gans.models.ops.native import fire

    assert fire.fire_supported(64, 16, 64, 64) and fire.fire_supported(384, 48, 192, 192, torch.float16)
    for bad in ((8, 16, 16, 16), (64, 24, 64, 64), (528, 16, 64, 64), (64, 80, 64, 64), (64, 16, 272, 64), (64, 16, 64, 40)):
        assert not fire.fire_supported(*bad), bad
    assert not fire.fire_supported(64, 16, 64, 64, torch.float64)
    assert native.fire_forward is fire.fire_forward

    def args(Cin=64, Cs=16, E1=64, E3=64, dtype=torch.float32):
        return dict(x=torch.zeros(1, Cin, 2, 4, dtype=dtype), w_s=torch.zeros(Cs, Cin, 1, 1), b_s=torch.zeros(Cs), bn_s=None,
                    w_d=None, b_d=None, w_1=torch.zeros(E1, Cs, 1, 1), b_1=torch.zeros(E1), bn_1=None,
                    w_3=torch.zeros(E3, Cs, 3, 3), b_3=torch.zeros(E3), bn_3=None)

    for kw in (dict(Cin=24), dict(Cs=80), dict(E1=8), dict(E3=320), dict(dtype=torch.float64)):
        with pytest.raises(ValueError):
            fire.fire_forward(**args(**kw))
    a = args()
    a["b_1"] = torch.zeros(3)
    with pytest.raises(ValueError):
        fire.fire_forward(**a)
    a = args()
    a["w_d"] = torch.zeros(16, 16, 1, 4)
    with pytest.raises(ValueError):
        fire.fire_forward(**a)
    a = args()
    a["bn_s"] = (torch.ones(16), torch.zeros(16), None, torch.ones(16), 1e-5)
    with pytest.raises(ValueError):
        fire.fire_forward(**a)
    with pytest.raises(ValueError):
        fire.fire_forward(**args(), skip=torch.zeros(1, 128, 2, 5))
    with pytest.raises(RuntimeError):      # in range, but CPU tensors: there is no CPU kernel
        fire.fire_forward(**args())


def test_cpu_forward_uses_the_composition_and_trains():
    """On the CPU (or with grad mode on) no native entry is reached; a tiny train-mode step gives finite gradients."""
    from gans.models.ops.native import fire
    from semseg.models import SqueezeSegV2
    model = _our_model(3)
    calls = []
    orig = fire.fire_forward
    fire.fire_forward = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        img = R.model_case_inputs(3)[0]
        with torch.no_grad():
            model(img)
        model.train()
        before = model.encoder["fire_2_3"][1].squeeze1x1[2].running_mean.clone()
        model(img).square().mean().backward()
    finally:
        fire.fire_forward = orig
    assert not calls
    assert isinstance(model, SqueezeSegV2)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert not torch.equal(before, model.encoder["fire_2_3"][1].squeeze1x1[2].running_mean)
