"""GPU checks of the one-launch Fire module (csrc/fire.hip, native.fire) and of the SqueezeSeg trunks routed through it.

Yardsticks.  float32: the reference's own float32 error, max|gpu - ref64| <= 4 E_ref + 2^-22 max|ref64| (DESIGN.md
section 29.4), E_ref = max|ref32 - ref64| from the fixture the reference's modules wrote; ref64 over the whole output
comes from squeezeseg_ref.fire_ref, which the fixture script pinned to the reference's float64 output over the whole
output and test_squeezeseg_cpu pins again at the stored sample.  16-bit: the module's composition of library ops at
that dtype, max|native16 - ref64| <= 2 E_comp.  Measured ratios: DESIGN.md section 31.3.
"""
import os

import numpy as np
import pytest
import torch

import squeezeseg_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1


@pytest.fixture(scope="module")
def fx():
    d = np.load(os.path.join(GOLDEN, "squeezeseg.npz"))
    return {k: d[k] for k in d.files}


def _bound(e_ref, top):
    return 4.0 * e_ref + 2.0 ** -22 * top


def _make_fire(ver, Cin, Cs, E, up, salt):
    from semseg.models import squeezeseg_v1, squeezeseg_v2
    fire = squeezeseg_v1.Fire(Cin, Cs, E, E, up=up) if ver == 1 else squeezeseg_v2.Fire(Cin, Cs, E, E, 0.001, up=up)
    sd = R.hash_fill_state_dict(fire.state_dict(), salt=salt)
    fire.load_state_dict(sd, strict=True)
    return fire.eval(), sd


_CASES = {}


def _case(i):
    """(module on the GPU, state dict, x, ref64 over the whole output), computed once per case and left unchanged."""
    if i not in _CASES:
        ver, B, Cin, Cs, E, H, W, up = R.FIRE_CASES[i]
        fire, sd = _make_fire(ver, Cin, Cs, E, up, R.fire_case_name(i) + "/")
        x = R.fire_case_input(i)
        _CASES[i] = (fire.to(DEV), sd, x, R.fire_ref(sd, x))
    return _CASES[i]


def _native(fire, x, skip=None):
    from semseg.models import common
    with torch.no_grad():
        assert common.fire_uses_native(fire, x)
        return common.fire_native(fire, x, skip)


def _model(i):
    from semseg.models import SqueezeSegV1, SqueezeSegV2
    ver, B, H, W, crf = R.MODEL_CASES[i]
    if ver == 1:
        model = SqueezeSegV1(R.MODEL_INPUTS, R.MODEL_CLASSES, use_crf=crf)
    else:
        model = SqueezeSegV2(R.MODEL_INPUTS, R.MODEL_CLASSES, use_crf=crf, pretrained_weights=False)
    model.load_state_dict(R.hash_fill_state_dict(model.state_dict(), salt=f"v{ver}/"), strict=True)
    return model.eval().to(DEV)


# ---- parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.FIRE_CASES)))
def test_fire_float32_parity(fx, i):
    name = R.fire_case_name(i)
    fire, sd, x, ref64 = _case(i)
    y = _native(fire, x.to(DEV)).cpu().double()
    e_ref, top = float(fx[name + "/e_ref"]), float(fx[name + "/max64"])
    err = float((y - ref64).abs().max())
    print(f"PARITY f32 {name}: err {err:.3e}  E_ref {e_ref:.3e}  ratio {err / e_ref:.2f}  bound {_bound(e_ref, top):.3e}")
    assert y.shape == ref64.shape
    assert err <= _bound(e_ref, top)


@pytest.mark.parametrize("i", range(len(R.MODEL_CASES)))
def test_model_float32_parity(fx, i):
    name = R.model_case_name(i)
    model = _model(i)
    img, xyz, mask = (torch.from_numpy(fx[f"{name}/{k}"]).to(DEV) for k in ("img", "xyz", "mask"))
    with torch.no_grad():
        logit = model(img, xyz, mask).cpu().double()
    ref64, ref32 = torch.from_numpy(fx[name + "/logit64"]), torch.from_numpy(fx[name + "/logit32"])
    e_ref, top = float((ref32.double() - ref64).abs().max()), float(ref64.abs().max())
    err = float((logit - ref64).abs().max())
    print(f"PARITY f32 {name}: err {err:.3e}  E_ref {e_ref:.3e}  ratio {err / e_ref:.2f}  bound {_bound(e_ref, top):.3e}")
    assert logit.shape == ref64.shape
    assert err <= _bound(e_ref, top)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("i", range(len(R.FIRE_CASES)))
def test_fire_16bit_parity(i, dtype):
    import copy
    name = R.fire_case_name(i)
    fire, sd, x, ref64 = _case(i)
    x16 = x.to(DEV).to(dtype)
    with torch.no_grad():
        from semseg.models import common
        comp = common.fire_composition(copy.deepcopy(fire).to(dtype), x16).float().cpu().double()
    y = _native(fire, x16)
    assert y.dtype == dtype
    e_comp = float((comp - ref64).abs().max())
    err = float((y.float().cpu().double() - ref64).abs().max())
    print(f"PARITY {str(dtype)[6:]} {name}: native err {err:.3e}  E_comp {e_comp:.3e}  ratio {err / e_comp:.2f}")
    assert err <= 2.0 * e_comp


@pytest.mark.parametrize("up", [False, True], ids=["plain", "up"])
def test_padding_is_of_the_squeezed_tensor(up):
    """Large border pixels and a squeeze bias that makes N_s(relu(b_s)) of order 1: a kernel that pads x instead of u,
    or squeezes clamped / wrapped pixels, is wrong at the border by far more than the float32 bound there."""
    import copy
    fire, sd = _make_fire(2, 64, 16, 32, up, f"padding{int(up)}/")
    with torch.no_grad():
        fire.squeeze1x1[0].bias.fill_(2.0)
    sd = {k: v.clone() for k, v in fire.state_dict().items()}
    bn = fire.squeeze1x1[2]
    ghost = (2.0 - bn.running_mean) * bn.weight / torch.sqrt(bn.running_var + bn.eps) + bn.bias    # N_s(relu(b_s))
    assert float(ghost.detach().abs().min()) > 0.3
    B, H, W = 1, 5, 37
    x = R.hash_tensor("padding/x", (B, 64, H, W), -1.0, 1.0)
    edge = torch.zeros(H, W, dtype=torch.bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    x = torch.where(edge, x * 50.0, x)
    ref64 = R.fire_ref(sd, x)
    with torch.no_grad():
        ref32 = copy.deepcopy(fire)(x.clone()).double()      # the library composition on the CPU in float32
    y = _native(fire.to(DEV), x.to(DEV)).cpu().double()
    Wo = ref64.shape[3]
    border = torch.zeros(H, Wo, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    e_ref = float((ref32 - ref64)[..., border].abs().max())
    top = float(ref64[..., border].abs().max())
    err = float((y - ref64)[..., border].abs().max())
    print(f"PADDING up={up}: border err {err:.3e}  E_ref {e_ref:.3e}  ratio {err / e_ref:.2f}  max {top:.1f}")
    assert err <= _bound(e_ref, top)
    assert float((y - ref64).abs().max()) <= _bound(float((ref32 - ref64).abs().max()), float(ref64.abs().max()))


# ---- exact properties -----------------------------------------------------------------------------------------------
RAGGED = [2, 3]   # 2 x 64 x 3 x 33 and 1 x 128 x 9 x 70 with up-sampling


@pytest.mark.parametrize("i", RAGGED)
def test_runs_are_bit_identical_and_layout_free(i):
    fire, sd, x, ref64 = _case(i)
    xg = x.to(DEV)
    y0 = _native(fire, xg)
    assert torch.equal(y0, _native(fire, xg))
    buf = torch.zeros(xg.numel() + 1, device=DEV)
    buf[1:] = xg.flatten()
    assert torch.equal(y0, _native(fire, buf[1:].view_as(xg)))            # one element into a buffer: 4-byte aligned only
    wide = torch.zeros(xg.shape[0], xg.shape[1], xg.shape[2], xg.shape[3] + 3, device=DEV)
    wide[..., 2:-1] = xg
    sliced = wide[..., 2:-1]
    assert not sliced.is_contiguous()
    assert torch.equal(y0, _native(fire, sliced))
    assert torch.equal(y0, _native(fire, xg, skip=torch.zeros_like(y0)))   # skip = None is skip = zeros
    skip = R.hash_tensor("skip", tuple(y0.shape), -1.0, 1.0).to(DEV)
    assert torch.equal(y0 + skip, _native(fire, xg, skip=skip))


def _prepared(fire, x, skip=None):
    """Operands as native.fire.fire_forward prepares them, for calls of the raw entry."""
    from gans.models.ops.native import fire as F
    from semseg.models import common
    sq, ns = common._conv_and_norm(fire.squeeze1x1)
    e1, n1 = common._conv_and_norm(fire.expand1x1)
    e3, n3 = common._conv_and_norm(fire.expand3x3)
    up = fire.upsample[0] if fire.upsample is not None else None
    P = lambda t: None if t is None else t.detach().contiguous()   # noqa: E731
    return dict(x=x.contiguous(), skip=skip, w_s=P(sq.weight), b_s=P(sq.bias), ns=F._norm("s", ns, sq.out_channels),
                w_d=None if up is None else P(up.weight), b_d=None if up is None else P(up.bias), w_1=P(e1.weight), b_1=P(e1.bias),
                n1=F._norm("1", n1, e1.out_channels), w_3=P(e3.weight), b_3=P(e3.bias), n3=F._norm("3", n3, e3.out_channels))


@pytest.mark.parametrize("i", RAGGED)
def test_canaries_stay_intact(i):
    from gans.models.ops.native import fire as F
    fire, sd, x, ref64 = _case(i)
    xg = x.to(DEV)
    y0 = _native(fire, xg)
    pad, canary = 4096, 12345.0
    buf = torch.full((y0.numel() + 2 * pad,), canary, device=DEV)
    y = buf[pad:pad + y0.numel()].view_as(y0)
    with torch.no_grad():
        F.fire_forward_into(y, **_prepared(fire, xg))
    torch.cuda.synchronize()
    assert torch.equal(y, y0)
    assert bool((buf[:pad] == canary).all()) and bool((buf[pad + y0.numel():] == canary).all())


def test_bad_arguments_return_einval_and_touch_nothing():
    import dgv2_native as N
    fire, sd, x, ref64 = _case(2)
    xg = x.to(DEV)
    y0 = _native(fire, xg)
    p = _prepared(fire, xg)
    B, Cin, H, W = xg.shape
    y = torch.full_like(y0, 7.0)

    def call(**over):
        a = dict(y=N.ptr(y), x=N.ptr(p["x"]), skip=None, w_s=N.ptr(p["w_s"]), b_s=N.ptr(p["b_s"]),
                 ns=[N.ptr(t) for t in p["ns"][:4]], w_d=None, b_d=None, w_1=N.ptr(p["w_1"]), b_1=N.ptr(p["b_1"]),
                 n1=[N.ptr(t) for t in p["n1"][:4]], w_3=N.ptr(p["w_3"]), b_3=N.ptr(p["b_3"]),
                 n3=[N.ptr(t) for t in p["n3"][:4]], eps=(1e-5, 1e-5, 1e-5), B=B, Cin=Cin, Cs=16, E1=64, E3=64, H=H, W=W,
                 up=0, dtype=N.F32)
        a.update(over)
        return N.lib.dgv2_fire_fwd(a["y"], a["x"], a["skip"], a["w_s"], a["b_s"], *a["ns"], a["w_d"], a["b_d"], a["w_1"],
                                   a["b_1"], *a["n1"], a["w_3"], a["b_3"], *a["n3"], *a["eps"], a["B"], a["Cin"], a["Cs"],
                                   a["E1"], a["E3"], a["H"], a["W"], a["up"], a["dtype"], N.stream())

    ns = [N.ptr(t) for t in p["ns"][:4]]
    bad = [dict(y=None), dict(x=None), dict(w_s=None), dict(b_3=None), dict(B=0), dict(H=0), dict(W=-1), dict(Cin=24),
           dict(Cin=528), dict(Cs=8), dict(Cs=80), dict(E1=0), dict(E3=272), dict(E1=40), dict(up=1), dict(up=2),
           dict(w_d=N.ptr(p["w_s"])), dict(dtype=2), dict(dtype=7), dict(ns=[ns[0], None, ns[2], ns[3]]),
           dict(eps=(-1.0, 1e-5, 1e-5)), dict(eps=(1e-5, float("nan"), 1e-5)),
           dict(w_s=N.ptr(p["w_s"]) + 4), dict(w_3=N.ptr(p["w_3"]) + 8)]      # weights are read with 16-byte loads
    for over in bad:
        assert call(**over) == EINVAL, over
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert call() == 0
    assert torch.equal(y, y0)


@pytest.mark.parametrize("i", RAGGED)
def test_fire_replays_from_a_graph(i):
    fire, sd, x, ref64 = _case(i)
    xg = x.to(DEV)
    skip = R.hash_tensor("skip", tuple(ref64.shape), -1.0, 1.0).to(DEV)
    eager = _native(fire, xg, skip)
    x_in = torch.zeros_like(xg)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _native(fire, x_in, skip)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _native(fire, x_in, skip)
    x_in.copy_(xg)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_a_call_reads_the_current_parameters():
    import copy
    fire, sd = _make_fire(2, 64, 16, 32, True, "current/")
    fire = fire.to(DEV)
    x = R.hash_tensor("current/x", (1, 64, 3, 21), -1.5, 1.5)
    first = _native(fire, x.to(DEV))
    with torch.no_grad():
        fire.squeeze1x1[2].running_mean.add_(0.25)
        fire.expand3x3[2].running_var.mul_(1.5)
        fire.expand3x3[0].weight.mul_(-0.5)
        fire.upsample[0].weight.add_(0.01)
    second = _native(fire, x.to(DEV)).cpu().double()
    new_sd = {k: v.detach().cpu() for k, v in fire.state_dict().items()}
    ref64 = R.fire_ref(new_sd, x)
    with torch.no_grad():
        ref32 = copy.deepcopy(fire).cpu()(x.clone()).double()
    e_ref, top = float((ref32 - ref64).abs().max()), float(ref64.abs().max())
    err = float((second - ref64).abs().max())
    print(f"CURRENT: err {err:.3e}  E_ref {e_ref:.3e}  ratio {err / e_ref:.2f}")
    assert err <= _bound(e_ref, top)
    assert float((first.cpu().double() - ref64).abs().max()) > 100 * _bound(e_ref, top)


# ---- routing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [1, 3])
def test_routing(i, monkeypatch):
    from gans.models.ops.native import fire as F
    from semseg.models import common
    model = _model(i)
    img = R.model_case_inputs(i)[0].to(DEV)
    calls = []
    orig = F.fire_forward
    monkeypatch.setattr(F, "fire_forward", lambda *a, **k: calls.append(1) or orig(*a, **k))
    with torch.no_grad():
        native = model(img)
    assert len(calls) == 12
    with torch.inference_mode():
        model(img)
    assert len(calls) == 24
    del calls[:]
    model(img)                                    # grad mode on
    monkeypatch.setattr(common, "FIRE_NATIVE", False)
    with torch.no_grad():
        composed = model(img)                     # the switch
    monkeypatch.setattr(common, "FIRE_NATIVE", True)
    model.train()
    with torch.no_grad():
        model(img)                                # training mode
    assert not calls
    assert float((native - composed).abs().max()) <= 1e-3 * float(composed.abs().max())


def test_train_mode_step_on_the_gpu():
    model = _model(3).train()
    img = R.model_case_inputs(3)[0].to(DEV)
    bn = model.encoder["fire_6_9"][4].expand3x3[2]
    before = bn.running_mean.clone()
    model(img).square().mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert not torch.equal(before, bn.running_mean) and int(bn.num_batches_tracked) == 1
