"""GPU checks of the one-launch context-aggregation module (csrc/cam.hip, native.cam).

Yardsticks, the project's own.  float32: max|gpu - ref64| <= 4 E_ref + 2^-22 max|ref64|,
E_ref = max|ref32 - ref64| from the fixture the reference's module wrote (tests/golden/cam.npz); ref64 over the whole
output comes from cam_ref.cam_ref, which the fixture script pinned to the reference's float64 output and
test_cam_cpu pins again at the stored sample.  16-bit: the module's composition of library ops at that dtype in the
same test, max|native16 - ref64| <= 2 E_comp.  Both are also taken over the border pixels alone (those whose 7x7
window leaves the image: where a wrong padding shows), with E_ref / E_comp over those pixels.  Measured ratios:
DESIGN.md section 35.3.
"""
import copy
import os

import numpy as np
import pytest
import torch

import cam_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fx():
    d = np.load(os.path.join(GOLDEN, "cam.npz"))
    return {k: d[k] for k in d.files}


def _bound(e_ref, top):
    return 4.0 * e_ref + 2.0 ** -22 * top


_CASES = {}


def _case(i):
    """(module on the GPU, state dict, x, ref64 over the whole output), computed once per case and left unchanged."""
    if i not in _CASES:
        from semseg.models.squeezeseg_v2 import CAM
        B, C, H, W, kind = R.CAM_CASES[i]
        cam = CAM(C, R.REDUCTION)
        sd = R.cam_case_state_dict(i, cam.state_dict())
        cam.load_state_dict(sd, strict=True)
        x = R.cam_case_input(i)
        _CASES[i] = (cam.eval().to(DEV), sd, x, R.cam_ref(sd, x))
    return _CASES[i]


def _native(cam, x):
    from semseg.models import common
    with torch.no_grad():
        assert common.cam_uses_native(cam, x) or not common.CAM_NATIVE
        return common.cam_native(cam, x)


# ---- parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.CAM_CASES)))
def test_cam_float32_parity(fx, i):
    name = R.cam_case_name(i)
    B, C, H, W, kind = R.CAM_CASES[i]
    cam, sd, x, ref64 = _case(i)
    y = _native(cam, x.to(DEV))
    assert y.shape == ref64.shape and y.dtype == torch.float32 and y.is_contiguous()
    diff = (y.cpu().double() - ref64).abs()
    e_ref, top = float(fx[name + "/e_ref"]), float(fx[name + "/max64"])
    err = float(diff.max())
    print(f"PARITY f32 {name}: err {err:.3e}  E_ref {e_ref:.3e}  ratio {err / e_ref:.2f}  bound {_bound(e_ref, top):.3e}")
    border = R.border_mask(H, W)
    e_b, top_b = float(fx[name + "/e_ref_border"]), float(fx[name + "/max64_border"])
    err_b = float(diff[..., border].max())
    print(f"BORDER f32 {name}: err {err_b:.3e}  E_ref {e_b:.3e}  ratio {err_b / e_b:.2f}  bound {_bound(e_b, top_b):.3e}")
    assert err <= _bound(e_ref, top)
    assert err_b <= _bound(e_b, top_b)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("i", range(len(R.CAM_CASES)))
def test_cam_16bit_parity(i, dtype):
    from semseg.models import common
    name = R.cam_case_name(i)
    B, C, H, W, kind = R.CAM_CASES[i]
    cam, sd, x, ref64 = _case(i)
    x16 = x.to(DEV).to(dtype)
    with torch.no_grad():
        comp = common.cam_composition(copy.deepcopy(cam).to(dtype), x16).float().cpu().double()
    y = _native(cam, x16)
    assert y.dtype == dtype and y.shape == ref64.shape
    d_nat, d_comp = (y.float().cpu().double() - ref64).abs(), (comp - ref64).abs()
    border = R.border_mask(H, W)
    err, e_comp = float(d_nat.max()), float(d_comp.max())
    err_b, e_comp_b = float(d_nat[..., border].max()), float(d_comp[..., border].max())
    print(f"PARITY {str(dtype)[6:]} {name}: native err {err:.3e}  E_comp {e_comp:.3e}  ratio {err / e_comp:.2f}  "
          f"border {err_b:.3e} / {e_comp_b:.3e}  ratio {err_b / e_comp_b:.2f}")
    assert err <= 2.0 * e_comp
    assert err_b <= 2.0 * e_comp_b


# ---- kernel behaviour -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_a_batch_equals_its_samples_bit_for_bit(dtype):
    cam, sd, x, ref64 = _case(1)                       # 2 x 64 x 3 x 33
    xg = x.to(DEV).to(dtype)
    both = _native(cam, xg)
    assert torch.equal(both, _native(cam, xg))
    for b in range(xg.shape[0]):
        assert torch.equal(both[b:b + 1], _native(cam, xg[b:b + 1]))
    stacked = torch.cat([xg[1:], xg[:1], xg[1:]])      # another batch size and order: another grid
    again = _native(cam, stacked)
    assert torch.equal(again[0], both[1]) and torch.equal(again[1], both[0]) and torch.equal(again[2], both[1])


def test_layout_free_and_canaries_stay_intact():
    import dgv2_native as N
    cam, sd, x, ref64 = _case(2)                       # 1 x 128 x 9 x 70: ragged tiles on both axes
    xg = x.to(DEV)
    y0 = _native(cam, xg)
    wide = torch.zeros(xg.shape[0], xg.shape[1], xg.shape[2], xg.shape[3] + 3, device=DEV)
    wide[..., 2:-1] = xg
    assert not wide[..., 2:-1].is_contiguous() and torch.equal(y0, _native(cam, wide[..., 2:-1]))
    assert torch.equal(y0, _native(cam, xg.contiguous(memory_format=torch.channels_last)))
    pad, canary = 4096, 12345.0
    buf = torch.full((y0.numel() + 2 * pad,), canary, device=DEV)
    y = buf[pad:pad + y0.numel()].view_as(y0)
    sq, ex = cam.attn[1], cam.attn[3]
    B, C, H, W = xg.shape
    N.call("dgv2_cam_fwd", N.ptr(y), N.ptr(xg), N.ptr(sq.weight), N.ptr(sq.bias), N.ptr(ex.weight), N.ptr(ex.bias),
           B, C, sq.out_channels, H, W, N.F32, N.stream())
    torch.cuda.synchronize()
    assert torch.equal(y, y0)
    assert bool((buf[:pad] == canary).all()) and bool((buf[pad + y0.numel():] == canary).all())


def test_a_call_reads_the_current_parameters():
    from semseg.models.squeezeseg_v2 import CAM
    cam = CAM(64, R.REDUCTION)
    cam.load_state_dict(R.hash_fill_state_dict(cam.state_dict(), salt="current/"), strict=True)
    cam = cam.eval().to(DEV)
    x = R.hash_tensor("current/x", (1, 64, 5, 21), -1.5, 1.5)
    first = _native(cam, x.to(DEV))
    with torch.no_grad():
        cam.attn[1].weight.mul_(-0.5)
        cam.attn[1].bias.add_(0.25)
        cam.attn[3].weight.add_(0.05)
        cam.attn[3].bias.sub_(0.5)
    second = _native(cam, x.to(DEV)).cpu().double()
    new_sd = {k: v.detach().cpu() for k, v in cam.state_dict().items()}
    ref64 = R.cam_ref(new_sd, x)
    with torch.no_grad():
        ref32 = copy.deepcopy(cam).cpu()(x.clone()).double()
    e_ref, top = float((ref32 - ref64).abs().max()), float(ref64.abs().max())
    err = float((second - ref64).abs().max())
    print(f"CURRENT: err {err:.3e}  E_ref {e_ref:.3e}  ratio {err / e_ref:.2f}")
    assert err <= _bound(e_ref, top)
    assert float((first.cpu().double() - ref64).abs().max()) > 100 * _bound(e_ref, top)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_one_call_is_one_kernel_and_no_aten_kernel(dtype, monkeypatch):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from semseg.models import common
    monkeypatch.setattr(common, "CAM_NATIVE", True)
    cam, sd, x, ref64 = _case(1)
    xg = x.to(DEV).to(dtype)
    with torch.inference_mode():
        want = cam(xg)                                 # warm: code object loaded outside the profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            got = cam(xg)                              # the module's own forward: the routing included
            torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    assert len(names) == 1 and "cam_fwd_kernel" in names[0], names
    assert torch.equal(got, want)
    monkeypatch.setattr(common, "CAM_NATIVE", False)   # the switch is read at every call
    with torch.inference_mode(), profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        cam(xg if dtype == torch.float32 else xg.float())
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    assert len(names) >= 5 and not any("cam_fwd_kernel" in n for n in names), names
