"""The CRF-RNN layer on the GPU (csrc/crf.hip, gans/models/ops/native/crf.py, semseg/models/crf_as_rnn.py) against
tests/golden/crf_rnn.npz, which the reference wrote on CPU in float64 and float32 (tests/golden/make_crf_golden.py).

Tolerance rule (the one of tests/test_gpu_inversion.py, scaled to the tensor): a result may differ from the reference's
float64 evaluation by 1e-6 * max|float64 reference of that tensor| plus twice the reference's OWN float32-vs-float64
maximum deviation for that tensor and case, which the fixture stores.  Shapes outside the fixture (the wide-window,
many-class, multi-tile case) use the same rule with tests/crf_ref.py, which test_crf_cpu.py pins to the reference at
1e-12, evaluated in both precisions on the CPU.

Measured on an MI355X: every tensor of every case lands at about the reference's own float32 deviation, far inside the
bound -- outputs 1.2e-7 .. 8.0e-7 (bounds 3.8e-6 .. 1.0e-5), g_unary 1.2e-7 .. 5.7e-7, parameter gradients up to
3.6e-5 on a magnitude of 663 (bound 8.7e-4).  The file runs in about a second."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from crf_ref import from_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
RESULTS = ("out", "g_unary", "g_weight_smoothness", "g_weight_appearance", "g_label_compatibility.weight")
PARAMS = ("weight_smoothness", "weight_appearance", "label_compatibility.weight")


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "crf_rnn.npz"))
    return {k: d[k] for k in d.files}


def t(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


def module_for(gold, name):
    from semseg.models.crf_as_rnn import CRFRNN
    B, C, H, W, kh, kw, iters = (int(v) for v in gold[f"{name}.shape"])
    crf = CRFRNN(C, kernel_size=(kh, kw), num_iters=iters)
    crf.load_state_dict({k[len(name) + 4:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(f"{name}.sd.")},
                        strict=True)
    return crf.to(DEV)


def run_native(crf, unary, xyz, mask, cot):
    """-> the five RESULTS tensors of one forward + backward."""
    u = unary.clone().requires_grad_(True)
    out = crf(u, xyz, mask)
    leaves = [u] + [dict(crf.named_parameters())[k] for k in PARAMS]
    grads = torch.autograd.grad((out * cot).sum(), leaves)
    return (out.detach(),) + grads


def tolerance(f64, f32):
    f64, f32 = torch.as_tensor(f64).double(), torch.as_tensor(f32).double()
    return 1e-6 * float(f64.abs().max()) + 2 * float((f32 - f64).abs().max())


def compare(label, got, f64, f32, bad):
    err = float((got.double().cpu() - torch.as_tensor(f64).double()).abs().max())
    tol = tolerance(f64, f32)
    print(f"{label}: max abs error {err:.2e}, tolerance {tol:.2e} "
          f"(reference's own float32 deviation {float((torch.as_tensor(f32).double() - torch.as_tensor(f64).double()).abs().max()):.2e})")
    if not err <= tol:
        bad.append((label, err, tol))


CASES = ["c0", "c1", "c2", "c3", "c4", "c5", "c6"]


@pytest.mark.parametrize("name", CASES)
def test_forward_and_gradients_match_the_reference(gold, name):
    crf = module_for(gold, name)
    got = run_native(crf, t(gold[f"{name}.unary"]), t(gold[f"{name}.xyz"]), t(gold[f"{name}.mask"]), t(gold[f"{name}.cot"]))
    bad = []
    for key, g in zip(RESULTS, got):
        assert tuple(g.shape) == tuple(gold[f"{name}.{key}.f64"].shape) and g.dtype == torch.float32
        compare(f"{name} {key}", g, gold[f"{name}.{key}.f64"], gold[f"{name}.{key}.f32"], bad)
    assert not bad, bad


@pytest.fixture(scope="module", params=["per_class", "shared"])
def wide(request):
    """C = 5 (the narrow tile of the many-class kernels), the largest window (5, 9), several tiles on both axes, a
    batch of 2, a float mask: inputs, the module's state and crf_ref's results in float64 and float32 (CPU).
    "shared": one theta_beta for every class, the layer's default, where the kernels evaluate a tap's bilateral weight
    once for all classes; "per_class": distinct ones, as in the fixture."""
    from semseg.models.crf_as_rnn import CRFRNN
    B, C, H, W = 2, 5, 11, 70
    g = torch.Generator().manual_seed(77)
    crf = CRFRNN(C, kernel_size=(5, 9), theta_gamma=[0.9 + 0.2 * c for c in range(C)], theta_alpha=1.1,
                 theta_beta=[0.015 * (1 + c) for c in range(C)] if request.param == "per_class" else 0.03, num_iters=2)
    with torch.no_grad():
        crf.weight_smoothness.mul_(1 + 0.5 * torch.rand(1, C, 1, 1, generator=g))
        crf.weight_appearance.mul_(0.3 * (1 + 0.5 * torch.rand(1, C, 1, 1, generator=g)))
        crf.label_compatibility.weight.add_(0.3 * torch.randn(C, C, 1, 1, generator=g))
    unary = 2 * torch.randn(B, C, H, W, generator=g)
    xyz = (10 + (0.02 * torch.randn(B, 3, 1, W, generator=g)).cumsum(3) + (0.02 * torch.randn(B, 3, H, 1, generator=g)).cumsum(2))
    mask = torch.rand(B, H, W, generator=g)
    cot = torch.randn(B, C, H, W, generator=g)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        sd = {k: v.detach().to(dtype) for k, v in crf.state_dict().items()}
        leaves = [unary.to(dtype).requires_grad_(True)] + [sd[k].requires_grad_(True) for k in PARAMS]
        out = from_state_dict(sd, leaves[0], xyz.to(dtype), mask.to(dtype), 2)
        ref[dtype] = (out.detach(),) + torch.autograd.grad((out * cot.to(dtype)).sum(), leaves)
    return crf, (unary, xyz, mask, cot), ref


def test_wide_window_many_classes_multi_tile(wide):
    crf, inputs, ref = wide
    got = run_native(crf.to(DEV), *(x.to(DEV) for x in inputs))
    bad = []
    for key, g, f64, f32 in zip(RESULTS, got, ref[torch.float64], ref[torch.float32]):
        compare(f"wide {key}", g, f64, f32, bad)
    assert not bad, bad


def test_zero_weights_return_the_unary_bit_for_bit(gold):
    for name in ("c0", "c5", "c6"):
        crf = module_for(gold, name)
        with torch.no_grad():
            crf.weight_smoothness.zero_()
            crf.weight_appearance.zero_()
        unary = t(gold[f"{name}.unary"])
        out = crf(unary, t(gold[f"{name}.xyz"]), t(gold[f"{name}.mask"]))
        assert out.data_ptr() != unary.data_ptr() and torch.equal(out, unary), name


def test_zero_iterations_return_the_unary(gold):
    crf = module_for(gold, "c0")
    crf.num_iters = 0
    unary = t(gold["c0.unary"])
    assert crf(unary, t(gold["c0.xyz"]), t(gold["c0.mask"])) is unary


def test_all_zero_mask_is_smoothness_only(gold):
    bad = []
    for name in ("c0", "c5"):
        crf = module_for(gold, name)
        unary, xyz = t(gold[f"{name}.unary"]), t(gold[f"{name}.xyz"])
        got = crf(unary, xyz, torch.zeros_like(t(gold[f"{name}.mask"])))
        sd = {k: v.detach().double().cpu() for k, v in crf.state_dict().items()}
        sd["weight_appearance"] = torch.zeros_like(sd["weight_appearance"])
        want = from_state_dict(sd, unary.double().cpu(), xyz.double().cpu(),
                               torch.from_numpy(gold[f"{name}.mask"]).double(), crf.num_iters)
        err = float((got.detach().double().cpu() - want).abs().max())
        dev = float(np.abs(gold[f"{name}.out.f32"].astype(np.float64) - gold[f"{name}.out.f64"]).max())
        tol = 1e-6 * float(want.abs().max()) + 2 * dev
        print(f"{name} zero mask: max abs error {err:.2e}, tolerance {tol:.2e}")
        if not err <= tol:
            bad.append((name, err, tol))
    assert not bad, bad


def test_bit_identical_run_to_run(gold):
    name = "c5"
    crf = module_for(gold, name)
    args = [t(gold[f"{name}.{k}"]) for k in ("unary", "xyz", "mask", "cot")]
    a, b = run_native(crf, *args), run_native(crf, *args)
    for key, x, y in zip(RESULTS, a, b):
        assert torch.equal(x, y), key


def test_mask_rank_does_not_matter(gold):
    name = "c1"
    crf = module_for(gold, name)
    unary, xyz, mask, cot = (t(gold[f"{name}.{k}"]) for k in ("unary", "xyz", "mask", "cot"))
    a, b = run_native(crf, unary, xyz, mask, cot), run_native(crf, unary, xyz, mask[:, None], cot)
    for key, x, y in zip(RESULTS, a, b):
        assert torch.equal(x, y), key


def test_double_backward_raises(gold):
    crf = module_for(gold, "c3")
    u = t(gold["c3.unary"]).requires_grad_(True)
    out = crf(u, t(gold["c3.xyz"]), t(gold["c3.mask"]))
    (g,) = torch.autograd.grad(out.sum(), u, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_unsupported_arguments_are_rejected(gold):
    import ctypes
    import dgv2_native as N
    from gans.models.ops import native
    from semseg.models.crf_as_rnn import CRFRNN
    crf = module_for(gold, "c0")
    unary, xyz, mask = t(gold["c0.unary"]), t(gold["c0.xyz"]), t(gold["c0.mask"])
    with pytest.raises(ValueError):
        crf(unary, xyz[:, :, :, :-1].contiguous(), mask)
    with pytest.raises(ValueError):
        crf(unary, xyz[:, :2].contiguous(), mask)
    with pytest.raises(ValueError):
        CRFRNN(9)
    with pytest.raises(ValueError):
        CRFRNN(3, kernel_size=(7, 5))
    with pytest.raises(ValueError):
        CRFRNN(3, kernel_size=(3, 4))
    big = torch.zeros(9, 9, 3, 5, device=DEV)
    with pytest.raises(ValueError):
        native.crf_rnn(torch.zeros(1, 9, 4, 6, device=DEV), xyz[:1, :, :4, :6].contiguous(), mask[:1, :4, :6].contiguous(),
                       big, big, torch.ones(9, device=DEV), torch.ones(9, device=DEV), torch.ones(9, device=DEV),
                       torch.ones(9, 9, device=DEV), 1)

    # the C entry points themselves: DGV2_EINVAL, nothing launched
    B, C, H, W = unary.shape
    out, qs = torch.empty_like(unary), torch.empty((2,) + tuple(unary.shape), device=DEV)
    sd = crf.state_dict()
    tail = [N.ptr(sd[k]) for k in ("kernel_gamma", "kernel_alpha", "theta_beta", "weight_smoothness", "weight_appearance",
                                   "label_compatibility.weight")]

    def fwd(o=N.ptr(out), q=N.ptr(qs), dims=(B, C, H, W, 3, 5, 3)):
        return N.lib.dgv2_crf_rnn_forward(o, q, N.ptr(unary), N.ptr(xyz), N.ptr(mask), *tail, *dims, N.stream())
    assert fwd() == 0
    assert fwd(o=None) == -1 and fwd(q=None) == -1
    for dims in ((B, 9, H, W, 3, 5, 3), (B, 0, H, W, 3, 5, 3), (B, C, H, W, 7, 5, 3), (B, C, H, W, 3, 11, 3),
                 (B, C, H, W, 2, 5, 3), (B, C, H, W, 3, 4, 3), (0, C, H, W, 3, 5, 3), (B, C, 0, W, 3, 5, 3),
                 (B, C, H, 0, 3, 5, 3), (B, C, H, W, 3, 5, 0)):
        assert fwd(dims=dims) == -1, dims
    need = ctypes.c_int64(0)
    assert N.lib.dgv2_crf_rnn_backward_scratch(ctypes.addressof(need), B, C, H, W, 3) == 0 and need.value > 0
    assert N.lib.dgv2_crf_rnn_backward_scratch(ctypes.addressof(need), B, 9, H, W, 3) == -1
    scratch = torch.empty(need.value, device=DEV)
    grads = [torch.empty_like(x) for x in (unary, sd["weight_smoothness"], sd["weight_appearance"],
                                           sd["label_compatibility.weight"])]

    def bwd(elems, dims=(B, C, H, W, 3, 5, 3), s=N.ptr(scratch)):
        return N.lib.dgv2_crf_rnn_backward(*[N.ptr(g) for g in grads], s, elems, N.ptr(out), N.ptr(qs), N.ptr(unary),
                                           N.ptr(xyz), N.ptr(mask), *tail, *dims, N.stream())
    assert bwd(need.value) == 0
    assert bwd(need.value - 1) == -1 and bwd(need.value, s=None) == -1
    assert bwd(need.value, dims=(B, C, H, W, 5, 11, 3)) == -1 and bwd(need.value, dims=(B, 9, H, W, 3, 5, 3)) == -1
    torch.cuda.synchronize()
