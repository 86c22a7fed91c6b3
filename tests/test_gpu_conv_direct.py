"""The direct conv engine (csrc/conv_direct.hip) behind its geometry entries dgv2_conv_direct_fwd / _fwd_fp8 / _dgrad,
through the Python call sites (native._conv_fwd_raw, _conv_dgrad_raw, _conv_dgrad_direct, _conv_fwd_fp8) at the smallest
shapes that reach each of its routes (tests/conv_direct_cases.py: strip kernel, conv8, image pairs, the unrolled and
the generic pipelined instances, the synchronous kernel, the channel-range split, the four-class stride-2 data gradient
and both unfused sequences).

(a) integer-valued operands (|v| <= 2, residual and bias |v| <= 3): every product and sum is exact in bf16 / fp32, so
    the result EQUALS the float64 ring conv (ops.Conv2d, gans/models/ops/common.py:187-210) and its autograd;
(b) random operands: the output bytes hash to what the tap-list engine of ABI 58 produced for the same call
    (tests/golden/conv_direct_digests.json, recorded by tests/golden/make_conv_direct_golden.py)."""
import json
import os

import pytest
import torch

import conv_direct_cases as cc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from gans.models.ops import native
    return native


@pytest.fixture(scope="module")
def digests():
    with open(os.path.join(GOLDEN, "conv_direct_digests.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_exact_on_integers_against_the_float64_ring_conv(nat, case):
    got, want = cc.run(nat, case, True)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert float(w.abs().max()) < 256
        assert torch.equal(g.double().cpu(), w)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_same_bits_as_the_tap_list_engine_on_random_operands(nat, digests, case):
    got, _ = cc.run(nat, case, False)
    for i, g in enumerate(got):
        assert bool(torch.isfinite(g.float()).all())
        assert cc.digest(g) == digests[f"{case[0]}/{i}"], f"{case[0]}/{i}"


def test_residual_of_an_unfused_data_gradient_is_refused_before_any_launch(nat):
    """dgv2_conv_direct_dgrad folds `resid` only into the fused stride-1 3x3 form: where that form is refused (W = 8) or does
    not exist (stride 2, 1x1) it answers DGV2_ENOTSUP and leaves gx untouched; the caller adds the residual itself."""
    import dgv2_native as N
    for (B, H, W, C, O, k, s) in [(2, 8, 8, 32, 32, 3, 1), (2, 16, 64, 32, 64, 3, 2), (2, 8, 32, 32, 32, 1, 1)]:
        Ho, Wo = H // s, W // s
        gy = torch.ones(B, Ho, Wo, O, device=cc.DEV, dtype=torch.bfloat16)
        wt = torch.ones(C, k * k, O, device=cc.DEV, dtype=torch.bfloat16)
        resid = torch.ones(B, H, W, C, device=cc.DEV, dtype=torch.bfloat16)
        gx = torch.full((B, H, W, C), 7.0, device=cc.DEV, dtype=torch.bfloat16)
        assert N.try_call("dgv2_conv_direct_dgrad", N.ptr(gx), N.ptr(gy), N.ptr(wt), B, H, W, C, O, k, s, N.ptr(resid), N.BF16,
                          N.stream()) is False
        assert bool((gx == 7.0).all())
        assert N.try_call("dgv2_conv_direct_dgrad", N.ptr(gx), N.ptr(gy), N.ptr(wt), B, H, W, C, O, k, s, None, N.BF16,
                          N.stream()) is True
