"""Host-side decisions of dgv2_conv_direct_fwd / _fwd_fp8 / _dgrad (conv_direct.hip): the argument checks and the
refusals that need no geometry are taken before anything touches the device, so they can be held without one.  The
pointers are never dereferenced on these paths."""
import pytest

import dgv2_native as N

P16, ODD = 1 << 20, (1 << 20) + 8   # a 16-byte aligned and a misaligned non-null address
EINVAL = -1


def fwd(y=P16, x=P16, w=P16, B=2, H=8, W=32, Cin=32, O=32, k=3, stride=1, resid=None, act=0, dt=N.BF16):
    return N.lib.dgv2_conv_direct_fwd(y, x, w, B, H, W, Cin, O, k, stride, None, resid, act, 0.2, 1.0, dt, None)


def fwd_fp8(y=P16, x=P16, w=P16, acc_scale=P16, B=2, H=8, W=32, Cin=64, O=64, k=3, stride=1, resid=None, act=0):
    return N.lib.dgv2_conv_direct_fwd_fp8(y, x, w, acc_scale, B, H, W, Cin, O, k, stride, None, resid, act, 0.2, 1.0, None)


def dgrad(gx=P16, gy=P16, wt=P16, B=2, H=8, W=32, C=32, O=32, k=3, stride=1, resid=None, dt=N.BF16):
    return N.lib.dgv2_conv_direct_dgrad(gx, gy, wt, B, H, W, C, O, k, stride, resid, dt, None)


@pytest.mark.parametrize("entry,out,a,w", [(fwd, "y", "x", "w"), (fwd_fp8, "y", "x", "w"), (dgrad, "gx", "gy", "wt")])
def test_invalid_arguments(entry, out, a, w):
    for operand in (out, a, w):
        assert entry(**{operand: None}) == EINVAL
    assert entry(**{a: ODD}) == EINVAL and entry(**{w: ODD}) == EINVAL
    assert entry(k=2) == EINVAL
    assert entry(stride=3) == EINVAL and entry(stride=0) == EINVAL
    assert entry(B=0) == EINVAL and entry(H=0) == EINVAL and entry(W=0) == EINVAL and entry(O=0) == EINVAL


def test_contraction_length_is_whole_k_chunks():
    """One 64-byte K-chunk: 32 bf16 / 16 fp32 values of the contraction -- Cin forward, O in the data gradient."""
    assert fwd(Cin=24) == EINVAL and fwd(Cin=24, dt=N.F32) == EINVAL
    assert dgrad(O=24) == EINVAL and dgrad(O=24, dt=N.F32) == EINVAL
    assert fwd(dt=2) == EINVAL and dgrad(dt=2) == EINVAL          # e4m3 has its own entry
    assert fwd(act=1) == EINVAL and fwd_fp8(act=1) == EINVAL
    assert fwd_fp8(acc_scale=None) == EINVAL


def test_data_gradient_geometry_the_callers_exclude():
    assert dgrad(H=7, stride=2) == EINVAL and dgrad(W=31, stride=2) == EINVAL     # stride 2 halves H and W
    assert dgrad(k=1, stride=2) == EINVAL


def test_e4m3_forward_asks_for_the_bf16_conv_outside_whole_chunks():
    assert fwd_fp8(Cin=32) == N.ENOTSUP and fwd_fp8(Cin=96) == N.ENOTSUP


def test_residual_of_a_data_gradient_that_cannot_fold_it_is_refused_before_any_launch():
    """resid rides only in the fused stride-1 3x3 form; elsewhere the entry answers DGV2_ENOTSUP without touching the device
    (this test runs without one)."""
    assert dgrad(k=1, resid=P16) == N.ENOTSUP
    assert dgrad(H=16, W=64, stride=2, resid=P16) == N.ENOTSUP
    assert dgrad(W=8, resid=P16) == N.ENOTSUP          # the ring wrap of the pipelined kernel needs W > 8
