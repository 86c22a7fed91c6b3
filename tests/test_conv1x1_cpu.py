"""Host-side decisions of dgv2_conv1x1_fwd / dgv2_conv1x1_dgrad (conv1x1.hip): they are taken before anything touches
the device, so they can be held without one.  The pointers are never dereferenced on these paths."""
import pytest

import dgv2_native as N

P16, ODD = 1 << 20, (1 << 20) + 8   # a 16-byte aligned and a misaligned non-null address


def rc(entry, out, a, w, B, P, C, O, resid=None, dt=N.BF16):
    return getattr(N.lib, entry)(out, a, w, B, P, C, O, resid, dt, None)


@pytest.mark.parametrize("entry", ["dgv2_conv1x1_fwd", "dgv2_conv1x1_dgrad"])
def test_invalid_arguments(entry):
    assert rc(entry, None, P16, P16, 1, 32, 32, 64) == -1
    assert rc(entry, P16, None, P16, 1, 32, 32, 64) == -1
    assert rc(entry, P16, P16, None, 1, 32, 32, 64) == -1
    assert rc(entry, P16, P16, P16, 0, 32, 32, 64) == -1
    assert rc(entry, P16, P16, P16, 1, 0, 32, 64) == -1
    assert rc(entry, P16, P16, P16, 1, 32, 0, 64) == -1


@pytest.mark.parametrize("entry", ["dgv2_conv1x1_fwd", "dgv2_conv1x1_dgrad"])
def test_uncovered_geometries_ask_for_the_fallback(entry):
    assert rc(entry, P16, P16, P16, 1, 32, 32, 64, dt=N.F32) == N.ENOTSUP
    assert rc(entry, P16, P16, P16, 1, 32, 48, 64) == N.ENOTSUP
    assert rc(entry, P16, P16, P16, 1, 32, 32, 80) == N.ENOTSUP
    assert rc(entry, ODD, P16, P16, 1, 32, 32, 64) == N.ENOTSUP
    assert rc(entry, P16, ODD, P16, 1, 32, 32, 64) == N.ENOTSUP
    assert rc(entry, P16, P16, ODD, 1, 32, 32, 64) == N.ENOTSUP
    assert rc(entry, P16, P16, P16, 1, 32, 32, 64, resid=ODD) == N.ENOTSUP


def test_contraction_limit_is_per_form():
    """The limit of 512 is on the contraction: C for the forward, O for the data gradient."""
    assert rc("dgv2_conv1x1_fwd", P16, P16, P16, 1, 32, 1024, 64) == N.ENOTSUP
    assert rc("dgv2_conv1x1_dgrad", P16, P16, P16, 1, 32, 64, 1024) == N.ENOTSUP
