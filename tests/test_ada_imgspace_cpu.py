"""CPU checks of the test-side oracle for ADA's image-space stages (tests/ada_imgspace_ref.py) against the fixture made
by the reference itself (tests/golden/ada_imgspace.npz), of the operator algebra that folds the band filter into the
separable form, and of the module's construction-time contract."""
import os

import numpy as np
import pytest
import torch

import ada_imgspace_ref as R
from conftest import GOLDEN

EPS64 = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def fx():
    d = np.load(os.path.join(GOLDEN, "ada_imgspace.npz"))
    return {k: (d[k] if d[k].dtype.kind in "US" else torch.from_numpy(d[k])) for k in d.files}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_reproduces_the_reference(fx, tag):
    """Lines 547-621 restated in float64, fed with the fixture's draws and the reference's own float64 output of the
    stages before them, against the reference's float64 output.  The same arithmetic in the same precision: the bound
    is 256 float64 roundings of the largest output (a 43 x 43-tap sum accumulates about 2 x 43 of them)."""
    want = fx[f"{tag}.y"]
    assert want.dtype == torch.float64 and fx[f"{tag}.y_geo"].dtype == torch.float64
    got = R.image_space_f64(fx[f"{tag}.y_geo"], fx["Hz_fbank"], g=fx[f"{tag}.g"], sigma=fx[f"{tag}.sigma"], cut=fx[f"{tag}.cut"],
                            eps=fx[f"{tag}.eps"])
    err = float((got - want).abs().max())
    print(f"case {tag}: max abs deviation {err:.3e} at magnitude {float(want.abs().max()):.3e}")
    assert err <= 256 * EPS64 * float(want.abs().max())
    # the stored gains are the sequential normalisation of the stored selects / log2-gains
    g = R.band_gains(fx[f"{tag}.band_select"], fx[f"{tag}.log2_gain"])
    assert float((g - fx[f"{tag}.g"]).abs().max()) <= 16 * EPS64 * float(g.abs().max())


def test_bank_is_symmetric_and_sums_to_a_delta(fx):
    fb = fx["Hz_fbank"].double()
    assert tuple(fb.shape) == (4, 43)
    assert torch.equal(fb, fb.flip(1))
    delta = torch.zeros(43, dtype=torch.float64)
    delta[21] = 1.0
    assert float((fb.sum(0) - delta).abs().max()) < 1e-6     # perfect reconstruction: unit gains filter nothing


@pytest.mark.parametrize("H,W,K,sgn", [(24, 96, 32, 1), (24, 96, 32, -1), (26, 64, 32, -1), (22, 21, 8, 1)])
def test_fold_identity(fx, H, W, K, sgn):
    """Filter-after-affine equals the folded operators, in float64:
        Fy (a Ay x Cx^T + c) Fx^T = a (Fy Ay) x (Fx Cx)^T + c (sum h)^2.
    The bank is symmetric, which would hide a wrong flip sign in the circulant composition, so the identity is also
    held with an ASYMMETRIC filter; W < K + 42 makes the composite taps wrap more than once."""
    gen = torch.Generator().manual_seed(H * 1000 + W + K + (sgn < 0))
    x = torch.randn(1, 1, H, W, generator=gen, dtype=torch.float64)
    Ay = torch.randn(H, H, generator=gen, dtype=torch.float64) / H ** 0.5
    kx = torch.randn(K, generator=gen, dtype=torch.float64)
    off, a, c = int(torch.randint(0, W, (1,), generator=gen)), 1.3, -0.4
    g = torch.rand(1, 4, generator=gen, dtype=torch.float64) + 0.5
    banks = [fx["Hz_fbank"].double(), torch.randn(4, 43, generator=gen, dtype=torch.float64) / 6]
    for fbank in banks:
        h = (g @ fbank)[0]
        v = a * (Ay @ x[0, 0] @ R.circulant(kx, off, sgn, W).T) + c
        want = R.image_space_f64(v[None, None], fbank, g=g)[0, 0]
        Ay2, kx2, off2, c2 = R.fold(Ay, kx, off, sgn, c, h, W)
        assert len(kx2) == K + 42
        got = a * (Ay2 @ x[0, 0] @ R.circulant(kx2, off2, sgn, W).T) + c2
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert abs(c2 - c * float(h.sum()) ** 2) <= 1e-15
        # the wrong flip sign is visibly wrong for the asymmetric filter on a flipped sample
        if sgn < 0 and fbank is banks[1]:
            bad = R.fold(Ay, kx, off, 1, c, h, W)
            wrong = a * (bad[0] @ x[0, 0] @ R.circulant(bad[1], bad[2], sgn, W).T) + bad[3]
            assert float((wrong - want).abs().max()) > 1e-3 * float(want.abs().max())


def test_module_accepts_the_multipliers_and_rejects_small_images():
    from gans.augment.adaptive_augment import AdaptiveAugment
    A = AdaptiveAugment(p_init=0.5, imgfilter=1, noise=1, cutout=1)
    assert A.image_space_on() and A.imgfilter_bands == [1, 1, 1, 1] and A.imgfilter_std == 1
    assert not AdaptiveAugment(p_init=0.5, lr_flip=1).image_space_on()
    assert list(AdaptiveAugment().state_dict()) == list(A.state_dict())
    for shape in ((1, 1, 21, 64), (1, 1, 24, 20)):
        with pytest.raises(ValueError, match="too small"):
            A(torch.zeros(shape))
