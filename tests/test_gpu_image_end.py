"""The fp32 kernels at the two ends of the image path, kernel by kernel, against float64 references at their edges
(references, input builders and their conditioning: tests/image_end_ref.py, checked on the CPU by
tests/test_image_end_cpu.py).

1. dgv2_gen_tail_fwd / _bwd (csrc/tail_coords.hip): shapes (3,6,32) (2,5,33) (1,1,7) (2,16,1030), temperature 1 / 0.5 /
   1.7, ray-drop constant -1 / 0 / 0.37, scale 0.25 / 1, shifts None / 0 / negative / below -2 pi / in (2 pi, 4 pi) / just
   below 2 pi; cotangents on each of the four outputs alone (the others None -> NULL) and on all four; the adjoint
   identity of the shift path.
2. dgv2_ada_apply / dgv2_ada_apply_img (csrc/ada.hip) called directly with dense Ay, signed asymmetric taps, both flip
   signs, offsets below -W .. above W, and for the image-space entry sigma (one sample 0), eps and cutout boxes of size
   0, across either border, covering everything and interior: forward, transposed (gradient) and double backward.  The
   table image_end_ref.ADA_CASES names the kernel and the branch of each case.
3. dgv2_coords_convert at and next to every validity threshold, modes 0 (with and without mask), 1 and 2 (d > 0 and
   x > 1e-11 are implied by the depth range and cannot be observed on their own: image_end_ref.coords_inputs).
4. dgv2_sum_squares: strided vectorised rows, strided scalar rows, more than one trip of the unrolled loop with and
   without the grid cap, the zero fill of the slots past the grid.

Bounds of 1 and 2: error = max |got - want| / max |want| against float64; the same reference formula evaluated in float32
on the CPU deviates from float64 by dev32; the bound is max(4 dev32, 1e-5) (image_end_ref.bound), computed from the
reference alone.  Each comparison prints the measured error beside its bound.

Largest measured errors on an MI355X:
  1. generator output stage: 4.1e-6 at W <= 33 (g_skip, all four cotangents, (2,5,33) T = 1.7; bound 1.6e-5, and the
     closest approach to a bound: 0.27 of it); 5.1e-5 at W = 1030 (image_orig under shifts of -4.75 and 1033.37 columns;
     dev32 1.9e-4, bound 7.7e-4: fp32 resolves a position near 2000 to 1.2e-4 of a column); without a shift <= 2.6e-7;
     adjoint identity 1.3e-6 relative at most (3.5e-7 at W = 1030 with shifts of -4.75 and 9.3 columns).
  2. ADA apply kernels: 3.9e-7 (generic kernel, H = 68, K = 64, W = 24, transposed; dev32 2.2e-7, bound 1e-5); the two
     LDS kernels <= 2.8e-7, the image-space entry <= 3.5e-7 (generic, H = 26, K = 74, W = 100, forward);
     ada_apply_img without image-space terms equals ada_apply bit for bit.
  3. coordinate conversion: zero sets identical with no threshold pixel left out, values 0 (modes 0, 1) and 9.6e-8 (2).
  4. sum_squares: <= 6.3e-8 relative in every case, every slot past the grid exactly 0.
"""
import numpy as np
import pytest
import torch

import image_end_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def nat():
    from gans.models.ops import native
    return native


def cl(x):  # NCHW (cpu) -> channels-last on device
    return x.permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(x):  # channels-last (device) -> NCHW cpu
    return x.permute(0, 3, 1, 2).cpu()


def check(what, got, want64, want32):
    dev32 = E.rel_err(want32, want64)
    tol = E.bound(dev32)
    e = E.rel_err(got, want64)
    print(f"{what}: rel err {e:.3e} (reference fp32-vs-fp64 {dev32:.2e}, bound {tol:.1e})")
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"


# ---------------------------------------------------------------------------- 1. generator output stage
def _run_tail(nat, i):
    c = E.tail_case(i)
    sd = cl(c["skip"]).requires_grad_(True)
    shift = None if c["shift"] is None else c["shift"].to(DEV)
    return sd, nat.gen_tail(sd, shift, c["u"].to(DEV), *c["cfg"])


@pytest.mark.parametrize("i", range(len(E.TAIL_CASES)), ids=E.tail_id)
def test_gen_tail_outputs_and_every_cotangent(nat, i):
    c = E.tail_case(i)
    outs64, grads64 = E.tail_reference(i, torch.float64)
    outs32, grads32 = E.tail_reference(i, torch.float32)
    sd, outs = _run_tail(nat, i)
    for k, name in enumerate(E.TAIL_OUTPUTS[:3]):
        check(f"{E.tail_id(i)} {name}", outs[k], outs64[k], outs32[k])
    assert torch.equal(outs[3].cpu().double(), outs64[3].round())       # the margin of tail_case makes it discrete
    for sel, g64, g32 in zip(E.TAIL_COTANGENTS, grads64, grads32):
        (gs,) = torch.autograd.grad([outs[k] for k in sel], sd, [c["cot"][k].to(DEV) for k in sel], retain_graph=True)
        check(f"{E.tail_id(i)} g_skip from {'+'.join(E.TAIL_OUTPUTS[k] for k in sel)}", nchw(gs), g64, g32)


# fp32 resolves the position t = shift / (2 pi) * W to ulp(t): the kernel's Jacobian can match the float64 one to 1e-5 only
# while ulp(t) is below that, |t| < 64 -- every shifted case at W = 7, 32, 33 and the W = 1030 case with small shifts
_ADJOINT = [i for i, c in enumerate(E.TAIL_CASES) if c[4] is not None and 0 < E.tail_max_position(i) < 64]


@pytest.mark.parametrize("i", _ADJOINT, ids=E.tail_id)
def test_gen_tail_shift_path_adjoint_identity(nat, i):
    """<J v, w> == <v, J^T w> accumulated in float64: J v from the float64 reference, J^T w from the kernel, w on all
    four outputs."""
    c = E.tail_case(i)
    assert len(_ADJOINT) >= 6 and any(E.TAIL_CASES[k][0][2] == 1030 for k in _ADJOINT)
    v = torch.randn(c["skip"].shape, generator=torch.Generator().manual_seed(7 + i))
    jv = E.tail_jvp(i, v)
    sd, outs = _run_tail(nat, i)
    (gs,) = torch.autograd.grad(list(outs), sd, [w.to(DEV) for w in c["cot"]])
    lhs = sum(float((a.double() * w.double()).sum()) for a, w in zip(jv, c["cot"]))
    rhs = float((v.double() * nchw(gs).double()).sum())
    print(f"{E.tail_id(i)}: <Jv,w> {lhs:.9e}  <v,JTw> {rhs:.9e}  rel diff {abs(lhs - rhs) / max(abs(lhs), abs(rhs)):.3e}")
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))


# ---------------------------------------------------------------------------- 2. ADA apply with arbitrary operators
def _ada_args(c):
    return [c[k].to(DEV) for k in ("Ay", "kx", "off", "sgn", "a", "c")]


def _ada_call(nat, i, x):
    entry = E.ADA_CASES[i][0]
    c = E.ada_case(i)
    if entry == "apply":
        return nat.ada_apply(x, *_ada_args(c))
    return nat.ada_apply_img(x, *_ada_args(c), cut=c["cut"].to(DEV), sigma=c["sigma"].to(DEV), eps=c["eps"].to(DEV))


@pytest.mark.parametrize("i", range(len(E.ADA_CASES)), ids=E.ada_id)
def test_ada_apply_forward_transposed_and_double_backward(nat, i):
    c = E.ada_case(i)
    (f64, g64, d64), (f32, g32, d32) = E.ada_reference(i, torch.float64), E.ada_reference(i, torch.float32)
    xd = c["x"].to(DEV).requires_grad_(True)
    y = _ada_call(nat, i, xd)
    check(f"{E.ada_id(i)} forward", y, f64, f32)
    gyd = c["cot"].to(DEV).requires_grad_(True)
    (gx,) = torch.autograd.grad(y, xd, gyd, create_graph=True)
    check(f"{E.ada_id(i)} transposed", gx, g64, g32)
    (ggy,) = torch.autograd.grad(gx, gyd, xd.detach())
    check(f"{E.ada_id(i)} double backward", ggy, d64, d32)


def test_ada_apply_img_without_image_space_terms_is_ada_apply(nat):
    i = E.ADA_CASES.index(("apply", 64, 24, 70, "-+-"))                        # K <= 64: two different LDS kernels
    c = E.ada_case(i)
    f64, f32 = E.ada_reference(i, torch.float64)[0], E.ada_reference(i, torch.float32)[0]
    x = c["x"].to(DEV)
    plain = nat.ada_apply(x, *_ada_args(c))
    img = nat.ada_apply_img(x, *_ada_args(c), cut=None, sigma=None, eps=None)
    check("ada_apply_img(cut=None, sigma=None, eps=None)", img, f64, f32)
    tol = E.bound(E.rel_err(f32, f64))
    e = E.rel_err(img, plain.cpu())
    print(f"ada_apply_img vs ada_apply: rel err {e:.3e} (bound {tol:.1e})")
    assert e <= tol


# ---------------------------------------------------------------------------- 3. coordinate conversion at the thresholds
@pytest.mark.parametrize("mode,with_mask,raydrop_const", [(0, False, -1.0), (0, True, -1.0), (0, True, 0.25), (1, False, -1.0),
                                                          (2, False, -1.0)])
def test_coords_convert_at_the_thresholds(nat, mode, with_mask, raydrop_const):
    x, want, compare = E.coords_case(mode, with_mask, raydrop_const)
    d = E.coords_inputs()
    got = nat.coords_convert(torch.from_numpy(x).to(DEV), mode, E.MIN_DEPTH, E.MAX_DEPTH,
                             angle=torch.from_numpy(d["angle"]).to(DEV) if mode == 2 else None,
                             mask=torch.from_numpy(d["mask"]).to(DEV) if with_mask else None,
                             raydrop_const=raydrop_const).cpu().numpy()
    assert got.shape == want.shape
    sel = np.broadcast_to(compare, want.shape)
    print(f"mode {mode} mask {with_mask}: {int((~compare).sum())} threshold pixels left out, "
          f"{int(((want == (-1.0 if with_mask else 0.0)) & sel).sum())} rejected values compared")
    # a pixel the predicates reject is 0 (blended: -1 under the mask, where the mask keeps the pixel); valid values are
    # positive (in (-0.97, 1] after the blend), so the set is read off the value
    zero = np.float32(-1.0) if with_mask else np.float32(0.0)
    kept = np.broadcast_to(d["mask"] == 1, want.shape) if with_mask else np.ones(want.shape, dtype=bool)
    assert np.array_equal((got == zero)[sel & kept], (want == zero)[sel & kept])
    assert (want == zero)[sel & kept].any() and (want != zero)[sel & kept].any()
    err = float(np.abs(got.astype(np.float64) - want)[sel].max() / np.abs(want[sel]).max())
    print(f"mode {mode} mask {with_mask}: rel err {err:.3e}")
    assert err <= 2e-6


# ---------------------------------------------------------------------------- 4. sum_squares branches
def _sum_squares(nat, x, C=None):
    """nat.sum_squares right after a freed NaN-filled tensor of the partials' size: the allocator then most likely hands the
    kernel dirty memory (the assertions do not rely on that)."""
    scratch = torch.full((512,), float("nan"), device=DEV)
    torch.cuda.synchronize()
    del scratch
    got = nat.sum_squares(x, C=C)
    assert got.shape == (512,) and got.dtype == torch.float32
    return got.cpu()


def _blocks(nvec_or_elems):
    return min(512, max(1, -(-nvec_or_elems // 2048)))


@pytest.mark.parametrize("dtype,tol,C,kernel", [
    (torch.float32, 1e-5, 16, "vec"), (torch.float32, 1e-5, 8, "vec"),     # cvecs = 4, 2 of ld / VN = 10
    (torch.bfloat16, 1e-2, 16, "vec"), (torch.bfloat16, 1e-2, 8, "vec"),   # cvecs = 2, 1 of ld / VN = 5
    (torch.bfloat16, 1e-2, 12, "scalar"),                                  # C % 8 != 0: scalar kernel on strided rows
])
def test_sum_squares_strided_rows(nat, dtype, tol, C, kernel):
    x = torch.randn(3, 7, 9, 40, generator=torch.Generator().manual_seed(0)).to(dtype)
    vn = 16 // x.element_size()
    assert (C % vn == 0 and 40 % vn == 0) == (kernel == "vec") and C // vn != 40 // vn
    want = float(x[..., :C].double().pow(2).sum())
    got = _sum_squares(nat, x.to(DEV), C)
    rows = x.numel() // 40
    nb = _blocks(rows * C // vn if kernel == "vec" else rows * C)
    assert torch.equal(got[nb:], torch.zeros(512 - nb)) and bool((got[:nb] > 0).all())
    e = abs(float(got.double().sum()) - want) / want
    print(f"sum_squares {dtype} C={C} ({kernel}, strided): rel err {e:.3e}")
    assert e <= tol


@pytest.mark.parametrize("rows,blocks", [(4100, 257), (8200, 512)])
def test_sum_squares_more_than_one_trip(nat, rows, blocks):
    """[4100,512] fp32 is 524 800 vectors, more than 512 * 256 * 4: no launch covers it in one trip of the four-deep loop
    (its grid is 257 blocks: two trips, the second partial).  [8200,512] is past 512 blocks of 2048 vectors as well: the
    grid is capped and the loop runs three times."""
    x = torch.randn(rows, 512, generator=torch.Generator().manual_seed(1))
    assert rows * 128 > 512 * 256 * 4 and _blocks(rows * 128) == blocks
    want = float(x.double().pow(2).sum())
    got = _sum_squares(nat, x.to(DEV))
    assert got.shape == (512,)
    assert torch.equal(got[blocks:], torch.zeros(512 - blocks)) and bool((got[:blocks] > 0).all())
    e = abs(float(got.double().sum()) - want) / want
    print(f"sum_squares [{rows},512]: rel err {e:.3e}")
    assert e <= 1e-5


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 1e-2)])
def test_sum_squares_tiny_tensor_zero_fills_every_other_slot(nat, dtype, tol):
    x = torch.tensor([0.5, -1.25, 2.0, 3.0]).reshape(1, 1, 1, 4).to(dtype)
    got = _sum_squares(nat, x.to(DEV))
    assert torch.equal(got[1:], torch.zeros(511))
    want = float(x.double().pow(2).sum())
    assert abs(float(got[0]) - want) <= tol * want
