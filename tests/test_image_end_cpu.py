"""The CPU half of tests/test_gpu_image_end.py: every input builder of tests/image_end_ref.py runs here (each asserts its
own conditioning), the case tables cover what they claim to cover, and the float64 restatements agree with the oracle
they restate."""
import numpy as np
import pytest
import torch

import image_end_ref as E
from oracle import ops as o


# ---------------------------------------------------------------------------- 1. generator output stage
@pytest.mark.parametrize("i", range(len(E.TAIL_CASES)), ids=E.tail_id)
def test_tail_case_conditions_and_reference(i):
    c = E.tail_case(i)                                     # asserts the shift fractions and the Gumbel margin
    outs64, grads64 = E.tail_reference(i, torch.float64)
    outs32, _ = E.tail_reference(i, torch.float32)
    assert all(t.dtype == torch.float64 for t in outs64 + grads64)
    assert torch.equal(outs64[3].round(), outs32[3].round().double())      # the margin holds the mask in fp32 too
    assert 0 < float(outs64[3].round().mean()) < 1 or c["skip"].shape[3] == 7
    for k in range(3):
        assert E.rel_err(outs32[k], outs64[k]) < 1e-3
    if c["shift"] is not None:                             # in float32 the restatement IS the oracle's formula
        assert torch.equal(E.ring_shift(c["skip"], c["shift"]), o.ring_shift(c["skip"], c["shift"]))
    # the cotangent on the mask alone reaches skip (straight-through), the one on image_orig alone only channel 0
    assert float(grads64[3][:, 1].abs().max()) > 0 and float(grads64[1][:, 1].abs().max()) == 0


def test_tail_table_covers_every_value():
    shapes = {c[0] for c in E.TAIL_CASES}
    assert shapes == {(3, 6, 32), (2, 5, 33), (1, 1, 7), (2, 16, 1030)}
    assert {c[1] for c in E.TAIL_CASES} == {1.0, 0.5, 1.7}
    assert {c[2] for c in E.TAIL_CASES} == {-1.0, 0.0, 0.37}
    assert {c[3] for c in E.TAIL_CASES} == {0.25, 1.0}
    kinds = {k for c in E.TAIL_CASES if c[4] for k in c[4]}
    assert kinds == {"zero", "neg", "small", "neg_wrap", "over", "below"} and any(c[4] is None for c in E.TAIL_CASES)
    for s in shapes:                                       # every shape with and without a shift
        assert {c[4] is None for c in E.TAIL_CASES if c[0] == s} == {True, False}


def test_tail_jvp_is_the_transpose_of_the_reference_gradient():
    i = 0
    c = E.tail_case(i)
    v = torch.randn(c["skip"].shape, generator=torch.Generator().manual_seed(1))
    jv = E.tail_jvp(i, v)
    lhs = sum(float((a * w.double()).sum()) for a, w in zip(jv, c["cot"]))
    rhs = float((v.double() * E.tail_reference(i, torch.float64)[1][4]).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))


# ---------------------------------------------------------------------------- 2. ADA
@pytest.mark.parametrize("i", range(len(E.ADA_CASES)), ids=E.ada_id)
def test_ada_case_conditions_and_reference(i):
    entry, H, K, W, signs = E.ADA_CASES[i]
    c = E.ada_case(i)                                      # asserts both signs, the box margins, sigma = 0 somewhere
    fwd, grad, lin = E.ada_reference(i, torch.float64)
    assert fwd.shape == grad.shape == lin.shape == (E.ADA_B, 1, H, W)
    assert [int(v) for v in c["sgn"]] == [1 if ch == "+" else -1 for ch in signs] and set(signs) == {"+", "-"}
    # (ada_reference asserts that a sample with an offset beyond +-W has non-zero results: something survives its cutout)
    # the explicit transpose is the adjoint of the linear part: <lin(x), g> == <x, grad(g)>
    lhs, rhs = float((lin * c["cot"].double()).sum()), float((c["x"].double() * grad).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs))
    # the circulant against the index formula of include/dgv2.h at a few places
    Cx, b, j = E.ada_operator(i), 1, W // 3
    want = sum(float(c["kx"][b, t]) * float(c["x"][b, 0, 0, (int(c["sgn"][b]) * j + int(c["off"][b]) + t) % W]) for t in range(K))
    assert abs(float((c["x"][b, 0, 0].double() * Cx[b, j]).sum()) - want) <= 1e-9 * max(1.0, abs(want))


def test_ada_table_covers_every_kernel_and_branch():
    by = {}
    for i, (entry, H, K, W, _) in enumerate(E.ADA_CASES):
        by.setdefault((entry, E.ada_kernel(entry, H, K)), []).append((i, H, K, W))
    assert set(by) == {("apply", "lds"), ("apply", "generic"), ("img", "img_lds"), ("img", "generic")}
    want_h = {("apply", "lds"): {4, 8, 20, 64}, ("apply", "generic"): {6, 8, 26, 68}, ("img", "img_lds"): {8, 24, 64},
              ("img", "generic"): {8, 26}}
    kmax = {("apply", "lds"): 64, ("apply", "generic"): 64, ("img", "img_lds"): 80, ("img", "generic"): 74}
    for key, cases in by.items():
        assert {h for _, h, _, _ in cases} == want_h[key], key
        for h in want_h[key]:
            mine = [(k, w) for _, hh, k, w in cases if hh == h]
            assert max(k for k, _ in mine) >= kmax[key] and min(w for _, w in mine) == 24, (key, h)
        # every kind of offset and (image entry) of box reaches every kernel
        assert {k for i, *_ in cases for k in E.ada_case(i)["off_kinds"]} == set(E.OFF_KINDS), key
        # ... with either flip sign, and for the image entry under a box that keeps something
        for kind in ("over", "under"):
            hits = {(int(E.ada_case(i)["sgn"][b]), (E.ada_case(i)["cut_kinds"] or [None] * 3)[b])
                    for i, *_ in cases for b in range(E.ADA_B) if E.ada_case(i)["off_kinds"][b] == kind}
            assert {s_ for s_, _ in hits} == {1, -1} and all(ck != "all" for _, ck in hits), (key, kind, hits)
        if key[0] == "img":
            assert {k for i, *_ in cases for k in E.ada_case(i)["cut_kinds"]} == set(E.CUT_KINDS), key
    ks, ws = {c[2] for c in E.ADA_CASES}, {c[3] for c in E.ADA_CASES}
    assert {1, 3, 24, 64, 65, 74, 80, 81} <= ks and {24, 64, 96, 100, 200} <= ws and ws & {70, 98}
    # the dispatch boundaries from both sides at the same (H, W)
    for entry, k in (("apply", 64), ("img", 80)):
        below = {(h, w) for e, h, kk, w, _ in E.ADA_CASES if e == entry and kk == k and E.ada_kernel(e, h, kk) != "generic"}
        above = {(h, w) for e, h, kk, w, _ in E.ADA_CASES if e == entry and kk == k + 1}
        assert len(below & above) >= 2, (entry, k)
    assert all(E.ada_kernel(e, h, k) == "generic" for e, h, k, _, _ in E.ADA_CASES if k in (65, 81) or h % 4 or h > 64)


# ---------------------------------------------------------------------------- 3. coordinates
@pytest.mark.parametrize("mode,with_mask", [(0, False), (0, True), (1, False), (2, False)])
def test_coords_case_conditions(mode, with_mask):
    x, want, compare = E.coords_case(mode, with_mask, 0.25)     # asserts: no neighbour of a threshold is ambiguous
    d = E.coords_inputs()
    thr = d["depth_thr"] if mode == 0 else d["inv_thr"]
    assert x.shape == E.COORD_SHAPE and x.dtype == np.float32 and np.isfinite(want).all()
    assert not (~compare & ~thr).any()
    # each flagged threshold sits between its two fp32 neighbours in the flattened first sample
    flat, tf = x[0].ravel(), thr[0].ravel()
    for p in np.nonzero(tf)[0]:
        assert flat[p - 1] == np.nextafter(flat[p], np.float32(-np.inf)) and flat[p + 1] == np.nextafter(flat[p], np.float32(np.inf))
    want_thr = ({1.45, 80.0, 0.0} if mode == 0 else {1.0, 1.45 / 80.0, 0.0, 1e-11})
    assert all(any(abs(float(v) - t) <= 1e-6 * t for v in flat[tf]) for t in want_thr)
    assert set(np.unique(d["mask"])) == {0.0, 1.0}
