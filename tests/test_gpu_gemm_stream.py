"""gemm_stream.hip: the staged-delivery engines of the generator's level-0 / level-1 per-sample-weight contractions
(dgv2_gemm_stream_nn / _nn_cat / _tn / _tn_cat) against the generic engines they stand in for (dgv2_bmm_nn_sq /
dgv2_bmm_nn_cat_sq / dgv2_bmm_tn / dgv2_bmm_tn_cat).

The claim is "the same bits": same tile, same fragment ownership, K-steps of 32 ascending into one accumulator, same
epilogue.  So every case runs the new entry directly, the routed call with the module flag off (the generic kernel) and
with it on, on canary-guarded outputs, and requires torch.equal -- of y, of EVERY sum-of-squares partial slot and of
sumsq_used on the NN forms, of gw on the TN forms.  Random bf16 operands carry the claim (the summation order);
small-integer operands ({-1, 0, 1}: every sum exact) are the second case, because they localise a fragment-map slip.

Shapes (the smallest at which each path of the kernels is taken):
* NN: B = 2, 3; P = 128 (one whole pixel tile), 160 (a ragged second tile); (Ka, Ks) = (0, 64) the level-0 form,
  (32, 64) a split inside a stage, (64, 96) five K-steps = one whole stage and a single-step tail, and (512, 512) once:
  the real depth, eight stages; O = 128, 192 (a half-empty second row tile), 256; bare, and with bias + leaky ReLU +
  row scale + partials.  The data gradient (dense form) at the same P with K = 64, 256 and O = 128, 512, with and
  without the residual.
* TN: P = 128 (one stage), 160 (a ragged last K-step in a second stage, zero-filled); O = 64, 256; J = 128, 192, 1024
  with Ka = 0 and Ka > 0.
* every refused geometry returns DGV2_ENOTSUP, writes nothing, and the routed call gives the generic result.
* one accuracy case per form against a float64 reference built on the CPU from the same bf16 values, the rule of
  test_gpu_conv1x1: the new kernel's deviation <= 1.5 x the generic kernel's own + 1e-3 of the output's maximum."""
import ctypes
import itertools

import pytest
import torch

import dgv2_native as N
from gans.models.ops.native import modgemm
from test_gpu_conv1x1 import guarded_empty

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SQ_CAP = 64
ALPHA, SCALE = 0.2, 2.0 ** 0.5
SENTINEL = float("nan")   # preset of every output: an element no kernel writes stays NaN, and NaN != NaN fails torch.equal


@pytest.fixture
def stream_switch():
    old = modgemm._GEMM_STREAM
    yield lambda on: setattr(modgemm, "_GEMM_STREAM", bool(on))
    modgemm._GEMM_STREAM = old


def make(shape, integer, g, scale=1.0):
    if integer:
        t = torch.randint(-1, 2, shape, generator=g).float()
    else:
        t = torch.randn(*shape, generator=g) * scale
    return t.to(BF).contiguous().to(DEV)


def epilogue_args(O, full, integer, g):
    """(row_scale, bias, act) fp32 on the device; integer data: powers of two and small integers keep every value exact."""
    if not full:
        return None, None, 0
    if integer:
        rs = (2.0 ** torch.randint(-1, 2, (O,), generator=g).float())
        b = torch.randint(-2, 3, (O,), generator=g).float()
    else:
        rs = torch.rand(O, generator=g) + 0.5
        b = torch.randn(O, generator=g)
    return rs.to(DEV), b.to(DEV), 3


class Sq:
    """A sum-of-squares partial buffer with every slot preset (an unwritten slot shows) and the sumsq_used word."""

    def __init__(self, on):
        self.buf = torch.full((SQ_CAP,), -1.0, device=DEV) if on else None
        self.used = ctypes.c_int(-7)

    def args(self):
        if self.buf is None:
            return None, 0, None
        return N.ptr(self.buf), SQ_CAP, ctypes.addressof(self.used)

    def state(self):
        torch.cuda.synchronize()
        return (None if self.buf is None else self.buf.clone(), self.used.value if self.buf is not None else None)


def same_sq(a, b):
    return a[1] == b[1] and (a[0] is None or torch.equal(a[0], b[0]))


# ------------------------------------------------------------------------------------------------------------------
# NN, concatenated form (forward of the level-input conv)
# ------------------------------------------------------------------------------------------------------------------
def nn_cat_operands(B, P, Ka, Ks, O, integer, seed):
    g = torch.Generator().manual_seed(seed)
    K = Ka + Ks
    xa = make((B, P, Ka), integer, g) if Ka else None
    xs = make((P, Ks), integer, g)
    w = make((B, O, K), integer, g, 1.0 if integer else K ** -0.5)
    return xa, xs, w


def nn_cat_run(how, t, B, P, Ka, Ks, O, epi, with_sq):
    """how: 'new' (the entry itself; must accept), 'routed' (modgemm's call, whichever engine the flag selects)."""
    xa, xs, w = t
    rs, b, act = epi
    y, check = guarded_empty((B, P, O))
    y.fill_(SENTINEL)     # a store that BOTH engines miss must not compare equal by allocator luck
    sq = Sq(with_sq)
    args = (N.ptr(y), N.ptr(xa), N.ptr(xs), N.ptr(w), B, P, Ka, Ks, O, N.ptr(rs), N.ptr(b), act, ALPHA, SCALE, N.BF16,
            N.BF16, *sq.args(), N.stream())
    if how == "new":
        assert N.try_call("dgv2_gemm_stream_nn_cat", *args), "the new entry refused a geometry it is built for"
    else:
        modgemm.bmm_nn_cat_sq_call(*args)
    check()
    return y, sq.state()


NN_CAT = [(B, P, Ka, Ks, O, full) for B, P in ((2, 128), (3, 160), (2, 160), (3, 128))
          for Ka, Ks in ((0, 64), (32, 64), (64, 96)) for O in (128, 192, 256) for full in (False, True)]
NN_CAT.append((2, 128, 512, 512, 256, True))


@pytest.mark.parametrize("integer", [False, True], ids=["random", "integer"])
@pytest.mark.parametrize("B,P,Ka,Ks,O,full", NN_CAT,
                         ids=[f"B{B}-P{P}-K{Ka}+{Ks}-O{O}-{'epi' if f else 'bare'}" for B, P, Ka, Ks, O, f in NN_CAT])
def test_nn_cat_same_bits(B, P, Ka, Ks, O, full, integer, stream_switch):
    t = nn_cat_operands(B, P, Ka, Ks, O, integer, 21)
    epi = epilogue_args(O, full, integer, torch.Generator().manual_seed(22))
    new, sq_new = nn_cat_run("new", t, B, P, Ka, Ks, O, epi, full)
    stream_switch(False)
    old, sq_old = nn_cat_run("routed", t, B, P, Ka, Ks, O, epi, full)
    stream_switch(True)
    routed, sq_routed = nn_cat_run("routed", t, B, P, Ka, Ks, O, epi, full)
    if full:
        assert sq_old[1] == B * ((O + 127) // 128) * ((P + 127) // 128)       # the generic kernel did leave partials
    if integer and not full:
        xa, xs, w = t
        x = xs.double().cpu().expand(B, P, Ks)
        if Ka:
            x = torch.cat([xa.double().cpu(), x], dim=2)
        assert torch.equal(old.double().cpu(), x @ w.double().cpu().transpose(1, 2)), "the generic engine is off on exact data"
    assert torch.equal(new, old)
    assert same_sq(sq_new, sq_old)
    assert torch.equal(routed, old)
    assert same_sq(sq_routed, sq_old)


# ------------------------------------------------------------------------------------------------------------------
# NN, dense form (the data gradient)
# ------------------------------------------------------------------------------------------------------------------
def nn_run(how, x, w, resid, B, P, K, O, epi=(None, None, 0), with_sq=False):
    rs, b, act = epi
    y, check = guarded_empty((B, P, O))
    y.fill_(SENTINEL)     # a store that BOTH engines miss must not compare equal by allocator luck
    sq = Sq(with_sq)
    args = (N.ptr(y), N.ptr(x), N.ptr(w), B, P, K, O, K, O, O * K, N.ptr(rs), N.ptr(b), act, ALPHA, SCALE, N.ptr(resid),
            N.BF16, N.BF16, *sq.args(), N.stream())
    if how == "new":
        assert N.try_call("dgv2_gemm_stream_nn", *args), "the new entry refused a geometry it is built for"
    else:
        modgemm.bmm_nn_sq_call(*args)
    check()
    return y, sq.state()


NN_DENSE = [(B, P, K, O, r) for B, P in ((2, 128), (3, 160), (2, 160), (3, 128)) for K in (64, 256) for O in (128, 512) for r in (False, True)]


@pytest.mark.parametrize("integer", [False, True], ids=["random", "integer"])
@pytest.mark.parametrize("B,P,K,O,with_resid", NN_DENSE,
                         ids=[f"B{B}-P{P}-K{K}-O{O}-{'resid' if r else 'bare'}" for B, P, K, O, r in NN_DENSE])
def test_nn_dense_same_bits(B, P, K, O, with_resid, integer, stream_switch):
    g = torch.Generator().manual_seed(31)
    x = make((B, P, K), integer, g)
    w = make((B, O, K), integer, g, 1.0 if integer else K ** -0.5)
    resid = make((B, P, O), integer, g) if with_resid else None
    new, _ = nn_run("new", x, w, resid, B, P, K, O)
    stream_switch(False)
    old, _ = nn_run("routed", x, w, resid, B, P, K, O)
    old_raw = modgemm._bmm_nn_raw(x, w, BF, resid=resid)
    stream_switch(True)
    routed, _ = nn_run("routed", x, w, resid, B, P, K, O)
    routed_raw = modgemm._bmm_nn_raw(x, w, BF, resid=resid)       # the call the layers make (with and without resid)
    if integer:
        want = x.double().cpu() @ w.double().cpu().transpose(1, 2) + (resid.double().cpu() if with_resid else 0.0)
        assert float(want.abs().max()) <= 256
        assert torch.equal(old.double().cpu(), want), "the generic engine is off on exact data"
    assert torch.equal(new, old)
    assert torch.equal(routed, old)
    assert torch.equal(old_raw, old)
    assert torch.equal(routed_raw, old)


def test_nn_dense_epilogue_and_partials(stream_switch):
    """The dense form with the whole epilogue (row scale, bias, leaky ReLU, residual, partials): B = 3, P = 160, K = 96."""
    B, P, K, O = 3, 160, 96, 192
    g = torch.Generator().manual_seed(32)
    x, w, resid = make((B, P, K), False, g), make((B, O, K), False, g, K ** -0.5), make((B, P, O), False, g)
    epi = epilogue_args(O, True, False, g)
    new, sq_new = nn_run("new", x, w, resid, B, P, K, O, epi, True)
    stream_switch(False)
    old, sq_old = nn_run("routed", x, w, resid, B, P, K, O, epi, True)
    assert sq_old[1] == B * 2 * 2
    assert torch.equal(new, old)
    assert same_sq(sq_new, sq_old)


@pytest.mark.parametrize("shared", [False, True], ids=["per-sample", "shared-w"])
def test_nn_dense_many_tiles_and_shared_weights(shared, stream_switch):
    """What the ENTRY takes beyond the routed shapes: a pixel axis of many tiles with a ragged last one (P = 1100: nine
    tiles) and batch-shared weights (wstride = 0, w [1, O, K]).  The layers' call keeps such shapes on the generic engine
    (modgemm._GEMM_STREAM_MAX_P, per-sample weights only), so `routed` is the generic result by construction."""
    B, P, K, O = 2, 1100, 128, 192
    g = torch.Generator().manual_seed(33)
    x, w = make((B, P, K), False, g), make((1 if shared else B, O, K), False, g, K ** -0.5)
    y, check = guarded_empty((B, P, O))
    y.fill_(SENTINEL)
    args = (N.ptr(y), N.ptr(x), N.ptr(w), B, P, K, O, K, O, 0 if shared else O * K, None, None, 0, ALPHA, SCALE, None, N.BF16,
            N.BF16, None, 0, None, N.stream())
    assert N.try_call("dgv2_gemm_stream_nn", *args)
    check()
    stream_switch(False)
    old = modgemm._bmm_nn_raw(x, w, BF)
    stream_switch(True)
    routed = modgemm._bmm_nn_raw(x, w, BF)
    assert torch.equal(y, old)
    assert torch.equal(routed, old)


# ------------------------------------------------------------------------------------------------------------------
# TN (the weight gradients)
# ------------------------------------------------------------------------------------------------------------------
def tn_run(how, gy, xa, xs, B, P, Ka, Ks, O, dense):
    J = Ka + Ks
    gw, check = guarded_empty((B, O, J), torch.float32)
    gw.fill_(SENTINEL)
    if dense:
        args = (N.ptr(gw), N.ptr(gy), N.ptr(xa), B, P, J, O, O, J, N.BF16, N.stream())
        entry, routed = "dgv2_gemm_stream_tn", modgemm.bmm_tn_call
    else:
        args = (N.ptr(gw), N.ptr(gy), N.ptr(xa), N.ptr(xs), B, P, Ka, Ks, O, N.BF16, N.stream())
        entry, routed = "dgv2_gemm_stream_tn_cat", modgemm.bmm_tn_cat_call
    if how == "new":
        assert N.try_call(entry, *args), "the new entry refused a geometry it is built for"
    else:
        routed(*args)
    check()
    return gw


# (Ka, Ks): J = 128, 192, 1024, each with Ka = 0 and Ka > 0; None = the dense entry with I = J
TN_SPLITS = [(0, 128), (64, 64), (0, 192), (64, 128), (0, 1024), (512, 512), (128, None), (192, None), (1024, None)]
TN = [(B, P, O, ka, ks) for (B, P), O in itertools.product(((2, 128), (3, 160)), (64, 256)) for ka, ks in TN_SPLITS]


@pytest.mark.parametrize("integer", [False, True], ids=["random", "integer"])
@pytest.mark.parametrize("B,P,O,Ka,Ks", TN, ids=[f"B{B}-P{P}-O{O}-J{ka}+{ks}" for B, P, O, ka, ks in TN])
def test_tn_same_bits(B, P, O, Ka, Ks, integer, stream_switch):
    g = torch.Generator().manual_seed(41)
    dense = Ks is None
    gy = make((B, P, O), integer, g)
    if dense:
        xa, xs, Ka, Ks = make((B, P, Ka), integer, g), None, Ka, 0
    else:
        xa, xs = (make((B, P, Ka), integer, g) if Ka else None), make((P, Ks), integer, g)
    new = tn_run("new", gy, xa, xs, B, P, Ka, Ks, O, dense)
    stream_switch(False)
    old = tn_run("routed", gy, xa, xs, B, P, Ka, Ks, O, dense)
    stream_switch(True)
    routed = tn_run("routed", gy, xa, xs, B, P, Ka, Ks, O, dense)
    if integer:
        x = xa.double().cpu() if dense else xs.double().cpu().expand(B, P, Ks)
        if not dense and Ka:
            x = torch.cat([xa.double().cpu(), x], dim=2)
        assert torch.equal(old.double().cpu(), gy.double().cpu().transpose(1, 2) @ x), "the generic engine is off on exact data"
    assert torch.equal(new, old)
    assert torch.equal(routed, old)


# ------------------------------------------------------------------------------------------------------------------
# refusals: DGV2_ENOTSUP, nothing written, the routed call gives the generic result
# ------------------------------------------------------------------------------------------------------------------
def test_refused_geometries_fall_through(stream_switch):
    g = torch.Generator().manual_seed(51)
    B, P = 2, 128
    # NN cat: 64 output channels (the generic TO = 64 instance), a contraction off the 32-grid, a split off the 32-grid, fp32
    for Ka, Ks, O, dt in ((32, 64, 64, BF), (0, 40, 128, BF), (8, 56, 128, BF), (32, 64, 128, torch.float32)):
        xa = make((B, P, Ka), False, g).to(dt) if Ka else None
        xs, w = make((P, Ks), False, g).to(dt), make((B, O, Ka + Ks), False, g, 0.1).to(dt)
        y, check = guarded_empty((B, P, O), dt)
        y.fill_(7.0)
        code = N.BF16 if dt == BF else N.F32
        args = (N.ptr(y), N.ptr(xa), N.ptr(xs), N.ptr(w), B, P, Ka, Ks, O, None, None, 0, ALPHA, SCALE, code, code, None, 0,
                None, N.stream())
        assert not N.try_call("dgv2_gemm_stream_nn_cat", *args)
        check()
        assert bool((y == 7.0).all())
        N.call("dgv2_bmm_nn_cat_sq", *args)
        old = y.clone()
        y.fill_(7.0)
        stream_switch(True)
        modgemm.bmm_nn_cat_sq_call(*args)
        check()
        assert torch.equal(y, old)
    # NN dense: a misaligned operand (the generic kernel takes its element-wise loads), 64 output channels, K = 48
    for K, O, off in ((64, 128, 4), (64, 64, 0), (48, 128, 0)):
        xbuf = make((B * P * K + 8,), False, g)
        x = xbuf[off:off + B * P * K].view(B, P, K)
        w = make((B, O, K), False, g, 0.1)
        y, check = guarded_empty((B, P, O))
        y.fill_(7.0)
        args = (N.ptr(y), N.ptr(x), N.ptr(w), B, P, K, O, K, O, O * K, None, None, 0, ALPHA, SCALE, None, N.BF16, N.BF16, None, 0,
                None, N.stream())
        assert not N.try_call("dgv2_gemm_stream_nn", *args)
        check()
        assert bool((y == 7.0).all())
        N.call("dgv2_bmm_nn_sq", *args)
        old = y.clone()
        y.fill_(7.0)
        modgemm.bmm_nn_sq_call(*args)
        check()
        assert torch.equal(y, old)
    # TN: 32 output channels (the generic TO = 32 instance), fp32, and a split-K geometry (B = 1, P = 1024, few tiles)
    for Bt, Pt, O, J, dt in ((2, 128, 32, 128, BF), (2, 128, 64, 128, torch.float32), (1, 1024, 64, 128, BF)):
        gy, x = make((Bt, Pt, O), False, g).to(dt), make((Bt, Pt, J), False, g).to(dt)
        gw, check = guarded_empty((Bt, O, J), torch.float32)
        gw.fill_(7.0)
        code = N.BF16 if dt == BF else N.F32
        args = (N.ptr(gw), N.ptr(gy), N.ptr(x), Bt, Pt, J, O, O, J, code, N.stream())
        assert not N.try_call("dgv2_gemm_stream_tn", *args)
        cat_args = (N.ptr(gw), N.ptr(gy), None, N.ptr(x[0].contiguous()), Bt, Pt, 0, J, O, code, N.stream())
        assert not N.try_call("dgv2_gemm_stream_tn_cat", *cat_args)
        check()
        assert bool((gw == 7.0).all())
        N.call("dgv2_bmm_tn", *args)
        old = gw.clone()
        gw.fill_(7.0)
        modgemm.bmm_tn_call(*args)
        check()
        assert torch.equal(gw, old)


# ------------------------------------------------------------------------------------------------------------------
# accuracy against float64 (one case per form)
# ------------------------------------------------------------------------------------------------------------------
def test_nn_accuracy_against_float64(stream_switch):
    B, P, Ka, Ks, O = 2, 128, 512, 512, 256
    t = nn_cat_operands(B, P, Ka, Ks, O, False, 61)
    epi = epilogue_args(O, True, False, torch.Generator().manual_seed(62))
    new, _ = nn_cat_run("new", t, B, P, Ka, Ks, O, epi, True)
    stream_switch(False)
    old, _ = nn_cat_run("routed", t, B, P, Ka, Ks, O, epi, True)
    xa, xs, w = (v.double().cpu() for v in t)
    rs, b = epi[0].double().cpu(), epi[1].double().cpu()
    pre = torch.cat([xa, xs.expand(B, P, Ks)], dim=2) @ w.transpose(1, 2) * rs + b
    want = torch.where(pre > 0, pre, pre * ALPHA) * SCALE
    dev_new = float((new.double().cpu() - want).abs().max())
    dev_old = float((old.double().cpu() - want).abs().max())
    print(f"gemm_stream nn_cat B{B} P{P} K{Ka}+{Ks} O{O}: new {dev_new:.3e}, generic engine {dev_old:.3e}, "
          f"max |ref| {float(want.abs().max()):.3e}")
    assert dev_new <= 1.5 * dev_old + 1e-3 * float(want.abs().max())


def test_tn_accuracy_against_float64(stream_switch):
    B, P, Ka, Ks, O = 3, 160, 64, 128, 64
    g = torch.Generator().manual_seed(63)
    gy, xa, xs = make((B, P, O), False, g), make((B, P, Ka), False, g), make((P, Ks), False, g)
    new = tn_run("new", gy, xa, xs, B, P, Ka, Ks, O, False)
    stream_switch(False)
    old = tn_run("routed", gy, xa, xs, B, P, Ka, Ks, O, False)
    x = torch.cat([xa.double().cpu(), xs.double().cpu().expand(B, P, Ks)], dim=2)
    want = gy.double().cpu().transpose(1, 2) @ x
    dev_new = float((new.double().cpu() - want).abs().max())
    dev_old = float((old.double().cpu() - want).abs().max())
    print(f"gemm_stream tn_cat B{B} P{P} J{Ka}+{Ks} O{O}: new {dev_new:.3e}, generic engine {dev_old:.3e}, "
          f"max |ref| {float(want.abs().max()):.3e}")
    assert dev_new <= 1.5 * dev_old + 1e-3 * float(want.abs().max())
