"""conv1x1.hip: the 1x1 stride-1 bf16 conv as a streaming GEMM (dgv2_conv1x1_fwd / dgv2_conv1x1_dgrad), the kernels the
residual blocks' skip conv runs on.

Shapes: the channel pairs (32, 64), (64, 128) and (256, 512) reach both slab widths (32 / 64 output channels: the data
gradient of (32, 64) has 32), every K-chunk depth (32, 64 and 128-channel multiples), several slabs per launch and the
largest weight slab; B = 2 at 4 x 32 pixels is whole 32-pixel wave tiles and whole 128-pixel blocks, B = 3 at 2 x 20 is 120
pixels: a ragged last tile and an idle wave.  Every case with and without the residual.

* guarded buffers: the entries are called on outputs with canary words behind them;
* integer exactness: on small-integer operands every sum is exact in fp32 and every result a bf16 value, so the new
  kernels must torch.equal the direct engine (the module flag flipped) -- any slip in a fragment map shows;
* accuracy: on random operands, against a float64 reference built on the CPU from the same bf16 values, the new kernel's
  maximum deviation may not exceed 1.5 x the direct engine's own deviation + 1e-3 of the output's maximum (the rule of
  test_gpu_full.check_vs_fixture, measured against the reference); both deviations are printed; and, since the kernel
  keeps the direct engine's summation order and epilogue arithmetic, the two results must also be torch.equal;
* block level: one ResidualBlock(64, 128) forward + backward at B = 2, 8 x 64 with the flag on and off against the
  float64 oracle of the block, same rule, and the status word stays 0.

The weight gradient of the skip conv stays on dgv2_conv_wgrad_stream_pl: nothing of it is tested here."""
import pytest
import torch

import dgv2_native as N
from gans.models.ops import native
from gans.models.ops.native import conv as nconv

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

PAIRS = [(32, 64), (64, 128), (256, 512)]
SIZES = [(2, 4, 32), (3, 2, 20)]
GEOM = native.ConvGeom(1, 1, 1, 0, True)
_GUARD_WORDS, _GUARD_PATTERN = 64, 0x5A5A5A5A


def guarded_empty(shape, dtype=BF):
    """torch.empty(shape) with canary words behind it (bench.guarded_empty's pattern) -> (tensor, check())."""
    n = 1
    for d in shape:
        n *= int(d)
    esz = torch.empty((), dtype=dtype).element_size()
    nbytes = (n * esz + 15) // 16 * 16
    flat = torch.empty(nbytes + 4 * _GUARD_WORDS, device=DEV, dtype=torch.uint8)
    flat[nbytes:].view(torch.int32).fill_(_GUARD_PATTERN)

    def check():
        torch.cuda.synchronize()
        assert bool((flat[nbytes:].view(torch.int32) == _GUARD_PATTERN).all()), f"write behind a buffer of shape {shape}"

    return flat[:n * esz].view(dtype).view(*shape), check


@pytest.fixture
def engine_switch():
    old = nconv._CONV1X1
    yield lambda on: setattr(nconv, "_CONV1X1", bool(on))
    nconv._CONV1X1 = old


def operands(C, O, size, integer, seed):
    """x [B,H,W,C], gy [B,H,W,O], w [O,1,1,C], its transpose [C,1,O], residuals of both outputs; bf16 on the device."""
    B, H, W = size
    g = torch.Generator().manual_seed(seed)
    if integer:   # {-1, 0, 1} operands, residual in [-3, 3]: |sum| <= 512 * 1 is far from reached, every value a bf16
        mk = lambda *s: torch.randint(-1, 2, s, generator=g).float()
        rs = lambda *s: torch.randint(-3, 4, s, generator=g).float()
    else:
        mk = lambda *s: torch.randn(*s, generator=g)
        rs = mk
    x, gy = mk(B, H, W, C), mk(B, H, W, O)
    w = mk(O, 1, 1, C) * (1.0 if integer else C ** -0.5)
    t = dict(x=x, gy=gy, w=w, wt=w.reshape(O, C).t().reshape(C, 1, O), ry=rs(B, H, W, O), rx=rs(B, H, W, C))
    return {k: v.to(BF).contiguous().to(DEV) for k, v in t.items()}


def run_new(t, form, with_resid):
    """The new entry of `form` on a guarded output."""
    B, H, W, C = t["x"].shape
    O = t["gy"].shape[3]
    if form == "fwd":
        out, check = guarded_empty((B, H, W, O))
        N.call("dgv2_conv1x1_fwd", N.ptr(out), N.ptr(t["x"]), N.ptr(t["w"]), B, H * W, C, O,
               N.ptr(t["ry"] if with_resid else None), N.BF16, N.stream())
    else:
        out, check = guarded_empty((B, H, W, C))
        N.call("dgv2_conv1x1_dgrad", N.ptr(out), N.ptr(t["gy"]), N.ptr(t["wt"]), B, H * W, C, O,
               N.ptr(t["rx"] if with_resid else None), N.BF16, N.stream())
    check()
    return out


def run_routed(t, form, with_resid):
    """The same product through native.conv's routing (whichever engine the module flag selects)."""
    if form == "fwd":
        return nconv._conv_fwd_raw(t["x"], t["w"], GEOM, resid=t["ry"] if with_resid else None)
    return nconv._conv_dgrad_raw(t["gy"], None, GEOM, tuple(t["x"].shape), wt=t["wt"], resid=t["rx"] if with_resid else None)


def reference64(t, form, with_resid):
    """float64 on the CPU from the same bf16 values."""
    c = {k: v.double().cpu() for k, v in t.items()}
    O, C = c["w"].shape[0], c["w"].shape[3]
    w = c["w"].reshape(O, C)
    if form == "fwd":
        return c["x"] @ w.t() + (c["ry"] if with_resid else 0.0)
    return c["gy"] @ w + (c["rx"] if with_resid else 0.0)


CASES = [(C, O, s, r) for C, O in PAIRS for s in SIZES for r in (False, True)]
IDS = [f"{C}to{O}-B{s[0]}x{s[1]}x{s[2]}-{'resid' if r else 'bare'}" for C, O, s, r in CASES]


@pytest.mark.parametrize("form", ["fwd", "dgrad"])
@pytest.mark.parametrize("C,O,size,with_resid", CASES, ids=IDS)
def test_integer_operands_equal_direct_engine(C, O, size, with_resid, form, engine_switch):
    t = operands(C, O, size, True, 11)
    new = run_new(t, form, with_resid)
    engine_switch(True)
    routed = run_routed(t, form, with_resid)
    engine_switch(False)
    old = run_routed(t, form, with_resid)
    want = reference64(t, form, with_resid)
    assert float(want.abs().max()) <= 256     # every result a bf16 value: the comparison is exact
    assert torch.equal(old.double().cpu(), want), "the direct engine itself is off on exact data"
    assert torch.equal(new, old)
    assert torch.equal(routed, old)


@pytest.mark.parametrize("form", ["fwd", "dgrad"])
@pytest.mark.parametrize("C,O,size,with_resid", CASES, ids=IDS)
def test_random_operands_against_float64(C, O, size, with_resid, form, engine_switch):
    t = operands(C, O, size, False, 12)
    new = run_new(t, form, with_resid)
    engine_switch(False)
    old = run_routed(t, form, with_resid)
    want = reference64(t, form, with_resid)
    dev_new = float((new.double().cpu() - want).abs().max())
    dev_old = float((old.double().cpu() - want).abs().max())
    print(f"conv1x1 {form} {C}->{O} {size} resid={with_resid}: new {dev_new:.3e}, direct engine {dev_old:.3e}, "
          f"max |ref| {float(want.abs().max()):.3e}")
    assert dev_new <= 1.5 * dev_old + 1e-3 * float(want.abs().max())
    # stronger, and the reason a training step computes the same bits on either engine: the K-steps enter the same
    # instruction in the same operand order, and the residual joins the rounded product the way the direct engine adds it
    assert torch.equal(new, old)


def test_unsupported_shapes_fall_through():
    """DGV2_ENOTSUP (not an error, nothing written) for fp32, a channel count off the 32-grid and a contraction past 512."""
    x = torch.zeros(1, 2, 16, 1024, device=DEV, dtype=BF)
    y, check = guarded_empty((1, 2, 16, 64))
    y.fill_(7.0)
    args = lambda C, O, dt: (N.ptr(y), N.ptr(x), N.ptr(x), 1, 32, C, O, None, dt, N.stream())
    assert not N.try_call("dgv2_conv1x1_fwd", *args(32, 64, N.F32))
    assert not N.try_call("dgv2_conv1x1_fwd", *args(48, 64, N.BF16))
    assert not N.try_call("dgv2_conv1x1_fwd", *args(32, 48, N.BF16))
    assert not N.try_call("dgv2_conv1x1_fwd", *args(1024, 64, N.BF16))
    assert not N.try_call("dgv2_conv1x1_dgrad", *args(64, 1024, N.BF16))
    check()
    assert bool((y == 7.0).all())


def test_residual_block_routing(engine_switch):
    """ResidualBlock(64, 128) at B = 2, 8 x 64, forward + backward, flag on and off, against the block's float64 oracle."""
    from gans.models.dusty_v2 import ResidualBlock
    from oracle import model as o_model

    torch.manual_seed(5)
    blk = ResidualBlock(64, 128)
    with torch.no_grad():
        blk.bias_act1.bias.normal_(0, 0.1)
        blk.bias_act2.bias.normal_(0, 0.1)
    x0 = torch.randn(2, 64, 8, 64).to(BF)
    gy0 = torch.randn(2, 128, 4, 32).to(BF)
    names = [k for k, _ in blk.named_parameters()]

    sd64 = {k: v.detach().double().requires_grad_(k in names) for k, v in blk.state_dict().items()}
    x64 = x0.double().requires_grad_(True)
    y64 = o_model.residual_block(sd64, "", x64)
    (y64 * gy0.double()).sum().backward()
    want = {"y": y64.detach(), "x": x64.grad, **{k: sd64[k].grad for k in names}}

    blk = blk.to(DEV)
    N.status_read()
    got = {}
    for on in (True, False):
        engine_switch(on)
        blk.zero_grad(set_to_none=True)
        x = x0.to(DEV).requires_grad_(True)
        y = blk(x)
        (y.float() * gy0.to(DEV).float()).sum().backward()
        got[on] = {"y": y.detach(), "x": x.grad, **{k: p.grad for k, p in blk.named_parameters()}}
    assert N.status_read() == 0
    assert set(got[True]) == set(want)
    for k, ref in want.items():
        dev_new = float((got[True][k].double().cpu() - ref).abs().max())
        dev_old = float((got[False][k].double().cpu() - ref).abs().max())
        print(f"ResidualBlock(64,128) {k}: conv1x1 {dev_new:.3e}, direct engine {dev_old:.3e}, max |ref| {float(ref.abs().max()):.3e}")
        assert dev_new <= 1.5 * dev_old + 1e-3 * float(ref.abs().max()), k
