"""CPU side of tests/test_gpu_image_end.py: the float64 restatements the fp32 kernels at the two ends of the image path
are held to (generator output stage, ADA separable operator with arbitrary operators, range-image conversion at its
thresholds) and the builders of the test inputs.

Everything here runs without a GPU.  Each builder ASSERTS the conditioning its case relies on (margins around the discrete
decisions, coverage of the parameter values), on reference data alone; tests/test_image_end_cpu.py runs every builder.
Builders and references are cached: treat what they return as read-only.
"""
import functools
import math

import numpy as np
import torch

import ada_imgspace_ref as R
from oracle import coords as o_coords
from oracle import ops as o

TWO_PI = 2 * math.pi
F32 = np.float32


def rel_err(got, want):
    """max |got - want| / max |want|, the measure of tests/test_gpu_ada_imgspace.py."""
    return float((got.detach().double().cpu() - want.double()).abs().max() / (want.double().abs().max() + 1e-30))


def bound(dev32):
    """4 x the float32-vs-float64 deviation of the reference formula itself (another summation order on the device: the
    kernels chain up to H + K = 144 fp32 FMAs), floor 1e-5 (the suite's bound for fp32 elementwise ops)."""
    return max(4 * dev32, 1e-5)


# ---------------------------------------------------------------------------- 1. generator output stage
def ring_shift(v, shift):
    """oracle.ops.ring_shift in v's dtype: with float64 inputs the position, its floor and the fraction are float64 (the
    oracle pins the position to float32); with float32 inputs it is the oracle's formula bit for bit."""
    B, C, H, W = v.shape
    pos = torch.arange(W, dtype=v.dtype)[None, :] + (shift.to(v.dtype) / TWO_PI)[:, None] * W
    j0 = pos.floor()
    f = (pos - j0)[:, None, None, :]
    j0 = j0.long()
    i0 = (j0 % W)[:, None, None, :].expand(B, C, H, W)
    i1 = ((j0 + 1) % W)[:, None, None, :].expand(B, C, H, W)
    return v.gather(3, i0) * (1 - f) + v.gather(3, i1) * f


def gen_tail(skip, shift, u, out_scale, raydrop_const, temperature):
    """skip [B,2,H,W] -> (image, image_orig, logit, mask) in skip's dtype; mask is the straight-through form of
    oracle.ops.gumbel_sigmoid (value hard, gradient of the relaxed sample)."""
    v = skip if shift is None else ring_shift(skip, shift)
    v = v * out_scale
    img0 = torch.tanh(v[:, 0:1])
    logit = v[:, 1:2]
    img, mask = o.raydrop_measure(img0, logit, u.to(skip.dtype), raydrop_const, temperature)
    return img, img0, logit, mask


def shift_value(kind, W):
    """A shift whose position t = shift / (2 pi) * W has the stated integer part and a fraction well inside (0, 1)."""
    t = {"neg": -4.75, "small": 9.3, "neg_wrap": -(W + 2) + 0.7, "over": W + 3 + 0.37, "below": W - 0.4}.get(kind)
    return 0.0 if kind == "zero" else t / W * TWO_PI


# (B,H,W), temperature, raydrop_const, out_scale, per-sample shift kinds (None: shift=None).  Every temperature, constant
# and scale appears (each case checks all four outputs and all five cotangent sets); every shift kind appears; the last
# shape is more than one block row.
TAIL_CASES = [
    ((3, 6, 32), 1.0, -1.0, 0.25, ("zero", "neg", "over")),
    ((3, 6, 32), 0.5, 0.0, 1.0, None),
    ((2, 5, 33), 1.7, 0.37, 0.25, ("below", "neg_wrap")),
    ((2, 5, 33), 0.5, -1.0, 1.0, ("over", "zero")),
    ((1, 1, 7), 1.7, 0.0, 1.0, ("neg",)),
    ((1, 1, 7), 1.0, 0.37, 0.25, None),
    ((1, 1, 7), 0.5, -1.0, 0.25, ("below",)),
    ((2, 16, 1030), 0.5, 0.37, 0.25, ("neg", "over")),
    ((2, 16, 1030), 1.7, -1.0, 1.0, None),
    ((2, 16, 1030), 1.0, 0.0, 1.0, ("below", "zero")),
    ((2, 5, 33), 1.0, 0.0, 0.25, None),
    ((2, 16, 1030), 1.7, 0.37, 1.0, ("neg", "small")),   # more than one block row with |t| < 64: the tight adjoint identity
]
TAIL_OUTPUTS = ("image", "image_orig", "logit", "mask")
TAIL_COTANGENTS = ((0,), (1,), (2,), (3,), (0, 1, 2, 3))   # each output alone (the others None), then all four


def tail_id(i):
    (B, H, W), T, rc, s, kinds = TAIL_CASES[i]
    return f"{B}x{H}x{W}-T{T}-c{rc}-s{s}-" + ("noshift" if kinds is None else "+".join(kinds))


def _gumbel_argument(skip, shift, u, out_scale, temperature):
    _, _, logit, _ = gen_tail(skip.double(), shift, u.double(), out_scale, 0.0, temperature)
    ud = u.double()
    return (logit + ud.log() - (-ud).log1p()) / temperature


@functools.lru_cache(maxsize=None)
def tail_case(i):
    """fp32 CPU inputs of case i: skip [B,2,H,W], shift [B] or None, u, four independent cotangents."""
    (B, H, W), T, rc, s, kinds = TAIL_CASES[i]
    g = torch.Generator().manual_seed(100 + i)
    skip = torch.randn(B, 2, H, W, generator=g)
    u = torch.rand(B, 1, H, W, generator=g).clamp(1e-6, 1 - 1e-6)
    cot = tuple(torch.randn(B, 1, H, W, generator=g) for _ in range(4))
    shift = None
    if kinds is not None:
        assert len(kinds) == B
        shift = torch.tensor([shift_value(k, W) for k in kinds], dtype=torch.float32)
        # condition: the fraction of every non-zero position, in float64, is inside [0.01, 0.99] -- the split k is then
        # the same in fp32 and fp64
        t = shift.double() / TWO_PI * W
        frac = t - t.floor()
        for k, sv, fr in zip(kinds, shift.tolist(), frac.tolist()):
            assert (k == "zero" and sv == 0.0) or 0.01 <= fr <= 0.99, (k, sv, fr)
            assert {"zero": sv == 0.0, "neg": -TWO_PI < sv < 0, "small": 0 < sv < TWO_PI, "neg_wrap": sv < -TWO_PI, "over": TWO_PI < sv < 2 * TWO_PI,
                    "below": 0.9 * TWO_PI < sv < TWO_PI}[k], (k, sv)
    # condition: |(logit + log u - log1p(-u)) / temperature| >= 1e-3 at EVERY pixel (none is left out).  A pixel lands
    # inside the margin with probability about 5e-4 x temperature, so at 2 x 16 x 1030 pixels no seed clears them all
    # (some 16 to 56 expected); instead of searching seeds per shape, every case halves a uniform that lands inside twice
    # the margin, which moves the argument down by more than log 2 / temperature.  Still a fixed, seeded input.
    z = _gumbel_argument(skip, shift, u, s, T)
    u = torch.where(z.abs() < 2e-3, u * 0.5, u)
    z = _gumbel_argument(skip, shift, u, s, T)
    assert float(z.abs().min()) >= 1e-3, float(z.abs().min())
    assert float(u.min()) > 0 and float(u.max()) < 1
    return {"skip": skip, "shift": shift, "u": u, "cot": cot, "cfg": (s, rc, T)}


@functools.lru_cache(maxsize=None)
def tail_reference(i, dtype):
    """The four outputs and, per cotangent set, the gradient w.r.t. skip by autograd through the straight-through form."""
    c = tail_case(i)
    skip = c["skip"].to(dtype).requires_grad_(True)
    outs = gen_tail(skip, c["shift"], c["u"], *c["cfg"])
    grads = []
    for sel in TAIL_COTANGENTS:
        (gs,) = torch.autograd.grad([outs[k] for k in sel], skip, [c["cot"][k].to(dtype) for k in sel], retain_graph=True)
        grads.append(gs)
    return tuple(t.detach() for t in outs), tuple(grads)


def tail_max_position(i):
    """Largest |shift / (2 pi) * W| of case i, in columns (0 without a shift)."""
    shift = tail_case(i)["shift"]
    return 0.0 if shift is None else float((shift.double() / TWO_PI * TAIL_CASES[i][0][2]).abs().max())


def tail_jvp(i, v):
    """J v of the whole stage (all four outputs) in float64, v shaped like skip."""
    c = tail_case(i)
    fn = lambda s_: gen_tail(s_, c["shift"], c["u"], *c["cfg"])   # noqa: E731
    _, jv = torch.autograd.functional.jvp(fn, c["skip"].double(), v.double())
    return jv


# ---------------------------------------------------------------------------- 2. ADA apply with arbitrary operators
ADA_B = 3
# (entry point, H, K, W, flip sign per sample); the comment gives (kernel; qa; qb; W vs 64 + K - 1).  In csrc/ada.hip
# qa = sgn and qb = 1 forward, -sgn transposed, so three sign pairs exist: (+,+) and (-,+) forward, (+,-) and (-,+)
# transposed; (-,-) cannot occur.  Every case runs forward and transposed with both signs in the batch, so every case
# takes all three; which sample takes which is what the comment spells out.  "wrap": W < 64 + K - 1, the staged columns
# wrap round the ring inside one tile; "ragged": W % 64 != 0, the last tile is partial.
ADA_CASES = [
    # LDS kernel of dgv2_ada_apply: H in {4, 8, 20, 64} (rpt 1, 2, 5, 16), each with K = 64 at W = 24
    ("apply", 4, 64, 24, "+-+"),# (lds; qa +-+; qb +++ fwd, -+- adj; wrap: W < K)
    ("apply", 8, 64, 24, "-+-"),# (lds; qa -+-; qb +++ fwd, +-+ adj; wrap: W < K)            K = 64 side of the 64/65 boundary at (8, 24)
    ("apply", 20, 64, 24, "+-+"),# (lds; qa +-+; qb +++ fwd, -+- adj; wrap: W < K)
    ("apply", 64, 64, 24, "-+-"),# (lds; qa -+-; qb +++ fwd, +-+ adj; wrap: W < K)
    ("apply", 4, 1, 64, "+-+"), # (lds; qa +-+; qb +++ fwd, -+- adj; W = 64 + K - 1: one full tile, no wrap)
    ("apply", 8, 3, 100, "-+-"),# (lds; qa -+-; qb +++ fwd, +-+ adj; W > 64 + K - 1; ragged, W % 4 = 0)
    ("apply", 20, 24, 200, "+-+"),# (lds; qa +-+; qb +++ fwd, -+- adj; W > 64 + K - 1; four tiles, ragged)
    ("apply", 64, 24, 70, "-+-"),# (lds; qa -+-; qb +++ fwd, +-+ adj; wrap; ragged, W % 4 = 2)
    ("apply", 20, 3, 98, "+-+"),# (lds; qa +-+; qb +++ fwd, -+- adj; W > 64 + K - 1; ragged, W % 4 = 2)
    ("apply", 64, 1, 98, "-+-"),# (lds; qa -+-; qb +++ fwd, +-+ adj; W > 64 + K - 1; ragged, W % 4 = 2)
    ("apply", 8, 64, 100, "+-+"),# (lds; qa +-+; qb +++ fwd, -+- adj; wrap; ragged)           K = 64 side of the boundary at (8, 100)
    ("apply", 64, 64, 200, "-+-"),# (lds; qa -+-; qb +++ fwd, +-+ adj; W > 64 + K - 1; ragged)
    # generic kernel through dgv2_ada_apply: H % 4 != 0, H > 64, K > 64
    ("apply", 6, 64, 24, "+-+"),# (generic; qa +-+; qb +++ fwd, -+- adj; W < K)
    ("apply", 26, 64, 24, "-+-"),# (generic; qa -+-; qb +++ fwd, +-+ adj; W < K)
    ("apply", 68, 64, 24, "+-+"),# (generic; qa +-+; qb +++ fwd, -+- adj; W < K)
    ("apply", 6, 3, 100, "-+-"),# (generic; qa -+-; qb +++ fwd, +-+ adj; ragged)
    ("apply", 26, 24, 70, "+-+"),# (generic; qa +-+; qb +++ fwd, -+- adj; ragged, W % 4 = 2)
    ("apply", 68, 1, 200, "-+-"),# (generic; qa -+-; qb +++ fwd, +-+ adj; ragged)
    ("apply", 8, 65, 24, "+-+"),# (generic; qa +-+; qb +++ fwd, -+- adj; W < K)              K = 65 side of the boundary at (8, 24)
    ("apply", 8, 65, 100, "-+-"),# (generic; qa -+-; qb +++ fwd, +-+ adj; ragged)             K = 65 side of the boundary at (8, 100)
    # image-space LDS kernel of dgv2_ada_apply_img: H in {8, 24, 64}, each with K = 80 at W = 24
    ("img", 8, 80, 24, "+-+"),  # (img lds; qa +-+; qb +++ fwd, -+- adj; wrap: W < K)        K = 80 side of the 80/81 boundary at (8, 24)
    ("img", 24, 80, 24, "-+-"), # (img lds; qa -+-; qb +++ fwd, +-+ adj; wrap: W < K)
    ("img", 64, 80, 24, "+-+"), # (img lds; qa +-+; qb +++ fwd, -+- adj; wrap: W < K)
    ("img", 8, 1, 96, "-+-"),   # (img lds; qa -+-; qb +++ fwd, +-+ adj; W > 64 + K - 1; ragged)
    ("img", 24, 74, 100, "+-+"),# (img lds; qa +-+; qb +++ fwd, -+- adj; wrap; ragged)
    ("img", 64, 74, 98, "-+-"), # (img lds; qa -+-; qb +++ fwd, +-+ adj; wrap; ragged, W % 4 = 2)
    ("img", 8, 80, 96, "+-+"),  # (img lds; qa +-+; qb +++ fwd, -+- adj; wrap; ragged)       K = 80 side of the boundary at (8, 96)
    ("img", 64, 80, 100, "-+-"),# (img lds; qa -+-; qb +++ fwd, +-+ adj; wrap; ragged)
    # generic kernel through dgv2_ada_apply_img: K > 80, H % 4 != 0
    ("img", 8, 81, 24, "+-+"),  # (generic; qa +-+; qb +++ fwd, -+- adj; W < K)              K = 81 side of the boundary at (8, 24)
    ("img", 8, 81, 96, "-+-"),  # (generic; qa -+-; qb +++ fwd, +-+ adj; ragged)             K = 81 side of the boundary at (8, 96)
    ("img", 26, 74, 24, "+-+"), # (generic; qa +-+; qb +++ fwd, -+- adj; W < K)
    ("img", 26, 74, 100, "-+-"),# (generic; qa -+-; qb +++ fwd, +-+ adj; ragged)
]
OFF_KINDS = ("neg", "zero", "small", "over", "under")
CUT_KINDS = ("zero", "left_top", "right_bottom", "all", "interior")
CUT_BOXES = {"zero": (0.43, 0.57, 0.0, 0.0), "left_top": (0.05, 0.1, 0.5, 0.5), "right_bottom": (0.93, 0.9, 0.5, 0.4),
             "all": (0.4, 0.6, 2.0, 2.5), "interior": (0.5, 0.45, 0.3, 0.5)}


def ada_kernel(entry, H, K):
    """The kernel the dispatch of csrc/ada.hip picks (the switch DGV2_NO_ADA_LDS is never set in the suite)."""
    lds = H <= 64 and H % 4 == 0 and K <= (64 if entry == "apply" else 80)
    return ("lds" if entry == "apply" else "img_lds") if lds else "generic"


def ada_id(i):
    entry, H, K, W, _ = ADA_CASES[i]
    return f"{entry}-{ada_kernel(entry, H, K)}-H{H}-K{K}-W{W}"


def cut_edge_distance(cut, H, W):
    """Smallest distance, in image units, of a pixel centre to a box edge (per sample)."""
    cut = cut.double()
    dx = (((torch.arange(W) + 0.5) / W)[None] - cut[:, 0:1]).abs() - cut[:, 2:3] / 2
    dy = (((torch.arange(H) + 0.5) / H)[None] - cut[:, 1:2]).abs() - cut[:, 3:4] / 2
    return torch.minimum(dx.abs().min(dim=1).values, dy.abs().min(dim=1).values)


@functools.lru_cache(maxsize=None)
def ada_case(i):
    """fp32 / int32 CPU inputs of case i with arbitrary operators: dense Ay, signed asymmetric taps, both flip signs,
    offsets of every kind; for the image-space entry also sigma (one sample 0), eps and the cutout boxes."""
    entry, H, K, W, signs = ADA_CASES[i]
    B = ADA_B
    g = torch.Generator().manual_seed(1000 + i)
    x = torch.randn(B, 1, H, W, generator=g)
    Ay = torch.randn(B, H, H, generator=g)
    kx = torch.randn(B, K, generator=g)
    a, c = torch.randn(B, generator=g), torch.randn(B, generator=g)
    cot = torch.randn(B, 1, H, W, generator=g)
    sgn = torch.tensor([1 if ch == "+" else -1 for ch in signs], dtype=torch.int32)
    assert {int(s) for s in sgn} == {1, -1}
    kinds = [OFF_KINDS[(3 * i + b) % 5] for b in range(B)]
    off = torch.tensor([{"neg": -7, "zero": 0, "small": 5, "over": W + 13, "under": -W - 9}[k] for k in kinds],
                       dtype=torch.int32)
    case = {"x": x, "Ay": Ay, "kx": kx, "off": off, "sgn": sgn, "a": a, "c": c, "cot": cot, "off_kinds": kinds,
            "cut": None, "sigma": None, "eps": None, "cut_kinds": None}
    if entry == "img":
        # shifted against the offset kinds: an offset beyond +-W never meets the box that keeps nothing
        ck = [CUT_KINDS[(3 * i + b + 2) % 5] for b in range(B)]
        assert all(k != "all" for k, ok in zip(ck, kinds) if ok in ("over", "under"))
        cut = torch.tensor([CUT_BOXES[k] for k in ck], dtype=torch.float32)
        # condition: no pixel centre within 1e-4 of a box edge -- jitter the centre until twice that holds
        for _ in range(100):
            trial = cut.clone()
            trial[:, :2] += (torch.rand(B, 2, generator=g) - 0.5) * 0.02
            if float(cut_edge_distance(trial, H, W).min()) >= 2e-4:
                cut = trial
                break
        assert float(cut_edge_distance(cut, H, W).min()) >= 1e-4
        keep = R.cutout_mask(cut, H, W).mean(dim=(1, 2, 3)).tolist()
        for k, frac in zip(ck, keep):
            assert {"zero": frac == 1.0, "all": frac == 0.0}.get(k, 0.0 < frac < 1.0), (k, frac)
        sigma = torch.tensor([0.0, 0.3, 1.1], dtype=torch.float32).roll(i)
        assert float(sigma.min()) == 0.0 and float(sigma.max()) > 0
        case.update(cut=cut, sigma=sigma, eps=torch.randn(B, 1, H, W, generator=g), cut_kinds=ck)
    return case


@functools.lru_cache(maxsize=None)
def ada_operator(i):
    """Cx [B,W,W] in float64 from tests/ada_imgspace_ref.circulant."""
    c = ada_case(i)
    W = c["x"].shape[3]
    return torch.stack([R.circulant(c["kx"][b], int(c["off"][b]), int(c["sgn"][b]), W) for b in range(ADA_B)])


@functools.lru_cache(maxsize=None)
def ada_reference(i, dtype):
    """(forward, gradient for the cotangent, double backward) in `dtype`:
    y_b = mask_b (a_b Ay_b x_b Cx_b^T + c_b + sigma_b eps_b),  gx_b = a_b Ay_b^T (mask_b g_b) Cx_b,  the double backward
    is the forward without c and the noise (mask and sigma absent for dgv2_ada_apply)."""
    c = ada_case(i)
    _, _, H, W = c["x"].shape
    Cx, Ay, x, g = (t.to(dtype) for t in (ada_operator(i), c["Ay"], c["x"][:, 0], c["cot"][:, 0]))
    a, cc = c["a"].to(dtype)[:, None, None], c["c"].to(dtype)[:, None, None]
    lin = a * (Ay @ x @ Cx.transpose(1, 2))
    fwd = lin + cc
    mask = None
    if c["sigma"] is not None:
        fwd = fwd + c["sigma"].to(dtype)[:, None, None] * c["eps"][:, 0].to(dtype)
    if c["cut"] is not None:
        mask = R.cutout_mask(c["cut"], H, W)[:, 0].to(dtype)
        fwd, lin, g = fwd * mask, lin * mask, g * mask
    grad = a * (Ay.transpose(1, 2) @ g @ Cx)
    # condition: an offset beyond +-W is exercised only where something survives the cutout -- no all-zero expectation there
    for b, kind in enumerate(c["off_kinds"]):
        if kind in ("over", "under"):
            assert all(float(t[b].abs().max()) > 0 and float((t[b] != 0).double().mean()) > 0.25 for t in (fwd, grad, lin)), (b, kind)
    return fwd[:, None], grad[:, None], lin[:, None]


# ---------------------------------------------------------------------------- 3. coordinate conversion at the thresholds
MIN_DEPTH, MAX_DEPTH, TOL = 1.45, 80.0, 1e-11
COORD_SHAPE = (2, 1, 4, 16)


def _around(v):
    """(next fp32 below, v, next fp32 above) -> values, and which of them is the threshold itself."""
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))], [False, True, False]


def _layout(vals, flags, pad):
    """Two samples of 64 pixels: the list, padded with interior values, forwards and backwards."""
    n = COORD_SHAPE[2] * COORD_SHAPE[3]
    assert len(vals) <= n, len(vals)
    vals = np.array(list(vals) + list(pad[:n - len(vals)]), dtype=F32)
    flags = np.array(list(flags) + [False] * (n - len(flags)))
    return (np.stack([vals, vals[::-1]]).reshape(COORD_SHAPE).copy(),
            np.stack([flags, flags[::-1]]).reshape(COORD_SHAPE).copy())


@functools.lru_cache(maxsize=None)
def coords_inputs():
    """depth and normalised-inverse-depth images [2,1,4,16] holding every threshold of every mode with its two fp32
    neighbours, `thr` flags on the threshold pixels themselves, a 0/1 ray-drop mask and an angle grid.
    Two of the kernel's comparisons are implied by others at these depths and cannot be observed from outside: d > 0
    (mode 0) by d >= min_depth, and x > 1e-11 (mode 2) by inv >= 1 / max_depth.  Their triples are still run -- they pin
    that nothing but 0 comes out around them -- but a change of those two comparisons alone would not show."""
    mn, mx = F32(MIN_DEPTH), F32(MAX_DEPTH)
    vals, flags = [], []
    for t in (mn, mx, F32(0)):                      # d >= min, d <= max, d > 0
        v, f = _around(t)
        vals += v
        flags += f
    other = [-1.45, -80.0, -3.0, -1e-10, 1.5, 2.0, 10.0, 37.7, 79.5]     # negatives and interior values (not -1e-11:
    # the reference's 1 / (x + 1e-11) * valid is inf * 0 there)
    vals += [F32(v) for v in other]
    flags += [False] * len(other)
    depth, depth_thr = _layout(vals, flags, np.geomspace(1.6, 78.0, 64))
    # the images of those depths (0 where invalid), then the thresholds in the normalised inverse depth itself:
    # inv = x / min <= 1 / min at x = 1, inv >= 1 / max at x = min / max, inv > 0 at x = 0, x > 1e-11 (mode 2)
    img = o_coords.convert(np.array(vals, dtype=F32), "depth", "inv_depth_norm", MIN_DEPTH, MAX_DEPTH)
    ivals = [F32(v) for v in img if v != 0]
    iflags = [False] * len(ivals)
    for t in (F32(1), mn / mx, F32(MIN_DEPTH / MAX_DEPTH), F32(0), F32(TOL)):
        v, f = _around(t)
        ivals += v
        iflags += f
    other = [-1.0, -0.5, -1e-10, 0.5, 0.02, 0.99]
    ivals += [F32(v) for v in other]
    iflags += [False] * len(other)
    inv, inv_thr = _layout(ivals, iflags, np.geomspace(0.019, 0.98, 64))
    mask = np.ones(COORD_SHAPE, dtype=F32)
    mask[1, 0, :, ::2] = 0                                               # sample 1: every other pixel dropped
    rng = np.random.default_rng(7)
    angle = np.stack([rng.uniform(-0.4, 0.1, COORD_SHAPE[2:]), rng.uniform(-3.1, 3.1, COORD_SHAPE[2:])])[None].astype(F32)
    assert float(np.abs(np.sin(angle)).min()) > 1e-3 and float(np.abs(np.cos(angle)).min()) > 1e-3
    return {"depth": depth, "depth_thr": depth_thr, "inv": inv, "inv_thr": inv_thr, "mask": mask, "angle": angle}


def coords_valid64(x, mode):
    """The validity predicate of each mode evaluated in float64 on the fp32 input."""
    x = x.astype(np.float64)
    if mode == 0:
        return (x >= MIN_DEPTH) & (x <= MAX_DEPTH) & (x > 0)
    inv = x / MIN_DEPTH
    ok = (inv >= 1 / MAX_DEPTH) & (inv <= 1 / MIN_DEPTH) & (inv > 0)
    return ok & (x > TOL) if mode == 2 else ok


def coords_case(mode, with_mask=False, raydrop_const=-1.0):
    """-> (input, oracle output, compare): `compare` is False on a threshold pixel whose fp32 predicate (the oracle's) and
    float64 predicate disagree -- only ever the threshold pixel itself, never a neighbour (asserted)."""
    d = coords_inputs()
    x = d["depth"] if mode == 0 else d["inv"]
    thr = d["depth_thr"] if mode == 0 else d["inv_thr"]
    if mode == 0:
        plain = o_coords.convert(x, "depth", "inv_depth_norm", MIN_DEPTH, MAX_DEPTH)
        want = o_coords.fetch_reals(x, d["mask"], MIN_DEPTH, MAX_DEPTH, raydrop_const) if with_mask else plain
    elif mode == 1:
        want = plain = o_coords.convert(x, "inv_depth_norm", "depth", MIN_DEPTH, MAX_DEPTH)
    else:
        want = o_coords.convert(x, "inv_depth_norm", "point_map", MIN_DEPTH, MAX_DEPTH, angle=d["angle"])
        plain = np.abs(want).max(axis=1, keepdims=True)
    valid32 = plain != 0
    ambiguous = valid32 != coords_valid64(x, mode)
    assert not (ambiguous & ~thr).any(), "a neighbour of a threshold is ambiguous"
    assert valid32.any() and (~valid32).any()
    return x, want.astype(F32), ~ambiguous
