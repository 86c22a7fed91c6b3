"""CPU restatements of include/dgv2.h "Beam upsampling", shared by tests/test_upsampling_cpu.py and
tests/test_gpu_upsampling.py: the depth scores with float32 terms from separately rounded torch ops and a float64 sum,
the same scores entirely in float64 (the oracle), the beam split by an explicit list of the observed rows, and the
seeded inputs of the score tests."""
import torch

KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "accuracy_1", "accuracy_2", "accuracy_3")
THRESHOLDS = (1.25, 1.5625, 1.953125)
SEEDS = (100, 101, 102, 103)
SHAPES = ((3, 1, 5, 7), (2, 1, 16, 64), (1, 1, 64, 512), (2, 1, 3, 43))


def make_inputs(seed, shape):
    """(ref, gen, mask) float32: depths in the sensor's range, a generated scan within a factor 0.2 .. 3 of it, about
    20 % of the pixels masked out."""
    g = torch.Generator().manual_seed(seed)
    ref = torch.rand(shape, generator=g) * 78.55 + 1.45
    gen = ref * (1 + 0.3 * torch.randn(shape, generator=g)).clamp(0.2, 3)
    mask = (torch.rand(shape, generator=g) > 0.2).float()
    return ref, gen, mask


def threshold_margin(ref, gen):
    """The smallest relative distance of a pixel's float64 delta from one of the three thresholds."""
    r, g = ref.double(), gen.double()
    delta = torch.max(r / g, g / r)
    return min(float(((delta - t).abs() / t).min()) for t in THRESHOLDS)


def score_sums_f32(ref, gen, mask=None):
    """The contract of dgv2_depth_score: every term and every product with the weight in float32, each operation a torch
    op of its own (one rounding each), the sums in float64; a pixel with weight 0 adds nothing.  -> float64 [B,8]"""
    assert ref.dtype == gen.dtype == torch.float32 and not ref.is_cuda
    m = torch.ones_like(ref) if mask is None else mask
    r, g = ref + 1e-8, gen + 1e-8
    d = r - g
    dd = d * d
    lg = r.log() - g.log()
    delta = torch.max(ref / gen, gen / ref)
    terms = [d.abs() / r, dd / r, dd, lg * lg] + [(delta < t).float() for t in THRESHOLDS] + [torch.ones_like(ref)]
    B = ref.shape[0]
    cols = [torch.where(m != 0, m * t, torch.zeros_like(t)).double().reshape(B, -1).sum(dim=1) for t in terms]
    return torch.stack(cols, dim=1)


def summary_f64(ref, gen, mask=None):
    """The reference's formulas (gans/metrics/depth.py:4-45) on the float32 inputs, entirely in float64 -> {key: [B]}"""
    ref, gen = ref.double(), gen.double()
    m = torch.ones_like(ref) if mask is None else mask.double()
    B = ref.shape[0]

    def mean(v):
        return (v * m).reshape(B, -1).sum(dim=1) / m.reshape(B, -1).sum(dim=1)
    r, g = ref + 1e-8, gen + 1e-8
    d = r - g
    delta = torch.max(ref / gen, gen / ref)
    out = {"abs_rel": mean(d.abs() / r), "sq_rel": mean(d ** 2 / r), "rmse": mean(d ** 2).sqrt(),
           "rmse_log": mean((r.log() - g.log()) ** 2).sqrt()}
    out.update({f"accuracy_{i + 1}": mean((delta < t).double()) for i, t in enumerate(THRESHOLDS)})
    return out


def make_scan(seed, B, H, W, factor, offset):
    """(depth, valid) float32 [B,1,H,W]: about 30 % of the pixels invalid, column 1 % W invalid in EVERY observed row (a
    pixel with no valid neighbour at all), a few valid pixels marked by a value other than 1."""
    g = torch.Generator().manual_seed(seed)
    depth = torch.rand(B, 1, H, W, generator=g) * 78.55 + 1.45
    valid = (torch.rand(B, 1, H, W, generator=g) > 0.3).float()
    valid[:, :, offset::factor, 1 % W] = 0.0
    other = (torch.rand(B, 1, H, W, generator=g) > 0.8) & (valid != 0)
    valid[other] = 0.5
    valid[0, 0, 0, 0] = -2.0
    return depth, valid


def beam_split_ref(depth, valid, factor, offset, mode):
    """The rules of dgv2_beam_split in float32 torch ops, row by row from the list of observed rows."""
    assert depth.dtype == torch.float32 and mode in ("none", "nearest", "linear")
    B, _, H, W = depth.shape
    v = torch.ones(B, 1, H, W, dtype=torch.bool) if valid is None else valid != 0
    observed = [h for h in range(H) if h % factor == offset]
    seen = torch.zeros(H, dtype=torch.bool)
    seen[observed] = True
    seen = seen[None, None, :, None]
    out = {"obs": (v & seen).float(), "held": (v & ~seen).float()}
    if mode == "none":
        return out
    recon, rmask = torch.zeros_like(depth), torch.zeros_like(depth)
    zero, no = torch.zeros(B, W), torch.zeros(B, W, dtype=torch.bool)
    for h in range(H):
        lo = max((o for o in observed if o <= h), default=None)
        hi = min((o for o in observed if o >= h), default=None)
        d_lo, v_lo = (depth[:, 0, lo], v[:, 0, lo]) if lo is not None else (zero, no)
        d_hi, v_hi = (depth[:, 0, hi], v[:, 0, hi]) if hi is not None else (zero, no)
        if mode == "linear":
            both = zero
            if lo is not None and hi is not None:
                t = torch.tensor(float(h - lo), dtype=torch.float32) / torch.tensor(float(factor), dtype=torch.float32)
                diff = d_hi - d_lo
                step = t * diff
                both = d_lo if lo == hi else d_lo + step
            val = torch.where(v_lo & v_hi, both, torch.where(v_lo, d_lo, torch.where(v_hi, d_hi, zero)))
        else:
            lo_first = lo is not None and (hi is None or h - lo <= hi - h)
            (d1, v1), (d2, v2) = ((d_lo, v_lo), (d_hi, v_hi)) if lo_first else ((d_hi, v_hi), (d_lo, v_lo))
            val = torch.where(v1, d1, torch.where(v2, d2, zero))
        recon[:, 0, h] = val
        rmask[:, 0, h] = (v_lo | v_hi).float()
    out["recon"], out["recon_mask"] = recon, rmask
    return out
