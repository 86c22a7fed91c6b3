"""native.upsample: beam hold-out with the interpolation baselines (dgv2_beam_split) and the depth scores of
gans/metrics/depth.py (reference: gans/metrics/depth.py:4-45) as fixed-order float64 sums (dgv2_depth_score).
include/dgv2.h, "Beam upsampling", states the arithmetic, DESIGN.md section 41 the kernels.

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI, see the package docstring).  Forward only, float32
in, no gradient is recorded; one launch per call.  Nothing is converted on the way in: a CPU tensor, another dtype, a
non-contiguous tensor or mismatched shapes raise before the library is called.
"""
import torch

import dgv2_native as N

BEAM_MODES = {"none": 0, "nearest": 1, "linear": 2}
DEPTH_SUMS = ("abs_rel", "sq_rel", "sq", "sq_log", "accuracy_1", "accuracy_2", "accuracy_3", "count")   # columns of depth_score
DEPTH_KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "accuracy_1", "accuracy_2", "accuracy_3")
DEPTH_N_MAX = 2 ** 31   # exclusive


def _f32(what, name, t, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: {name} must be a CUDA/HIP tensor (no CPU fallback)")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous")
    return t.detach()


def beam_split(depth, valid, factor, offset=0, mode="none"):
    """depth [B,1,H,W], valid the same or None (all valid) -> {"obs", "held"} and, for mode "nearest" / "linear",
    {"recon", "recon_mask"}: row h is observed when h % factor == offset; obs = observed and valid, held = valid and not
    observed, recon the interpolation of the observed rows (dgv2_beam_split).  All float32 [B,1,H,W]."""
    if mode not in BEAM_MODES:
        raise ValueError(f"beam_split: mode must be one of {sorted(BEAM_MODES)}, got {mode!r}")
    if not isinstance(depth, torch.Tensor) or depth.ndim != 4 or depth.shape[1] != 1:
        raise ValueError(f"beam_split: depth must be [B,1,H,W], got {tuple(getattr(depth, 'shape', ()))}")
    depth = _f32("beam_split", "depth", depth)
    valid = None if valid is None else _f32("beam_split", "valid", valid, depth.shape)
    if valid is not None and valid.device != depth.device:
        raise ValueError(f"beam_split: depth is on {depth.device}, valid on {valid.device}")
    B, _, H, W = depth.shape
    factor, offset = int(factor), int(offset)
    if min(B, H, W) < 1:
        raise ValueError(f"beam_split: empty input {tuple(depth.shape)}")
    if not 1 <= factor <= H:
        raise ValueError(f"beam_split: factor {factor} is outside 1 .. H = {H}")
    if not 0 <= offset < factor:
        raise ValueError(f"beam_split: offset {offset} is outside 0 .. factor - 1 = {factor - 1}")
    out = {"obs": torch.empty_like(depth), "held": torch.empty_like(depth)}
    if mode != "none":
        out["recon"], out["recon_mask"] = torch.empty_like(depth), torch.empty_like(depth)
    with torch.cuda.device(depth.device):
        N.call("dgv2_beam_split", N.ptr(out.get("recon")), N.ptr(out.get("recon_mask")), N.ptr(out["obs"]), N.ptr(out["held"]),
               N.ptr(depth), N.ptr(valid), B, H, W, factor, offset, BEAM_MODES[mode], N.stream())
    return out


def depth_score(ref, gen, mask=None):
    """ref, gen [B,...], mask the same or None (all ones; a weight, as in the reference) -> float64 [B,8]: per image the
    sums of mask * (abs_rel, sq_rel, squared, squared-log error, accuracy 1..3 indicator) and of mask, every term in
    float32 as gans/metrics/depth.py computes it, summed in float64 in a fixed order (dgv2_depth_score); a pixel whose
    mask is 0 is skipped.  depth_summary turns the sums into the reference's seven values."""
    if not isinstance(ref, torch.Tensor) or ref.ndim < 1:
        raise ValueError(f"depth_score: ref must be [B,...], got {tuple(getattr(ref, 'shape', ()))}")
    ref = _f32("depth_score", "ref", ref)
    gen = _f32("depth_score", "gen", gen, ref.shape)
    mask = None if mask is None else _f32("depth_score", "mask", mask, ref.shape)
    if any(t is not None and t.device != ref.device for t in (gen, mask)):
        raise ValueError("depth_score: ref, gen and mask must be on one device")
    B = ref.shape[0]
    n = ref.numel() // B if B else 0
    if B < 1 or n < 1:
        raise ValueError(f"depth_score: empty input {tuple(ref.shape)}")
    if n >= DEPTH_N_MAX:
        raise ValueError(f"depth_score: {n} pixels per image; the kernel takes fewer than {DEPTH_N_MAX}")
    sums = torch.empty(B, len(DEPTH_SUMS), device=ref.device, dtype=torch.float64)
    with torch.cuda.device(ref.device):
        N.call("dgv2_depth_score", N.ptr(sums), N.ptr(ref), N.ptr(gen), N.ptr(mask), B, n, N.stream())
    return sums


def depth_summary(sums):
    """sums [..., 8] (depth_score's, or rows of it added up) -> the seven values of compute_depth_error /
    compute_depth_accuracy as float64 [...]: the first seven sums over the count, a square root on rmse and rmse_log.
    A zero count gives NaN, as the reference's 0 / 0 does.  Tensor ops on whatever device `sums` is on."""
    if not isinstance(sums, torch.Tensor) or sums.ndim < 1 or sums.shape[-1] != len(DEPTH_SUMS):
        raise ValueError(f"depth_summary: sums must be [..., {len(DEPTH_SUMS)}], got {tuple(getattr(sums, 'shape', ()))}")
    mean = sums[..., :7].double() / sums[..., 7:].double()
    return {k: (mean[..., i].sqrt() if k in ("rmse", "rmse_log") else mean[..., i]) for i, k in enumerate(DEPTH_KEYS)}


__all__ = ["beam_split", "depth_score", "depth_summary", "BEAM_MODES", "DEPTH_SUMS", "DEPTH_KEYS", "DEPTH_N_MAX"]
