"""LiDAR beam upsampling, the paper's second application: hold out beams of a dense scan (every `factor`-th row stays),
reconstruct them -- by the interpolation baselines or by fitting a trained generator to the sparse scan -- and score the
held-out pixels with the depth errors and threshold accuracies of gans/metrics/depth.py.  The reference ships the
scoring file and no caller of it; nothing there holds beams out or interpolates them.

The masks and the baselines are one launch (native.beam_split), the scores one launch of fixed-order float64 sums
(native.depth_score); the generator fit is gans.sim2real.LatentFitter as the caller built it.  Nothing here reads a
value back to the host except UpsamplingBenchmark.summary(), once.  Out of scope: bicubic interpolation, 3-D metrics on
the reconstructed cloud, pivotal tuning (gans.inversion.invert remains the tool for a single scan), sharding the scan
list over GPUs."""
import torch

from .models.ops import native

__all__ = ["METHODS", "upsample_scans", "score_upsampling", "UpsamplingBenchmark"]

METHODS = ("nearest", "linear", "gan")


def upsample_scans(depth, valid, *, factor=4, offset=0, method, fitter=None):
    """depth, valid [b,1,H,W] (metric depth, validity; valid may be None) -> {"depth", "mask", "obs", "held"}, all
    [b,1,H,W] float32: the reconstruction from the rows h % factor == offset alone and where it holds a value, the
    fitting mask (observed and valid) and the scoring mask (valid, not observed).
    method "nearest" / "linear": one native.beam_split call.  method "gan": `fitter` (a gans.sim2real.LatentFitter, used
    as it is: its batch size, steps and graph setting are the caller's) is fitted to depth * obs under obs; the depth is
    its inv_depth_orig converted back to metres and the mask is raydrop_prob >= 0.5."""
    if method not in METHODS:
        raise ValueError(f"upsample_scans: method must be one of {METHODS}, got {method!r}")
    if method == "gan":
        if fitter is None:
            raise ValueError("upsample_scans: method 'gan' needs a fitter (gans.sim2real.LatentFitter)")
        split = native.beam_split(depth, valid, factor, offset, mode="none")
        obs = split["obs"]
        out = fitter.fit(depth * obs, obs)
        coord = fitter.coord
        with torch.no_grad():
            rec = coord.convert(coord.convert(out["inv_depth_orig"], "inv_depth_norm", "depth_norm"), "depth_norm", "depth")
            mask = (out["raydrop_prob"] >= 0.5).float()
        return {"depth": rec, "mask": mask, "obs": obs, "held": split["held"]}
    split = native.beam_split(depth, valid, factor, offset, mode=method)
    return {"depth": split["recon"], "mask": split["recon_mask"], "obs": split["obs"], "held": split["held"]}


def score_upsampling(depth_ref, depth_gen, held):
    """native.depth_score sums [b,8] of the reconstruction over the held-out pixels; they stay on the device."""
    return native.depth_score(depth_ref, depth_gen, held)


class UpsamplingBenchmark:
    """Runs `methods` over batches of dense scans and keeps, per method and on the device, one float64 [8] total of the
    depth_score sums (the pooled pixels) beside the sums of the per-scan summaries and the coverage counts.

    update(depth, valid, fitter=None) adds a batch with no host readback and returns the batch's sums per method;
    summary() makes one readback and returns per method {"per_scan": the seven metrics as means of per-scan values (the
    reference's convention; a scan without a held-out pixel has no value and is not counted), "pooled": the same seven
    over all held-out pixels together, "coverage": the share of held-out pixels whose reconstruction mask is 1, "scans",
    "scored_scans", "pixels"}."""

    def __init__(self, methods=("nearest", "linear"), factor=4, offset=0):
        methods = tuple(methods)
        if not methods or len(set(methods)) != len(methods) or any(m not in METHODS for m in methods):
            raise ValueError(f"UpsamplingBenchmark: methods must be distinct names out of {METHODS}, got {methods}")
        if int(factor) < 1 or not 0 <= int(offset) < int(factor):
            raise ValueError(f"UpsamplingBenchmark: need factor >= 1 and 0 <= offset < factor, got {factor}, {offset}")
        self.methods, self.factor, self.offset = methods, int(factor), int(offset)
        self._state = None   # float64 [len(methods), 3, 8] on the scans' device: pooled sums / per-scan sums / coverage

    def update(self, depth, valid, fitter=None):
        if "gan" in self.methods and fitter is None:
            raise ValueError("UpsamplingBenchmark.update: method 'gan' needs a fitter")
        if self._state is None:
            self._state = torch.zeros(len(self.methods), 3, 8, device=depth.device, dtype=torch.float64)
        batch = {}
        for i, method in enumerate(self.methods):
            out = upsample_scans(depth, valid, factor=self.factor, offset=self.offset, method=method, fitter=fitter)
            sums = score_upsampling(depth, out["depth"], out["held"])
            with torch.no_grad():
                scored = sums[:, 7] > 0
                per_scan = torch.stack(list(native.depth_summary(sums).values()), dim=1)       # [b,7], NaN where not scored
                per_scan = torch.where(scored[:, None], per_scan, torch.zeros_like(per_scan)).sum(dim=0)
                held = out["held"]
                row = self._state[i]
                row[0] += sums.sum(dim=0)
                row[1, :7] += per_scan
                row[1, 7] += scored.sum()
                row[2, 0] += (held * out["mask"]).sum(dtype=torch.float64)
                row[2, 1] += held.sum(dtype=torch.float64)
                row[2, 2] += len(depth)
            batch[method] = sums
        return batch

    def summary(self):
        if self._state is None:
            raise RuntimeError("UpsamplingBenchmark.summary: no batch was added")
        state = self._state.cpu()   # the one readback
        result = {}
        for i, method in enumerate(self.methods):
            pooled, per_scan, cover = state[i]
            n = per_scan[7]
            result[method] = {
                "per_scan": {k: float(per_scan[j] / n) for j, k in enumerate(native.DEPTH_KEYS)},
                "pooled": {k: float(v) for k, v in native.depth_summary(pooled).items()},
                "coverage": float(cover[0] / cover[1]),
                "scans": int(cover[2]), "scored_scans": int(n), "pixels": float(pooled[7]),
            }
        return result
