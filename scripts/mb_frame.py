"""Post-processing of a batch of 3-D frames of a latent walk at 64 x 512: launches and wall time of
  * `fused`: the one launch (native.frame_points);
  * `composed`: the same result from the project's own ops -- tanh_to_sigmoid, convert to a point map, a 3x3 median
    from F.unfold + sort, / max_depth, convert to a normal map, (n + 1) / 2, two rearranges (kept here for the
    comparison only -- the walk has no such path);
  * `frame_batch`: a whole batch of the walk, generator forward + the one launch (gans.interpolation.interpolate).

    python scripts/mb_frame.py [--batches 8 32] [--iters 200] [--rounds 3]

fused and composed alternate within one process (rounds), each window ends in a device synchronise; launches are
counted with torch.profiler in a pass of its own.  Prints one JSON line per (batch, variant)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dusty-gan-v2_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gans.config import load_config  # noqa: E402
from gans.coords import CoordBridge, synthetic_angle_grid  # noqa: E402
from gans.interpolation import LatentPath, interpolate, sample_anchors  # noqa: E402
from gans.models.builder import build_generator  # noqa: E402
from gans.models.ops import native  # noqa: E402
from gans.utils import tanh_to_sigmoid  # noqa: E402

DEV = "cuda"


def composed(coord, image):
    pm = coord.convert(tanh_to_sigmoid(image), "inv_depth_norm", "point_map")
    B, C, H, W = pm.shape
    med = F.unfold(pm, 3, padding=1).view(B, C, 9, H, W).sort(dim=2).values[:, :, 4]
    points = med / coord.max_depth
    colors = (coord.convert(med, "point_map", "normal_map") + 1) / 2
    return points.flatten(2).permute(0, 2, 1).contiguous(), colors.flatten(2).permute(0, 2, 1).contiguous()


def launches(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_frame: needs the GPU (no CPU path)")
    cfg = load_config()
    torch.manual_seed(0)
    G = build_generator(cfg.model.generator).to(DEV).eval().requires_grad_(False)
    coord = CoordBridge(64, 512, 1.45, 80.0, angle_array=synthetic_angle_grid(64)).to(DEV)
    path = LatentPath(sample_anchors(G, 4))
    u = native.gumbel_uniform((1, 1, 64, 512), DEV)
    for B in args.batches:
        steps = path.steps(B)[:B]
        with torch.no_grad():
            image = G(z=path(steps).float(), angle=coord.angle, truncation_psi=0.7, input_w=True,
                      noise={"gumbel_u": u.expand(B, 1, 64, 512)})["image"]
        fns = {"fused": lambda: native.frame_points(image, coord.angle, coord.min_depth, coord.max_depth, "zeros"),
               "composed": lambda: composed(coord, image),
               "frame_batch": lambda: list(interpolate(G, coord, path, steps, mode="3d", batch=B, u=u))}
        same = all(torch.equal(a, b) for a, b in zip(fns["fused"](), fns["composed"]()))
        iters = {k: (args.iters if k != "frame_batch" else max(10, args.iters // 10)) for k in fns}
        for k, fn in fns.items():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters[k]):
                    fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / iters[k] * 1e6)
        for k, fn in fns.items():
            print(json.dumps({"bench": "frame_points", "variant": k, "batch": B, "us_per_call_rounds": [round(t, 1) for t in times[k]],
                              "us_per_call_min": round(min(times[k]), 1), "launches_per_call": launches(fn),
                              "fused_equals_composed": same}), flush=True)


if __name__ == "__main__":
    main()
