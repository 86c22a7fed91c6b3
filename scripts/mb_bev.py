"""The bird's-eye-view splat as three native launches (csrc/bev.hip) against the same arithmetic as tensor ops
(tests/bev_ref.py in float32) on the same device.

    python scripts/mb_bev.py [--window 1.0] [--rounds 5] [--out profiles/bev_mb.txt]

Shape: B = 8 range images of 64 x 512 points (a synthetic scene through CoordBridge, 10 % dropped rays), normal colours,
size 512, t = (0, 0, 0.7) -- the "pointcloud" panel of train_gan.py at the full configuration.  Variants, alternating
within one process: `entry` (native.bev_render: clear, splat, resolve), `public` (gans.render.render_point_clouds: the
entry plus the power-of-two colour scaling around it) and `tensor_ops` (the restatement).  Each timed window is about
`--window` seconds of calls (the count per variant is fixed after the warm-up from a short trial and reported) ending
in a device synchronise; the figure reported is the minimum per call over the rounds, with the rounds beside it.
Launches are counted and kernel times taken with torch.profiler (not rocprofv3) in a pass of its own, in this
process.  $DGV2_LIB_PATH measures another build of the library (an experiment variant of the splat).  The splat's atomic
traffic (8 bytes per add, counted from the restatement's corner masks) is set against its profiled kernel time.  Prints
one JSON line per variant and writes the same lines to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dusty-gan-v2_amd"), os.path.join(ROOT, "tests")]
B, H, W, SIZE = 8, 64, 512, 512
DEV = "cuda"


def kernels(fn):
    import torch
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [(e.name[:96], round(e.time_range.elapsed_us(), 1)) for e in prof.events() if e.device_type == DeviceType.CUDA]


def window(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def time_rounds(fns, seconds, rounds):
    """({variant: [us per call, per round]}, {variant: calls per window})"""
    for fn in fns.values():
        window(fn, 10)
    iters = {k: max(20, int(seconds / window(fn, 20))) for k, fn in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, iters[k]) * 1e6)
    return times, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "bev_mb.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mb_bev: needs the GPU (no CPU path)")
    import bev_ref
    from gans.coords import CoordBridge, synthetic_angle_grid
    from gans.models.ops import native
    from gans.render import render_point_clouds
    from gans.utils import points_to_normal_2d
    torch.set_grad_enabled(False)

    g = torch.Generator().manual_seed(0)
    azim = torch.linspace(0, 2 * torch.pi, W)[None, None, None]
    depth = 20.0 + 12.0 * torch.sin(3 * azim + torch.rand(B, 1, 1, 1, generator=g) * 6.28) + 3.0 * torch.rand(B, 1, H, W, generator=g)
    inv = 1.45 / depth
    inv[torch.rand(inv.shape, generator=g) < 0.1] = 0.0
    bridge = CoordBridge(H, W, 1.45, 80.0, angle_array=synthetic_angle_grid(H)).to(DEV)
    points_map = bridge.convert(inv.to(DEV), "inv_depth_norm", "point_map") / 80.0
    points = points_map.flatten(2).transpose(1, 2).contiguous()
    colors = points_to_normal_2d(points_map, mode="closest").flatten(2).transpose(1, 2).contiguous()
    t = torch.tensor([0.0, 0.0, 0.7], device=DEV)

    fns = {"entry": lambda: native.bev_render(points, colors, SIZE, None, t, 1.0),
           "public": lambda: render_point_clouds(points, colors, size=SIZE, t=t),
           "tensor_ops": lambda: bev_ref.render(points, colors, SIZE, None, t, 1.0, dtype=torch.float32)}
    outs = {k: fn() for k, fn in fns.items()}
    geo = bev_ref.project(points, SIZE, None, t, 1.0)
    adds = sum(int(ok.sum()) + colors.shape[-1] * int((ok & geo["keep"]).sum())
               for _, _, _, ok, _ in bev_ref.corners(geo["row"], geo["col"], SIZE, SIZE))
    times, iters = time_rounds(fns, args.window, args.rounds)
    lines = []
    for k, fn in fns.items():
        names = kernels(fn)
        rec = {"bench": "bev", "variant": k, "shape": {"B": B, "N": H * W, "C": int(colors.shape[-1]), "size": SIZE},
               "library": os.path.relpath(native.N.LIB_PATH, ROOT), "calls_per_window": iters[k],
               "us_per_call_rounds": [round(v, 1) for v in times[k]], "us_per_call_min": round(min(times[k]), 1),
               "launches_per_call": len(names), "device_us_profiled_call": round(sum(v for _, v in names), 1),
               "bit_identical_on_rerun": bool(torch.equal(outs[k], fn())),
               "max_abs_diff_to_tensor_ops": float((outs[k] - outs["tensor_ops"]).abs().max())}
        if k != "tensor_ops":
            rec["speedup_over_tensor_ops"] = round(min(times["tensor_ops"]) / min(times[k]), 2)
            rec["kernels_us"] = names
        if k == "entry":
            splat_us = sum(v for n, v in names if "splat" in n)
            rec.update(atomic_adds=adds, atomic_bytes=8 * adds,
                       splat_atomic_GBps=round(8 * adds / (splat_us * 1e-6) / 1e9, 1) if splat_us else None)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
