"""One EMD distance matrix of the COV / MMD / 1-NNA protocol two ways: the match-free all-pairs kernel
(pairwise_emd_cost, csrc/pointcloud.hip) against the batched row x chunk loop it stands in for
(_pairwise_distance(..., 256, ("emd",)): approxmatch + matchcost per (row, chunk of 256)).

    python scripts/mb_emd_pairwise.py [--rows 64] [--cols 256] [--points 2048] [--rounds 3]

The matrix is [rows, cols] at `points` points per cloud.  The two paths alternate within one process; a timed window is
one whole matrix ending in a device synchronise; reported are the rounds and their minimum, the device time and the
launches of one profiled call of each (torch.profiler, a pass of its own), the worst relative difference of the two
matrices, and the time of the protocol's three 2048 x 2048 matrices EXTRAPOLATED from the minimum by the pair count.
Prints one JSON line per path."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dusty-gan-v2_amd")]
DEV = "cuda"
PROTOCOL_PAIRS = 3 * 2048 * 2048


def kernels(fn):
    import torch
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [(e.name, e.time_range.elapsed_us()) for e in prof.events() if e.device_type == DeviceType.CUDA]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--cols", type=int, default=256)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    from gans.metrics.cov_mmd_1nna import _pairwise_distance
    from gans.metrics.distance.emd.earth_mover_distance import pairwise_emd_cost
    if not torch.cuda.is_available():
        raise SystemExit("mb_emd_pairwise: needs the GPU (no CPU path)")
    torch.set_grad_enabled(False)
    g = torch.Generator().manual_seed(0)
    a = (torch.randn(args.rows, args.points, 3, generator=g) * 0.4).to(DEV)
    b = (torch.randn(args.cols, args.points, 3, generator=g) * 0.4).to(DEV)
    fns = {"pairwise": lambda: pairwise_emd_cost(a, b) / float(args.points),
           "batched": lambda: _pairwise_distance(a, b, 256, ("emd",), False)["emd"]}
    small = {"pairwise": lambda: pairwise_emd_cost(a[:2], b[:2]), "batched": lambda: _pairwise_distance(a[:2], b[:2], 256, ("emd",), False)}
    for fn in small.values():   # warm-up: code objects loaded, allocator primed
        fn()
    torch.cuda.synchronize()
    out = {k: fn() for k, fn in fns.items()}
    torch.cuda.synchronize()
    diff = float(((out["pairwise"] - out["batched"]).abs() / out["batched"]).max())
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    pairs = args.rows * args.cols
    for k, fn in fns.items():
        names = kernels(fn)
        best = min(times[k])
        rec = {"bench": "emd_pairwise", "variant": k, "matrix": [args.rows, args.cols], "points": args.points,
               "ms_per_matrix_rounds": [round(t * 1e3, 1) for t in times[k]], "ms_per_matrix_min": round(best * 1e3, 1),
               "spread_ms": round((max(times[k]) - best) * 1e3, 1), "launches_per_matrix": len(names),
               "device_ms_profiled_call": round(sum(t for _, t in names) / 1e3, 1), "us_per_pair": round(best / pairs * 1e6, 2),
               "protocol_3x2048x2048_minutes_EXTRAPOLATED": round(best / pairs * PROTOCOL_PAIRS / 60, 1),
               "worst_relative_difference_of_the_two": diff}
        if k == "pairwise":
            rec["speedup_over_batched"] = round(min(times["batched"]) / best, 2)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
