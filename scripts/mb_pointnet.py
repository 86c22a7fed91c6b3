"""The PointNet trunks of FPD / KPD as native calls (csrc/pointnet.hip) against the library-GEMM composition of
gans/metrics/pointnet.py on the same device, in one process.

    python scripts/mb_pointnet.py [--iters 5] [--rounds 3] [--shapes 32x32768 8x32768 32x2048]

Shapes are the workload's own: (B, N) = (32, 32768) is one test_gan.py batch of 64 x 512 clouds, then (8, 32768) and
(32, 2048).  Per shape two benches: the whole PointNet1.forward, and the feature trunk alone (the bmm with the
transform, three per-point layers, the max; folded float32 weights prepared outside the timed window).  The variants
alternate within one process (rounds); each timed window is `iters` calls ending in one device synchronise and the
figure reported is the minimum per call over the rounds, with the rounds beside it.  Launches are counted and the device
time of one profiled call is taken with torch.profiler in a pass of its own; torch.cuda.max_memory_allocated of one call
(above what was allocated before it) is reported per variant.  For the trunk the achieved FLOP/s (2 N B (3*3 + 3*64 +
64*128 + 128*1024)) is set against the 157.3 TFLOP/s peak of v_mfma_f32_32x32x2_f32, the form the kernel uses.  The last
line extrapolates the feature time of the 3 x 50 000-cloud protocol from the (32, 32768) whole-forward figure: an
extrapolation, not a measurement.  Prints one JSON line per (bench, shape, variant)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
PEAK_F32_MFMA = 157.3e12
PROTOCOL_CLOUDS = 3 * 50000


def kernels(fn):
    import torch
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [(e.name, round(e.time_range.elapsed_us(), 1)) for e in prof.events() if e.device_type == DeviceType.CUDA]


def time_rounds(fns, iters, rounds):
    import torch
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / iters * 1e6)
    return times


def peak_bytes(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def report(bench, shape, fns, iters, rounds, flops, extra):
    times = time_rounds(fns, iters, rounds)
    recs = {}
    for k, fn in fns.items():
        names = kernels(fn)
        rec = {"bench": bench, "variant": k, "shape": list(shape), "us_per_call_rounds": [round(t, 1) for t in times[k]],
               "us_per_call_min": round(min(times[k]), 1), "launches_per_call": len(names),
               "device_us_profiled_call": round(sum(t for _, t in names), 1), "max_memory_allocated_bytes": peak_bytes(fn), **extra}
        if flops:
            rec["TFLOPs"] = round(flops / (min(times[k]) * 1e-6) / 1e12, 1)
            rec["fraction_of_f32_mfma_peak"] = round(flops / (min(times[k]) * 1e-6) / PEAK_F32_MFMA, 3)
        if k == "native":
            rec["speedup_over_library"] = round(min(times["library"]) / min(times["native"]), 2)
            rec["kernels"] = sorted({n for n, _ in names})
        recs[k] = rec
        print(json.dumps(rec), flush=True)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["32x32768", "8x32768", "32x2048"])
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dusty-gan-v2_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("mb_pointnet: needs the GPU (no CPU path)")
    import recipe
    from gans.metrics import pointnet as M
    from gans.models.ops.native import pointnet as W
    torch.set_grad_enabled(False)
    net = M.PointNet1(k=16)
    recipe.fill_pointnet(net.state_dict())
    net = net.eval().requires_grad_(False).to(DEV)
    feat = net.feat
    layers = [tuple(t.contiguous() for t in M._fold(c, b)) for c, b in ((feat.conv1, feat.bn1), (feat.conv2, feat.bn2), (feat.conv3, feat.bn3))]
    print(json.dumps({"bench": "pointnet", "device": torch.cuda.get_device_name(0), "pointnet_native_default": M.POINTNET_NATIVE,
                      "tile": W.P, "span": W.S, "iters": args.iters, "rounds": args.rounds}), flush=True)

    def routed(flag, x):
        before = M.POINTNET_NATIVE
        M.POINTNET_NATIVE = flag
        try:
            return net(x)
        finally:
            M.POINTNET_NATIVE = before

    def library_trunk(pts, trans):
        chunk = max(1, int(M.PointNet1.ACT_BYTES // (1024 * 4 * pts.size(1))))   # the chunk walk of PointNet1.forward
        outs = []
        for i in range(0, pts.size(0), chunk):
            x = torch.bmm(pts[i:i + chunk], trans[i:i + chunk])
            x = F.relu(F.linear(x, *layers[0]))
            x = F.relu(F.linear(x, *layers[1]))
            outs.append(F.linear(x, *layers[2]).amax(dim=1))
        return torch.cat(outs)

    whole = {}
    for s in args.shapes:
        B, n = (int(v) for v in s.split("x"))
        pts = (recipe.point_clouds(1000 + n, B, n) + torch.tensor((2.0, -1.0, 0.5))).to(DEV)
        x = pts.transpose(1, 2)
        trans = net.feat.stn(pts).contiguous()
        fns = {"native": lambda: routed(True, x), "library": lambda: routed(False, x)}
        a, b = fns["native"](), fns["library"]()
        extra = {"max_diff_over_max": float((a - b).abs().max() / b.abs().max())}
        whole[(B, n)] = report("pointnet1_forward", (B, n), fns, args.iters, args.rounds, 0, extra)
        fns = {"native": lambda: W.pointnet_trunk(pts, trans, *layers, False), "library": lambda: library_trunk(pts, trans)}
        a, b = fns["native"](), fns["library"]()
        extra = {"max_diff_over_max": float((a - b).abs().max() / b.abs().max())}
        flops = 2.0 * B * n * (3 * 3 + 3 * 64 + 64 * 128 + 128 * 1024)
        report("feature_trunk", (B, n), fns, args.iters, args.rounds, flops, extra)
        del pts, x, trans
        torch.cuda.empty_cache()
    if (32, 32768) in whole:
        recs = whole[(32, 32768)]
        print(json.dumps({"bench": "protocol_extrapolation", "clouds": PROTOCOL_CLOUDS, "points_per_cloud": 32768,
                          "EXTRAPOLATED_from": "pointnet1_forward (32, 32768) us_per_call_min",
                          **{f"{k}_seconds": round(r["us_per_call_min"] * 1e-6 * PROTOCOL_CLOUDS / 32, 1) for k, r in recs.items()}}),
              flush=True)


if __name__ == "__main__":
    main()
