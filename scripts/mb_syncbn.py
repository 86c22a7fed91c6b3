"""Training-mode batch norm as the native synchronised one (csrc/syncbn.hip, two launches each way) against the library's
nn.BatchNorm2d in training mode on the same device, forward alone and forward + backward.

    python scripts/mb_syncbn.py [--iters 50] [--rounds 3] [--dtypes float32 float16] [--batch 40]

Configurations: the three activation shapes SqueezeSegV2's norms see most bytes at, at the published batch of 40 --
40 x 64 x 64 x 512, 40 x 128 x 64 x 128, 40 x 512 x 64 x 32.  The variants alternate within one process (rounds); each
timed window is `iters` calls ending in a device synchronise and the figure reported is the minimum per call over the
rounds, with the rounds beside it; launches are counted and the device time of one profiled call taken with
torch.profiler in a pass of its own.  Compulsory bytes: a batch norm reads its input twice whatever the code (the
statistics are needed before the first output) -- forward x twice + y once = 3 N s bytes; backward dy and x twice +
dx once = 5 N s; forward + backward 8 N s -- set against the rate of a 1 GiB device-to-device copy measured in the same
process.  (N elements of s bytes; the activations here are 84 to 336 MB, above the 256 MB the last-level cache holds
only in the first configuration in float32.)  Prints one JSON line per (configuration, dtype, pass, variant)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dusty-gan-v2_amd")]
SHAPES = [("bn_64", (64, 64, 512)), ("bn_128", (128, 64, 128)), ("bn_512", (512, 64, 32))]
DEV = "cuda"


def kernels(fn):
    import torch
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [(e.name, round(e.time_range.elapsed_us(), 1)) for e in prof.events() if e.device_type == DeviceType.CUDA]


def copy_roof():
    """bytes per second (read + write) of a 1 GiB device-to-device copy"""
    import torch
    src = torch.empty(1 << 28, device=DEV, dtype=torch.float32).normal_()
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        dst.copy_(src)
    torch.cuda.synchronize()
    return 2 * src.numel() * 4 * 20 / (time.perf_counter() - t0)


def time_rounds(fns, iters, rounds):
    import torch
    for fn in fns.values():
        for _ in range(10):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtypes", nargs="+", default=["float32", "float16"])
    ap.add_argument("--batch", type=int, default=40)
    args = ap.parse_args()
    import torch
    from semseg.models import SyncBatchNorm2d
    if not torch.cuda.is_available():
        raise SystemExit("mb_syncbn: needs the GPU (no CPU path)")
    roof = copy_roof()
    print(json.dumps({"bench": "syncbn", "copy_roof_GBps": round(roof / 1e9, 1), "batch": args.batch}), flush=True)
    for dname in args.dtypes:
        dtype = getattr(torch, dname)
        for seed, (name, (C, H, W)) in enumerate(SHAPES):
            shape = (args.batch, C, H, W)
            g = torch.Generator().manual_seed(seed)
            x = torch.randn(shape, generator=g).to(DEV).to(dtype).requires_grad_(True)
            dy = torch.randn(shape, generator=g).to(DEV).to(dtype)
            mods = {"native": SyncBatchNorm2d(C, momentum=0.001).to(DEV).train(),
                    "library": torch.nn.BatchNorm2d(C, momentum=0.001).to(DEV).train()}
            for m in mods.values():
                with torch.no_grad():
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.uniform_(-0.3, 0.3)
            mods["library"].load_state_dict(mods["native"].state_dict())

            def fwd(m):
                with torch.no_grad():
                    return m(x)

            def fwd_bwd(m):
                y = m(x)
                return torch.autograd.grad(y, (x, m.weight, m.bias), dy)

            a, b = fwd(mods["native"]).float(), fwd(mods["library"]).float()
            ga, gb = fwd_bwd(mods["native"])[0].float(), fwd_bwd(mods["library"])[0].float()
            extra = {"y_max_diff_over_max": float((a - b).abs().max() / b.abs().max()),
                     "dx_max_diff_over_max": float((ga - gb).abs().max() / gb.abs().max())}
            del a, b, ga, gb
            nbytes = x.numel() * x.element_size()
            for pass_name, run, factor in (("forward", fwd, 3), ("forward_backward", fwd_bwd, 8)):
                fns = {k: (lambda m=m: run(m)) for k, m in mods.items()}
                times = time_rounds(fns, args.iters, args.rounds)
                for k, fn in fns.items():
                    names = kernels(fn)
                    best = min(times[k])
                    rec = {"bench": name, "pass": pass_name, "variant": k, "shape": list(shape), "dtype": dname,
                           "us_per_call_rounds": [round(t, 1) for t in times[k]], "us_per_call_min": round(best, 1),
                           "launches_per_call": len(names), "device_us_profiled_call": round(sum(t for _, t in names), 1),
                           "compulsory_bytes": factor * nbytes, "achieved_GBps": round(factor * nbytes / (best * 1e-6) / 1e9, 1),
                           "fraction_of_copy_roof": round(factor * nbytes / (best * 1e-6) / roof, 3), **extra}
                    if k == "native":
                        rec["speedup_over_library"] = round(min(times["library"]) / best, 2)
                        rec["kernels"] = sorted({n for n, _ in names})
                    print(json.dumps(rec), flush=True)
            del x, dy, mods
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
