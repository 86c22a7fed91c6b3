"""The evaluation-mode Fire module as one native launch (csrc/fire.hip) against the same module composed of library
ops on the same device, and a whole SqueezeSegV2 evaluation forward with the Fire modules routed either way.

    python scripts/mb_fire.py [--iters 100] [--rounds 3] [--dtypes float32 float16]

Configurations: the first encoder Fire (64 -> 16 -> 64 + 64) at 8 x 64 x 64 x 128, Fire(512, 64, 256, 256) at
8 x 512 x 64 x 32, the decoder's fire_13 (64 -> 16 -> 32 + 32, up, with skip) at 8 x 64 x 64 x 256, and SqueezeSegV2
(five input channels, four classes) at 8 x 5 x 64 x 512.  The variants alternate within one process (rounds); each timed
window ends in a device synchronise and reports the minimum per call over the rounds; launches are counted and the
device time of one profiled call taken with torch.profiler in a pass of its own.  The Fire's compulsory bytes are x
read once, skip read once and y written once -- set against the rate of a 1 GiB device-to-device copy measured in the
same process.  The composed 16-bit variant runs a copy of the module cast to that dtype.  Prints one JSON line per
(configuration, dtype, variant)."""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dusty-gan-v2_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from semseg.models import SqueezeSegV2, common, squeezeseg_v2  # noqa: E402

DEV = "cuda"
# name, (in_ch, s1x1, e1x1, e3x3, up), input shape, skip
FIRES = [("fire_2", (64, 16, 64, 64, False), (8, 64, 64, 128), False),
         ("fire_9", (512, 64, 256, 256, False), (8, 512, 64, 32), False),
         ("fire_13", (64, 16, 32, 32, True), (8, 64, 64, 256), True)]
MODEL_SHAPE = (8, 5, 64, 512)


def kernels(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [(e.name, round(e.time_range.elapsed_us(), 1)) for e in prof.events() if e.device_type == DeviceType.CUDA]


def copy_roof():
    """bytes per second (read + write) of a 1 GiB device-to-device copy"""
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


def randomise(module, seed):
    """He-scaled conv weights, non-trivial biases and batch-norm statistics: no branch of the kernel sees zeros."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if name.endswith("num_batches_tracked"):
                continue
            if t.ndim == 4:
                fan = t.shape[0] * 2 if "upsample" in name else t.shape[1] * t.shape[2] * t.shape[3]
                t.copy_((torch.rand(t.shape, generator=g) * 2 - 1) * (6.0 / fan) ** 0.5)
            elif name.endswith("running_var") or name.endswith(".weight"):
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            else:
                t.copy_(torch.rand(t.shape, generator=g) * 0.6 - 0.3)
    return module


def report(bench, shape, dtype, fns, iters, rounds, nbytes, roof, agree):
    times = time_rounds(fns, iters, rounds)
    for k, fn in fns.items():
        names = kernels(fn)
        rec = {"bench": bench, "variant": k, "shape": list(shape), "dtype": str(dtype).split(".")[1],
               "us_per_call_rounds": [round(t, 1) for t in times[k]], "us_per_call_min": round(min(times[k]), 1),
               "launches_per_call": len(names), "device_us_profiled_call": round(sum(t for _, t in names), 1), **agree}
        if k == "native":
            rec["speedup_over_composed"] = round(min(times["composed"]) / min(times["native"]), 2)
            if nbytes:
                rate = nbytes / (min(times[k]) * 1e-6)
                dev_rate = nbytes / (rec["device_us_profiled_call"] * 1e-6)
                rec.update(kernels=sorted({n for n, _ in names}), compulsory_bytes=nbytes, achieved_GBps=round(rate / 1e9, 1),
                           fraction_of_copy_roof=round(rate / roof, 3), fraction_of_copy_roof_device=round(dev_rate / roof, 3))
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtypes", nargs="+", default=["float32", "float16"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_fire: needs the GPU (no CPU path)")
    roof = copy_roof()
    print(json.dumps({"bench": "fire", "copy_roof_GBps": round(roof / 1e9, 1)}), flush=True)
    torch.set_grad_enabled(False)
    for dname in args.dtypes:
        dtype = getattr(torch, dname)
        for seed, (name, (cin, cs, e1, e3, up), shape, with_skip) in enumerate(FIRES):
            fire = randomise(squeezeseg_v2.Fire(cin, cs, e1, e3, 0.001, up=up), seed).eval().to(DEV)
            cast = fire if dtype == torch.float32 else copy.deepcopy(fire).to(dtype)
            g = torch.Generator().manual_seed(100 + seed)
            x = torch.randn(shape, generator=g).to(DEV).to(dtype)
            oshape = (shape[0], e1 + e3, shape[2], shape[3] * (2 if up else 1))
            skip = torch.randn(oshape, generator=g).to(DEV).to(dtype) if with_skip else None
            fns = {"native": lambda: common.fire_native(fire, x, skip), "composed": lambda: common.fire_composition(cast, x, skip)}
            a, b = fns["native"]().float(), fns["composed"]().float()
            agree = {"max_diff_over_max": float((a - b).abs().max() / b.abs().max())}
            esz = x.element_size()
            nbytes = esz * (x.numel() + (2 if with_skip else 1) * a.numel())
            report(name, shape, dtype, fns, args.iters, args.rounds, nbytes, roof, agree)

        model = randomise(SqueezeSegV2(["xyz", "depth", "mask"], 4, pretrained_weights=False), 7).eval().to(DEV)
        composed_model = model
        if dtype != torch.float32:
            # the stem, CAMs and head are library ops and need parameters of the activations' dtype; the native Fire reads
            # the module's float32 parameters, the composed Fire needs them cast as well
            composed_model = copy.deepcopy(model).to(dtype)
            model = copy.deepcopy(composed_model)
            for m in model.modules():
                if isinstance(m, squeezeseg_v2.Fire):
                    m.float()
        img = torch.randn(MODEL_SHAPE, generator=torch.Generator().manual_seed(9)).to(DEV).to(dtype)

        def routed(flag):
            common.FIRE_NATIVE = flag
            try:
                return (model if flag else composed_model)(img)
            finally:
                common.FIRE_NATIVE = True
        fns = {"native": lambda: routed(True), "composed": lambda: routed(False)}
        a, b = fns["native"]().float(), fns["composed"]().float()
        agree = {"max_diff_over_max": float((a - b).abs().max() / b.abs().max())}
        report("squeezeseg_v2_eval", MODEL_SHAPE, dtype, fns, max(args.iters // 4, 5), args.rounds, 0, roof, agree)


if __name__ == "__main__":
    main()
