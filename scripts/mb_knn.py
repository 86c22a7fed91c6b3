"""The kNN label filter (semseg.models.kNN2d: csrc/knn.hip) against the tensor-op composition of tests/knn_ref.py in
float32 on the same device, and the confusion counts (csrc/segcount.hip) against the reference's evaluate loop written
with tensor ops: B = 8, 4 classes, kernel_size 3 / k 3 and kernel_size 5 / k 5, at 64 x 512 and 64 x 2048.

    python scripts/mb_knn.py [--widths 512 2048] [--iters 200] [--rounds 3]

The variants alternate within one process (rounds); each timed window ends in a device synchronise; launches are
counted with torch.profiler in a pass of its own.  The filter's algorithmic bytes are depth (4) + labels (8) in and
labels (8) out per pixel, set against the rate of a device-to-device copy of 1 GiB (the copy-kernel roof, half read
and half write) measured in the same process; `composition_tensor_bytes` is the [B,K,H*W] float32 tensor the
composition materialises (several times over).  The counts move 8 + 8 + 4 bytes per pixel.  Prints one JSON line per
(width, kernel_size, variant)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dusty-gan-v2_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from knn_ref import distances, fragile_threshold, knn_ref  # noqa: E402
from semseg.metrics import confusion, counts_from_confusion  # noqa: E402
from semseg.models import kNN2d  # noqa: E402

DEV = "cuda"
B, C, H = 8, 4, 64


def launches(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)


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


def evaluate_composed(label, pred, num_classes):
    """the reference's loop (test_semseg.py:32-40) with tensor ops, counts kept on the device"""
    tps, fps, fns = [], [], []
    for c in range(num_classes):
        tps.append((pred[label == c] == c).sum())
        fps.append((label[pred == c] != c).sum())
        fns.append((pred[label == c] != c).sum())
    return torch.stack(tps), torch.stack(fps), torch.stack(fns)


def time_rounds(fns, iters, rounds, slow_prefix="composed"):
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            n = max(5, iters // 10) if k.startswith(slow_prefix) else iters
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / n * 1e6)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_knn: needs the GPU (no CPU path)")
    roof = copy_roof()
    print(json.dumps({"bench": "knn2d", "copy_roof_GBps": round(roof / 1e9, 1)}), flush=True)
    for W in args.widths:
        g = torch.Generator().manual_seed(W)
        depth = 1 + (0.012 * torch.randn(B, 1, 1, W, generator=g)).cumsum(3) + (0.012 * torch.randn(B, 1, H, 1, generator=g)).cumsum(2)
        depth = depth + 0.004 * torch.randn(B, 1, H, W, generator=g)
        u = torch.rand(B, 1, H, W, generator=g)
        depth = torch.where(u < 0.015, torch.full_like(depth, -1.0), torch.where(u < 0.035, torch.zeros_like(depth), depth)).to(DEV)
        label = (torch.arange(W) // 23 % C).expand(B, H, W)
        label = torch.where(torch.rand(B, H, W, generator=g) < 0.08, torch.randint(0, C, (B, H, W), generator=g), label).to(DEV)
        mask = (torch.rand(B, H, W, generator=g) < 0.8).float().to(DEV)
        px = B * H * W
        for ks in (3, 5):
            knn = kNN2d(C, k=ks, kernel_size=ks).to(DEV)

            def native():
                return knn(depth, label)

            def composed():
                return knn_ref(depth, label, knn.dist_kernel, knn.k, C, knn.cutoff, with_margin=False)[0]
            a, b = native(), composed()
            differ = int((a != b).sum())
            # which of the two is off: the first two samples against the restatement on the CPU, in float32 outside
            # the pixels whose float64 decision margin is within rounding (the rule of tests/test_gpu_knn.py); and
            # the NaNs among the composition's distances on the device (its conv2d meets inf there)
            d_cpu, l_cpu, w_cpu = depth[:2].cpu(), label[:2].cpu(), knn.dist_kernel.cpu()
            l32, d32, _ = knn_ref(d_cpu, l_cpu, w_cpu, knn.k, C, knn.cutoff)
            _, d64, m64 = knn_ref(d_cpu.double(), l_cpu, w_cpu.double(), knn.k, C, knn.cutoff)
            solid = m64 >= fragile_threshold(d64, d32)[0]
            check = {"pixels_checked_on_cpu": int(solid.sum()),
                     "native_differs_from_cpu": int(((a[:2].cpu() != l32) & solid).sum()),
                     "composed_differs_from_cpu": int(((b[:2].cpu() != l32) & solid).sum()),
                     "composed_nan_distances": int(torch.isnan(distances(depth, knn.dist_kernel)).sum()),
                     "cpu_nan_distances": int(torch.isnan(d32).sum())}
            times = time_rounds({"native": native, "composed": composed}, args.iters, args.rounds)
            for k, fn in (("native", native), ("composed", composed)):
                rec = {"bench": "knn2d", "variant": k, "shape": [B, H, W], "kernel_size": ks, "k": ks, "classes": C,
                       "us_per_call_rounds": [round(t, 1) for t in times[k]], "us_per_call_min": round(min(times[k]), 1),
                       "launches_per_call": launches(fn), "pixels_native_differs_from_composed": differ,
                       "labels_changed_share": round(float((a != label).float().mean()), 3),
                       "composition_tensor_bytes": 4 * px * ks * ks, **check}
                if k == "native":
                    rate = 20 * px / (min(times[k]) * 1e-6)
                    rec.update(algorithmic_bytes=20 * px, achieved_GBps=round(rate / 1e9, 1),
                               fraction_of_copy_roof=round(rate / roof, 3),
                               speedup_over_composed=round(min(times["composed"]) / min(times["native"]), 1))
                print(json.dumps(rec), flush=True)

        pred = knn(depth, label)
        lab_m, pred_m = (label * mask).long(), (pred * mask).long()
        conf = torch.zeros(C + 1, C + 1, device=DEV, dtype=torch.int64)

        def native_counts():
            return counts_from_confusion(confusion(label, pred, C, mask=mask, out=conf.zero_()))

        def native_kernel():
            return confusion(label, pred, C, mask=mask, out=conf)      # the launch alone, accumulating

        def composed_counts():
            return evaluate_composed(lab_m, pred_m, C)      # the mask already multiplied in: not timed
        same = all(torch.equal(x, y) for x, y in zip(native_counts(), composed_counts()))
        times = time_rounds({"native": native_counts, "native_kernel": native_kernel, "composed": composed_counts}, args.iters,
                            args.rounds)
        for k, fn in (("native", native_counts), ("native_kernel", native_kernel), ("composed", composed_counts)):
            rec = {"bench": "seg_confusion", "variant": k, "shape": [B, H, W], "classes": C,
                   "us_per_call_rounds": [round(t, 1) for t in times[k]], "us_per_call_min": round(min(times[k]), 1),
                   "launches_per_call": launches(fn), "counts_equal": same}
            if k == "native":
                rec.update(speedup_over_composed=round(min(times["composed"]) / min(times["native"]), 1))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
