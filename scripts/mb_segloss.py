"""The segmentation training objective (semseg.models.MaskedSegLoss: csrc/segloss.hip) against the same objective
composed of tensor ops under autograd on the same device: forward + backward of the masked focal loss with the step's
predictions and training confusion counts, B = 8, 4 classes, gamma 2, class weights, at 64 x 512 and 64 x 2048, float32
and bfloat16 logits.

    python scripts/mb_segloss.py [--widths 512 2048] [--iters 200] [--rounds 3]

The variants alternate within one process (rounds); each timed window ends in a device synchronise; launches are
counted, and the native kernels listed by name with the device time of that one profiled call, with torch.profiler in
a pass of its own.  The native algorithmic bytes per pixel: C logits read twice (forward, backward) and C gradients
written in the logits' dtype, labels (8) and mask (4) read twice, predictions (8) written -- set against the rate of a
device-to-device copy of 1 GiB measured in the same process.  Prints one JSON line per (width, dtype, variant)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dusty-gan-v2_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from semseg.metrics import confusion  # noqa: E402
from semseg.models import MaskedSegLoss  # noqa: E402

DEV = "cuda"
B, C, H, GAMMA = 8, 4, 64, 2.0


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
        for _ in range(50):
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
    ap.add_argument("--widths", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_segloss: needs the GPU (no CPU path)")
    roof = copy_roof()
    print(json.dumps({"bench": "segloss", "copy_roof_GBps": round(roof / 1e9, 1)}), flush=True)
    alpha = torch.tensor([0.33, 1.0, 3.5, 2.0], device=DEV)
    crit = MaskedSegLoss(GAMMA, alpha=alpha)
    for W in args.widths:
        g = torch.Generator().manual_seed(W)
        label = torch.randint(0, C, (B, H, W), generator=g).to(DEV)
        mask = (torch.rand(B, H, W, generator=g) < 0.8).float().to(DEV)
        conf = torch.zeros(C + 1, C + 1, device=DEV, dtype=torch.int64)
        px = B * H * W
        for dtype in (torch.float32, torch.bfloat16):
            z = (3 * torch.randn(B, C, H, W, generator=g)).to(DEV).to(dtype).requires_grad_(True)

            def native():
                z.grad = None
                loss, pred = crit(z, label, mask, conf=conf)
                loss.backward()
                return loss, pred

            def composed():
                # the objective as tensor ops: weighted cross-entropy, the label's softmax probability, the focal
                # weight, the masked mean; then the argmax and the masked counts of the training scores
                z.grad = None
                xent = F.cross_entropy(z, label, weight=alpha.to(z.dtype), reduction="none")
                py = F.softmax(z, dim=1).gather(1, label[:, None]).squeeze(1)
                loss = ((1 - py) ** GAMMA * xent * mask).sum() / mask.sum()
                loss.backward()
                pred = (z.detach().argmax(dim=1) * mask).long()
                confusion((label * mask).long(), pred, C, out=conf)
                return loss, pred
            (la, pa), ga = native(), z.grad.clone()
            (lb, pb), gb = composed(), z.grad.clone()
            la, lb = float(la.detach()), float(lb.detach())
            agree = {"loss_rel_diff": abs(la - lb) / abs(lb), "pred_differ": int((pa != pb).sum()),
                     "grad_max_diff_over_max": float((ga.float() - gb.float()).abs().max() / gb.float().abs().max())}
            times = time_rounds({"native": native, "composed": composed}, args.iters, args.rounds)
            esz = z.element_size()
            nbytes = px * (3 * C * esz + 2 * (8 + 4) + 8)
            for k, fn in (("native", native), ("composed", composed)):
                names = kernels(fn)
                rec_kernel_us = round(sum(t for _, t in names), 1)
                rec = {"bench": "segloss", "variant": k, "shape": [B, C, H, W], "dtype": str(dtype).split(".")[1],
                       "us_per_call_rounds": [round(t, 1) for t in times[k]], "us_per_call_min": round(min(times[k]), 1),
                       "launches_per_call": len(names), "device_us_profiled_call": rec_kernel_us, **agree}
                if k == "native":
                    rate = nbytes / (min(times[k]) * 1e-6)
                    rec.update(kernels=names, algorithmic_bytes=nbytes, achieved_GBps=round(rate / 1e9, 1),
                               fraction_of_copy_roof=round(rate / roof, 3),
                               speedup_over_composed=round(min(times["composed"]) / min(times["native"]), 1))
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
