"""The CRF-RNN layer (semseg.models.CRFRNN: csrc/crf.hip) against the tensor-op composition of tests/crf_ref.py in
float32 on the same device: forward and forward + backward at 64 x 512 and 64 x 2048, B = 8, C = 4, 3 iterations.

    python scripts/mb_crf.py [--widths 512 2048] [--iters 100] [--rounds 3]

The two variants alternate within one process (rounds); each timed window ends in a device synchronise; launches are
counted with torch.profiler in a pass of its own.  Bytes per iteration are the compulsory traffic of the native
kernels computed from the shapes (every operand read once, every result written once):
    forward   Q in, U, Q out (3C planes), xyz (3), mask (1)
    backward  fields launch: Q, dQ', dU in and out (4C), xyz + mask (4), fields out (3C);
              gather launch: fields in (3C), Q (C), xyz + mask (4), dQ out (C)
and are set against the rate of a device-to-device copy of 1 GiB (the copy-kernel roof, half read and half write)
measured in the same process.  `bilateral_kernel_bytes` is the [B,C,K-1,H*W] tensor the reference's composition
materialises and re-reads every iteration.  Both run with one theta_beta for all classes (the layer's default) and with per-class ones.  Prints one JSON line
per (width, theta_beta, variant)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dusty-gan-v2_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from crf_ref import from_state_dict  # noqa: E402
from semseg.models import CRFRNN  # noqa: E402

DEV = "cuda"
B, C, H, ITERS = 8, 4, 64, 3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_crf: needs the GPU (no CPU path)")
    roof = copy_roof()
    print(json.dumps({"bench": "crf_rnn", "copy_roof_GBps": round(roof / 1e9, 1)}), flush=True)
    for W, theta in [(W, theta) for W in args.widths for theta in ("shared", "per_class")]:
        g = torch.Generator().manual_seed(W)
        # "shared": the layer's default, one theta_beta for all classes (a tap's bilateral weight is evaluated once);
        # "per_class": distinct ones (C evaluations per tap)
        crf = CRFRNN(C, theta_beta=0.015 if theta == "shared" else [0.015 * (1 + c) for c in range(C)],
                     num_iters=ITERS).to(DEV)
        unary = (2 * torch.randn(B, C, H, W, generator=g)).to(DEV).requires_grad_(True)
        xyz = (10 + (0.02 * torch.randn(B, 3, 1, W, generator=g)).cumsum(3)
               + (0.02 * torch.randn(B, 3, H, 1, generator=g)).cumsum(2)).to(DEV)
        mask = (torch.rand(B, H, W, generator=g) < 0.8).float().to(DEV)
        cot = torch.randn(B, C, H, W, generator=g).to(DEV)
        params = list(crf.parameters())
        sd = dict(crf.state_dict(keep_vars=True))

        def native_fwd():
            return crf(unary, xyz, mask)

        def composed_fwd():
            return from_state_dict(sd, unary, xyz, mask, ITERS)

        def fb(fwd):
            return lambda: torch.autograd.grad((fwd() * cot).sum(), [unary] + params)
        fns = {"native.fwd": native_fwd, "composed.fwd": composed_fwd, "native.fwd_bwd": fb(native_fwd),
               "composed.fwd_bwd": fb(composed_fwd)}
        diff = {"out": float((native_fwd() - composed_fwd()).detach().abs().max())}
        for k, (a, b) in zip(("g_unary", "g_wa", "g_ws", "g_M"), zip(fns["native.fwd_bwd"](), fns["composed.fwd_bwd"]())):
            diff[k] = float((a - b).abs().max() / b.abs().max())
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                n = args.iters if k.startswith("native") else max(5, args.iters // 10)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / n * 1e6)
        px = B * H * W
        bytes_it = {"native.fwd": 4 * px * (3 * C + 4), "native.fwd_bwd": 4 * px * ((3 * C + 4) + (7 * C + 4) + (5 * C + 4))}
        for k, fn in fns.items():
            rec = {"bench": "crf_rnn", "variant": k, "shape": [B, C, H, W], "theta_beta": theta, "iterations": ITERS,
                   "us_per_call_rounds": [round(t, 1) for t in times[k]], "us_per_call_min": round(min(times[k]), 1),
                   "launches_per_call": launches(fn), "native_vs_composed": diff,
                   "bilateral_kernel_bytes": 4 * px * C * (15 - 1)}
            if k in bytes_it:
                rate = bytes_it[k] * ITERS / (min(times[k]) * 1e-6)
                rec.update(bytes_per_iteration=bytes_it[k], achieved_GBps=round(rate / 1e9, 1),
                           fraction_of_copy_roof=round(rate / roof, 3))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
