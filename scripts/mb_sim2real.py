"""One stage-1 latent-fitting step on the 64 x 512 dusty_v2 generator (bf16 trunk, random weights), "w+" with the phase:
wall time and launches of

    (a) invert      gans.inversion.invert's stage 1 as it stands (torch.optim.Adam + LambdaLR + geocross_loss in tensor
                    ops): timed as invert(num_steps_1st = S + 1) minus invert(num_steps_1st = 1), num_steps_2nd = 0
    (b) fitter      gans.sim2real.LatentFitter, every step eager (forward, backward, ONE dgv2_latent_step)
    (c) fitter+graph the same step replayed as a hipGraph

    python scripts/mb_sim2real.py [--batches 8 16 32] [--steps 30] [--rounds 3]

The variants alternate within one process (rounds), each window ends in a device synchronise, the first window of every
variant is preceded by warm steps; launches are counted with torch.profiler in a pass of its own (device events of one
step; a replayed graph is ONE host call whatever it contains).  Prints one JSON line per (batch, variant), then the two
decisions the numbers make: LatentFitter's default `graph` (True only if (c) beats (b) by more than the measured spread
at B = 8) and render_gan_noise.py's default --batch_size (the B with the most scans per second)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dusty-gan-v2_amd")]
import torch  # noqa: E402

from gans.config import load_config  # noqa: E402
from gans.coords import CoordBridge, frontal_angle_grid  # noqa: E402
from gans.inversion import invert  # noqa: E402
from gans.models.builder import build_generator  # noqa: E402
from gans.sim2real import LatentFitter, latent_prior  # noqa: E402

DEV = "cuda"
FIT_STEPS = 500   # the production setting: the counters of a timed fitter never reach it


def device_events(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_sim2real: needs the GPU (no CPU path)")
    cfg = load_config()
    cfg.model.generator.synthesis_kwargs.num_fp16_layers = -1
    torch.manual_seed(0)
    G = build_generator(cfg.model.generator).to(DEV).eval().requires_grad_(False)
    coord = CoordBridge(64, 512, 1.45, 80.0, angle_array=frontal_angle_grid(64, 512)).to(DEV)
    prior = latent_prior(G, 1000, torch.Generator(device=DEV).manual_seed(0))
    S = args.steps
    rows = {}
    for B in args.batches:
        g = torch.Generator(device=DEV).manual_seed(B)
        depth = torch.rand(B, 1, 64, 512, device=DEV, generator=g) * 70 + 2
        mask = (torch.rand(B, 1, 64, 512, device=DEV, generator=g) < 0.85).float()

        def run_invert(steps):
            invert(G, coord, depth, mask, latent_type="w+", num_steps_1st=steps, num_steps_2nd=0, optimize_phase=True,
                   generator=torch.Generator(device=DEV).manual_seed(1), num_z_samples=64)
            G.requires_grad_(False)

        fitters = {"fitter": LatentFitter(G, coord, B, num_steps=FIT_STEPS, prior=prior, graph=False),
                   "fitter+graph": LatentFitter(G, coord, B, num_steps=FIT_STEPS, prior=prior, graph=True)}
        for f in fitters.values():
            f._load(depth, mask)
            for _ in range(5):      # the graph variant captures on its third call
                f._advance()
        run_invert(5)
        torch.cuda.synchronize()
        if not fitters["fitter+graph"].captured:
            print(json.dumps({"bench": "sim2real_step", "batch": B, "note": "capture failed: (c) is not measured"}))
        windows = {"invert": lambda: run_invert(S + 1), "invert_1": lambda: run_invert(1)}
        for name, f in fitters.items():
            windows[name] = (lambda f=f: [f._advance() for _ in range(S)])
        times = {k: [] for k in ("invert",) + tuple(fitters)}
        for _ in range(args.rounds):
            t_full, t_one = timed(windows["invert"]), timed(windows["invert_1"])
            times["invert"].append((t_full - t_one) / S * 1e3)
            for name in fitters:
                times[name].append(timed(windows[name]) / S * 1e3)
        launches = {"invert": (device_events(lambda: run_invert(3)) - device_events(lambda: run_invert(1))) / 2}
        for name, f in fitters.items():
            try:
                launches[name] = device_events(f._advance)
            except RuntimeError as e:   # a profiler that cannot follow a graph replay: the count is left out
                launches[name] = f"not counted ({type(e).__name__})"
        for name, ts in times.items():
            if name == "fitter+graph" and not fitters[name].captured:
                continue
            med = statistics.median(ts)
            row = {"bench": "sim2real_step", "variant": name, "batch": B, "dtype": "bf16",
                   "ms_per_step_rounds": [round(t, 3) for t in ts], "ms_per_step_median": round(med, 3),
                   "spread_ms": round(max(ts) - min(ts), 3), "device_events_per_step": launches[name],
                   "host_launch_calls_per_step": 1 if name == "fitter+graph" else launches[name],
                   "scans_per_second_at_500_steps": round(B / (med * 500 / 1e3), 3),
                   "scans_per_hour_at_500_steps": round(B / (med * 500 / 1e3) * 3600)}
            rows[(B, name)] = row
            print(json.dumps(row), flush=True)
        del fitters
    # the two decisions
    b8 = 8 if 8 in args.batches else args.batches[0]
    eager, graph = rows.get((b8, "fitter")), rows.get((b8, "fitter+graph"))
    use_graph = bool(graph) and eager["ms_per_step_median"] - graph["ms_per_step_median"] > max(eager["spread_ms"],
                                                                                             graph["spread_ms"])
    variant = "fitter+graph" if use_graph else "fitter"
    best = max((r for (B, n), r in rows.items() if n == variant), key=lambda r: r["scans_per_second_at_500_steps"])
    print(json.dumps({"decision": "defaults", "graph": use_graph, "decided_at_batch": b8,
                      "eager_ms": eager["ms_per_step_median"], "graph_ms": graph["ms_per_step_median"] if graph else None,
                      "spread_ms": max(eager["spread_ms"], graph["spread_ms"] if graph else 0.0),
                      "batch_size": best["batch"], "scans_per_second": best["scans_per_second_at_500_steps"],
                      "scans_per_hour": best["scans_per_hour_at_500_steps"]}), flush=True)


if __name__ == "__main__":
    main()
