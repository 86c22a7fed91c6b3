"""The segmentation training step (semseg.trainer.Trainer) measured two ways.

(a) The optimizer tail alone over SqueezeSegV2's real parameter list (4 classes, CRF): native.fused_clip_sgd_step
    against torch's sequence -- clip_grad_norm_ + SGD.step, and under AMP GradScaler.unscale_ + clip_grad_norm_ +
    GradScaler.step + GradScaler.update.  The two alternate within one process for --rounds rounds; a timed window is
    --calls calls ending in ONE device synchronise, and the figure is the smallest window divided by the calls.  The
    gradients have norm 0.5 and torch's loss scale is 1, so neither sequence changes them from call to call.  The
    launches of one call of each (kernels and device-to-device copies; profiler ranges are not counted) are listed
    with torch.profiler in a pass of their own.
(b) A whole training step at 64 x 512, batch --batch, split by events into forward, loss, backward and optimizer, in
    float32 and under AMP (float16 autocast), after --warmup steps: mean and smallest time per phase over --steps.

    python scripts/mb_semseg_step.py [--rounds 3] [--calls 50] [--batch 40] [--steps 20] [--warmup 20] [--skip_step]
                                     [--skip_tail] [--sync_bn]

--sync_bn measures (b) with the model's batch norms swapped for the native synchronised ones (section 39) beside the
library's, the two alternating.

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dusty-gan-v2_amd")]
import torch  # noqa: E402

from gans.models.ops.native import fused_clip_sgd_step  # noqa: E402
from semseg.config import default_config  # noqa: E402
from semseg.datasets import SyntheticFrontal  # noqa: E402
from semseg.trainer import BACKOFF, GROWTH, GROWTH_INTERVAL, Trainer, build_model  # noqa: E402

DEV = "cuda"
MAX_NORM = 1.0


def launches(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    # kernels and device copies only: the profiler also reports torch's range `Optimizer.step#SGD.step` as a device event
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and not e.name.startswith("Optimizer.step#")]


def model_params(cfg):
    """Two copies of the model's parameters with equal gradients of total norm 0.5 (below MAX_NORM: no sequence scales them)."""
    torch.manual_seed(0)
    model = build_model(cfg, pretrained_weights=False).to(DEV)
    sets = []
    for _ in range(2):
        ps = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
        gen = torch.Generator(device=DEV).manual_seed(1)
        for p in ps:
            p.grad = torch.randn(p.shape, device=DEV, generator=gen)
        norm = torch.sqrt(sum((p.grad ** 2).sum() for p in ps))
        for p in ps:
            p.grad.mul_(0.5 / norm)
        sets.append(ps)
    return sets


def tail_variants(cfg, amp):
    tr = cfg.training
    kw = dict(lr=tr.lr, momentum=tr.lr_momentum, weight_decay=tr.weight_decay)
    ours, theirs = model_params(cfg)
    opt_f, opt_t = torch.optim.SGD(ours, **kw), torch.optim.SGD(theirs, **kw)
    if not amp:
        def fused():
            fused_clip_sgd_step(opt_f, MAX_NORM)

        def torch_seq():
            torch.nn.utils.clip_grad_norm_(theirs, MAX_NORM)
            opt_t.step()
    else:
        state = torch.tensor([1.0, 0.0], device=DEV)
        scaler = torch.amp.GradScaler("cuda", init_scale=1.0, growth_interval=1 << 30)
        scaler.scale(torch.ones(1, device=DEV))      # creates the scaler's device state

        def fused():
            fused_clip_sgd_step(opt_f, MAX_NORM, scale_state=state, growth_interval=1 << 30)

        def torch_seq():
            scaler.unscale_(opt_t)
            torch.nn.utils.clip_grad_norm_(theirs, MAX_NORM)
            scaler.step(opt_t)
            scaler.update()
    return {"fused": fused, "torch": torch_seq}, sum(p.numel() for p in ours), len(ours)


def measure_tail(cfg, amp, rounds, calls):
    fns, numel, tensors = tail_variants(cfg, amp)
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    best = {k: float("inf") for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            best[k] = min(best[k], (time.perf_counter() - t0) / calls)
    for k, fn in fns.items():
        names = launches(fn)
        print(json.dumps({"measure": "tail", "amp": amp, "variant": k, "us_per_call": round(best[k] * 1e6, 1),
                          "launches": len(names), "tensors": tensors, "elements": numel,
                          "kernels": sorted(set(names))[:12]}), flush=True)


def measure_step(cfg, amp, batch, steps, warmup, fused, sync_bn=False):
    cfg.use_amp = amp
    torch.manual_seed(0)
    tr = Trainer(cfg, DEV, fused_optimizer=fused, pretrained_weights=False, sync_bn=sync_bn)
    data = SyntheticFrontal(batch, tuple(cfg.dataset.shape), cfg.dataset.num_classes, seed=0)
    item = next(iter(torch.utils.data.DataLoader(data, batch_size=batch)))
    item = tr._to_device(item)
    phases = ("forward", "loss", "backward", "optimizer")
    times = {k: [] for k in phases}
    for it in range(warmup + steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        logit = tr._forward(item)
        ev[1].record()
        loss, _ = tr.criterion(logit, item["label"], item["mask"], conf=tr.conf_train)
        loss = loss * tr.loss_coef
        ev[2].record()
        tr.optimizer.zero_grad(set_to_none=True)
        if fused:
            (loss * tr.scale[0] if tr.scale is not None else loss).backward()
            ev[3].record()
            fused_clip_sgd_step(tr.optimizer, tr.max_grad_norm, scale_state=tr.scale, growth=GROWTH, backoff=BACKOFF,
                                growth_interval=GROWTH_INTERVAL)
        elif tr.grad_scaler is None:
            loss.backward()
            ev[3].record()
            torch.nn.utils.clip_grad_norm_(list(tr.model.parameters()), tr.max_grad_norm)
            tr.optimizer.step()
        else:
            tr.grad_scaler.scale(loss).backward()
            ev[3].record()
            tr.grad_scaler.unscale_(tr.optimizer)
            torch.nn.utils.clip_grad_norm_(list(tr.model.parameters()), tr.max_grad_norm)
            tr.grad_scaler.step(tr.optimizer)
            tr.grad_scaler.update()
        ev[4].record()
        torch.cuda.synchronize()
        if it >= warmup:
            for k, a, b in zip(phases, ev[:-1], ev[1:]):
                times[k].append(a.elapsed_time(b))
    row = {"measure": "step", "amp": amp, "fused_optimizer": fused, "sync_bn": sync_bn, "batch": batch, "shape": list(cfg.dataset.shape),
           "loss_scale": tr.loss_scale(), "loss": float(loss)}
    for k in phases:
        row[k + "_ms_mean"] = round(sum(times[k]) / len(times[k]), 3)
        row[k + "_ms_min"] = round(min(times[k]), 3)
    row["total_ms_mean"] = round(sum(row[k + "_ms_mean"] for k in phases), 3)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--batch", type=int, default=40)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--skip_step", action="store_true")
    ap.add_argument("--skip_tail", action="store_true")
    ap.add_argument("--sync_bn", action="store_true")
    args = ap.parse_args()
    cfg = default_config()
    if not args.skip_tail:
        for amp in (False, True):
            measure_tail(cfg, amp, args.rounds, args.calls)
    if args.sync_bn:
        for amp in (False, True):
            for sync_bn in (False, True, False, True):
                measure_step(default_config(), amp, args.batch, args.steps, args.warmup, True, sync_bn=sync_bn)
    elif not args.skip_step:
        for amp in (False, True):
            for fused in (True, False):
                measure_step(default_config(), amp, args.batch, args.steps, args.warmup, fused)


if __name__ == "__main__":
    main()
