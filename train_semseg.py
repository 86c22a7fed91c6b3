"""Train a range-image segmentation model on one or several GPUs (reference: train_semseg.py), headless.

    python train_semseg.py --config configs.yaml [--num_gpus N] [--sync_bn] [--max_steps N] [--batch_size B]
                           [--out_dir DIR] [--no_fused_optimizer]
    python train_semseg.py --synthetic --max_steps 100          # no data on disk: semseg.datasets.SyntheticFrontal

--num_gpus N (1 .. 8, default 1) splits training.batch_size over N fresh child processes (spawn), started before this
process touches a GPU: rank r trains on device r with its own shard of the sample stream, the batch norms' statistics
run over all N shards (semseg.models.SyncBatchNorm2d) and the gradients are averaged; only rank 0 logs, validates and
saves.  --sync_bn uses those batch norms on one GPU as well (off by default: DESIGN.md section 39 has the timing).

Every cfg.training.checkpoint.stats steps one JSON line goes to <out_dir>/train_log.jsonl and to stdout: step, mean
loss and gradient norm since the last line (over the steps where they are finite; non-finite values are written as
null and the steps skipped for a float16 overflow are counted), lr, loss scale and the per-class IoU of the training predictions (the only
place the loop reads anything back).  Every cfg.training.checkpoint.test steps the validation scores are logged and
<out_dir>/models/checkpoint_step-XXXXXXXXXX.pth is written.  Nothing is fetched from anywhere."""
import argparse
import json
import math
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "dusty-gan-v2_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gans.config import to_config  # noqa: E402
from semseg.config import default_config, load_config, to_plain  # noqa: E402
from semseg.datasets import GTALiDAR, GTALiDAR_GAN, KITTIRawFrontal, SyntheticFrontal  # noqa: E402
from semseg.metrics import counts_from_confusion  # noqa: E402
from semseg.trainer import Trainer  # noqa: E402
from semseg.utils import InfiniteSampler  # noqa: E402

RAYDROP_MAP = "data/avg_raydrop/kitti_raw_frontal.npy"
MAX_GPUS = 8
CPU_BUDGET = 16   # data-loader workers of all ranks together stay within this many CPUs


def build_datasets(cfg, synthetic):
    """(train, val) for cfg.dataset.name (the reference's table, train_semseg.py:80-106), or the synthetic pair."""
    shape, flip = tuple(cfg.dataset.shape), cfg.dataset.random_flip
    if synthetic:
        n = int(cfg.dataset.num_classes)
        return (SyntheticFrontal(256, shape, n, seed=cfg.random_seed), SyntheticFrontal(32, shape, n, seed=cfg.random_seed + 1))
    name = cfg.dataset.name
    val = KITTIRawFrontal(split="val", shape=shape)
    if name == "kitti_raw_frontal":
        return KITTIRawFrontal(split="train", shape=shape, flip=flip), val
    if name in ("gta_lidar", "gta_lidar_w_uniform_noise"):
        dropout_map = np.load(RAYDROP_MAP)
        if name == "gta_lidar_w_uniform_noise":
            dropout_map.fill(dropout_map.mean())
        return GTALiDAR(shape=shape, flip=flip, raydrop_p=dropout_map), val
    if name == "gta_lidar_wo_noise":
        return GTALiDAR(shape=shape, flip=flip, raydrop_p=None), val
    gan_dirs = {"gta_lidar_w_gan_noise_dustyv1": "GTAV_noise_v1", "gta_lidar_w_gan_noise_dustyv2": "GTAV_noise_v2"}
    if name in gan_dirs:
        return GTALiDAR_GAN(shape=shape, flip=flip, gan_dir=gan_dirs[name]), val
    raise ValueError(name)


def finite_or_none(x):
    """A float for the JSON log: non-finite values (the gradient norm of a step skipped for an overflow) become null."""
    x = float(x)
    return x if math.isfinite(x) else None


def mean_finite(ts):
    """Mean over the finite entries of a list of 0-dim device tensors (one readback), None where there is none."""
    v = torch.stack(ts).double()
    ok = torch.isfinite(v)
    return finite_or_none(v[ok].mean()) if bool(ok.any()) else None


def iou_list(conf, eps=1e-12):
    tp, fp, fn = (t.double().cpu() for t in counts_from_confusion(conf))
    return (tp / (tp + fp + fn + eps)).tolist()


def parse(argv=None):
    """(args, cfg): the command line, and the configuration with its overrides applied and the batch split checked --
    before anything is built and without touching a device."""
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", type=str, default=None)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--max_steps", type=int, default=None)
    ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--out_dir", type=str, default=None)
    ap.add_argument("--no_fused_optimizer", action="store_true")
    ap.add_argument("--num_gpus", type=int, default=1)
    ap.add_argument("--sync_bn", action="store_true")
    args = ap.parse_args(argv)
    if args.config is None and not args.synthetic:
        ap.error("--config or --synthetic is required")
    if not 1 <= args.num_gpus <= MAX_GPUS:
        ap.error(f"--num_gpus must be in 1 .. {MAX_GPUS}, got {args.num_gpus}")

    cfg = load_config(args.config) if args.config else default_config()
    if args.max_steps is not None:
        cfg.training.max_steps = args.max_steps
    if args.batch_size is not None:
        cfg.training.batch_size = args.batch_size
    if cfg.training.batch_size % args.num_gpus != 0:
        raise ValueError(f"training.batch_size ({cfg.training.batch_size}) must be divisible by --num_gpus ({args.num_gpus})")
    cfg.training.num_gpus = args.num_gpus
    cfg.training.batch_size_per_gpu = cfg.training.batch_size // args.num_gpus
    return args, cfg


def workers_per_rank(cfg):
    """cfg.training.num_workers, bounded so that the loaders of all ranks stay within CPU_BUDGET CPUs (each rank's
    main process counts as one)."""
    n = int(cfg.training.num_gpus)
    return max(0, min(int(cfg.training.get("num_workers", 0)), CPU_BUDGET // n - 1))


def training_loop(rank, cfg, opts, temp_dir):
    """One rank's loop (reference: train_semseg.py:65-362).  cfg: plain dicts (it crosses a process boundary)."""
    from pathlib import Path

    from gans.utils import init_dist_process

    cfg = to_config(cfg)
    num_gpus = int(cfg.training.num_gpus)
    device = torch.device("cuda", rank)
    torch.cuda.set_device(device)
    if num_gpus > 1:
        init_dist_process(rank, Path(temp_dir), num_gpus, cfg.random_seed)
    else:
        torch.manual_seed(cfg.random_seed)
        np.random.seed(cfg.random_seed)
    first = rank == 0
    out_dir = opts["out_dir"]
    train_set, val_set = build_datasets(cfg, opts["synthetic"])
    workers = workers_per_rank(cfg)
    per_gpu = int(cfg.training.batch_size_per_gpu)
    sampler = InfiniteSampler(train_set, rank=rank, num_replicas=num_gpus, seed=cfg.random_seed + rank)
    loader = torch.utils.data.DataLoader(train_set, batch_size=per_gpu, num_workers=workers, sampler=sampler, drop_last=True)
    val_loader = torch.utils.data.DataLoader(val_set, batch_size=per_gpu, num_workers=workers) if first else None
    trainer = Trainer(cfg, device, fused_optimizer=not opts["no_fused_optimizer"], pretrained_weights=not opts["synthetic"],
                      sync_bn=opts["sync_bn"])

    ck = cfg.training.checkpoint
    losses, norms = [], []
    batches = iter(loader)
    log = open(os.path.join(out_dir, "train_log.jsonl"), "a") if first else None
    try:
        def emit(row):
            line = json.dumps(row, allow_nan=False)
            log.write(line + "\n")
            log.flush()
            print(line, flush=True)

        for step in range(1, int(cfg.training.max_steps) + 1):
            lr = trainer.optimizer.param_groups[0]["lr"]
            out = trainer.step(next(batches))
            losses.append(out["loss"])
            norms.append(out["grad_norm"])
            last = step == int(cfg.training.max_steps)
            if step % int(ck.stats) == 0 or last:
                conf = trainer.conf_total()   # (a collective with several ranks: every rank is here at this step)
                if first:
                    emit({"step": step, "loss": mean_finite(losses), "lr": lr, "grad_norm": mean_finite(norms),
                          "skipped_steps": int((~torch.isfinite(torch.stack(norms))).sum()), "loss_scale": trainer.loss_scale(),
                          "iou": iou_list(conf), "classes": list(train_set.class_list)})
                trainer.reset_conf()
                losses, norms = [], []
            if first and (step % int(ck.test) == 0 or last):
                val = trainer.validate(val_loader)
                emit({"step": step, "val_iou": [finite_or_none(v) for v in val["iou"]], "val_mean_iou": finite_or_none(val["mean_iou"])})
                torch.save(trainer.state_dict(), os.path.join(out_dir, "models", f"checkpoint_step-{step:010d}.pth"))
    finally:
        if log is not None:
            log.close()
    if num_gpus > 1:
        torch.distributed.destroy_process_group()


def launch(cfg, opts):
    """One rank runs here; several run as fresh child processes, started before this process has touched a GPU (a child
    of the spawn context begins as a new interpreter: nothing of this process's device state is carried over)."""
    num_gpus = int(cfg.training.num_gpus)
    with tempfile.TemporaryDirectory() as temp_dir:
        if num_gpus == 1:
            training_loop(0, to_plain(cfg), opts, temp_dir)
            return 0
        import torch.multiprocessing as mp
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=training_loop, args=(rank, to_plain(cfg), opts, temp_dir)) for rank in range(num_gpus)]
        for p in procs:
            p.start()
        while any(p.is_alive() for p in procs):
            for p in procs:
                p.join(timeout=1.0)
            if any(p.exitcode not in (None, 0) for p in procs):   # a rank died: the others wait in a collective
                for p in procs:
                    if p.is_alive():
                        p.terminate()
        return max(abs(p.exitcode or 0) for p in procs)


def main(argv=None):
    args, cfg = parse(argv)
    out_dir = args.out_dir or os.path.join("logs", "semseg", cfg.dataset.name, cfg.arch.name)
    os.makedirs(os.path.join(out_dir, "models"), exist_ok=True)
    opts = {"out_dir": out_dir, "synthetic": bool(args.synthetic), "no_fused_optimizer": bool(args.no_fused_optimizer),
            "sync_bn": bool(args.sync_bn)}
    return launch(cfg, opts)


if __name__ == "__main__":
    sys.exit(main())
