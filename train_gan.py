"""Train the GAN (reference: train_gan.py), headless: one process per GPU, gans.trainer.Trainer underneath.

    python train_gan.py --config configs/gans/dusty_v2.yaml [--num_gpus 1] [--resume CKPT] [--dry_run]
                        [--out_dir DIR] [--max_iters N] [--synthetic]
    python train_gan.py --config configs/gans/dusty_v2.yaml --synthetic --max_iters 100   # no data on disk

--config, --num_gpus, --resume and --dry_run are the reference's four.  --out_dir replaces the time-stamped
logs/gans/<dataset>/<G>+<D>/<time> directory, --max_iters N ends the run at iteration N instead of total_kimg,
--synthetic forces dataset.name=synthetic (scans generated in HBM).  --resume takes the log directory from the
checkpoint's path (two levels up) and appends to its log.

Scalars are 100-iteration moving averages; every checkpoint.save_stats iterations one JSON line goes to
<out_dir>/train_log.jsonl and to stdout, the loop's only readback.  Every checkpoint.save_image iterations
<out_dir>/images/{real,fake}_<num_imgs>.npz hold the reference's image panels as uint8 [B, 3 or 1, H, W] under its tags
(image, image/spectrum, normal, pointcloud, image/orig, image/aug, raydrop_prob, raydrop_mask); where tensorboard is
importable the same panels and scalars also go to <out_dir>/tensorboard.  Every checkpoint.validation iterations the
PointNet scores are logged if cls_model_39.pth is on disk (one line says so, once, if it is not).  Checkpoints:
<out_dir>/models/checkpoint_<num_imgs>.pth every checkpoint.save_model iterations and at the end.  --num_gpus N > 1
starts N fresh child processes (spawn) before this process touches a GPU; only rank 0 logs.  Nothing is fetched."""
import argparse
import datetime
import json
import math
import os
import sys
import tempfile
from collections import defaultdict, deque
from pathlib import Path

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "dusty-gan-v2_amd")) if p not in sys.path]

MAX_GPUS = 16
REAL_TAGS = ("image", "image/spectrum", "normal", "pointcloud", "raydrop_mask", "image/aug")
FAKE_TAGS = ("image", "image/spectrum", "normal", "pointcloud", "image/orig", "raydrop_prob", "raydrop_mask")
BEV_T = (0.0, 0.0, 0.7)   # the camera of the "pointcloud" panel (reference: train_gan.py:60)


def plain(o):
    """A Config tree as plain dicts / lists (what yaml.safe_dump and pickle take)."""
    if isinstance(o, dict):
        return {k: plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [plain(v) for v in o]
    return o


def parse(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--config", type=str, required=True)
    parser.add_argument("--num_gpus", type=int, default=1)
    parser.add_argument("--resume", type=str, default=None)
    parser.add_argument("--dry_run", action="store_true")
    parser.add_argument("--out_dir", type=str, default=None)
    parser.add_argument("--max_iters", type=int, default=None, metavar="N", help="end at iteration N, not at total_kimg")
    parser.add_argument("--synthetic", action="store_true", help="dataset.name=synthetic: scans generated in HBM")
    args = parser.parse_args(argv)
    if not 1 <= args.num_gpus <= MAX_GPUS:
        parser.error(f"--num_gpus must be in 1 .. {MAX_GPUS}, got {args.num_gpus}")
    if args.max_iters is not None and args.max_iters < 0:
        parser.error("--max_iters must not be negative")
    return args


def derive_config(args):
    """The configuration of the run: the file, --synthetic, and the machine-dependent keys (reference:
    train_gan.py:177-187, 194).  The reference also records a num_workers guess from the host's CPU count; the loaders
    here run in the training process (the projection is a GPU kernel), so no such key is written."""
    from gans.config import load_config
    cfg = load_config(args.config)
    if args.synthetic:
        cfg.dataset.name = "synthetic"
    if cfg.training.batch_size % args.num_gpus != 0:
        raise ValueError(f"training.batch_size ({cfg.training.batch_size}) must be divisible by --num_gpus ({args.num_gpus})")
    cfg.training.num_gpus = args.num_gpus
    cfg.training.batch_size_per_gpu = cfg.training.batch_size // args.num_gpus
    cfg.training.rank = 0   # every child writes its own
    cfg.training.resume = args.resume
    return cfg


def log_dir_for(args, cfg, now=None):
    """Where the run logs (reference: train_gan.py:195-203): --resume CKPT continues <dir>/models/CKPT's <dir>."""
    if args.resume is not None:
        return Path(args.resume).parents[1]
    if args.out_dir is not None:
        return Path(args.out_dir)
    stamp = (now or datetime.datetime.now()).strftime("%Y%m%dT%H%M%S")
    return Path("logs/gans") / f"{cfg.dataset.name}" / f"{cfg.model.generator.arch}+{cfg.model.discriminator.arch}" / stamp


def total_iterations(args, cfg):
    if args.max_iters is not None:
        return int(args.max_iters)
    return int(int(cfg.training.total_kimg * 1e3) / cfg.training.batch_size)


def json_line(row):
    def num(v):
        if isinstance(v, (int, str)) or v is None:
            return v
        v = float(v)
        return v if math.isfinite(v) else None
    return json.dumps({k: num(v) for k, v in row.items()}, allow_nan=False)


def image_panels(converter, image=None, image_orig=None, image_aug=None, raydrop_logit=None, raydrop_mask=None):
    """tag -> float panel [B, 3 or 1, H, W] in [0, 1] on the device (reference: log_images, train_gan.py:29-68)."""
    import torch
    from gans.render import render_point_clouds
    from gans.utils import colorize, points_to_normal_2d, power_spectrum_2d, tanh_to_sigmoid
    panels = {}
    if image_orig is not None:
        panels["image/orig"] = colorize(tanh_to_sigmoid(image_orig).clamp(0, 1))
    if image_aug is not None:
        panels["image/aug"] = colorize(tanh_to_sigmoid(image_aug).clamp(0, 1))
    if raydrop_logit is not None:
        panels["raydrop_prob"] = colorize(torch.sigmoid(raydrop_logit))
    if raydrop_mask is not None:
        panels["raydrop_mask"] = raydrop_mask.float()
    if image is not None:
        inv_depth = tanh_to_sigmoid(image).clamp(0, 1)
        points_map = converter.convert(inv_depth, "inv_depth_norm", "point_map") / converter.max_depth
        normal_map = points_to_normal_2d(points_map, mode="closest")
        bev = render_point_clouds(points=points_map.flatten(2).transpose(1, 2), colors=normal_map.flatten(2).transpose(1, 2),
                                  t=torch.tensor(BEV_T, device=inv_depth.device))
        spectrum = power_spectrum_2d(inv_depth)
        spectrum = spectrum - spectrum.min()
        spectrum = spectrum / spectrum.max()
        panels.update({"image": colorize(inv_depth), "image/spectrum": colorize(spectrum), "normal": normal_map,
                       "pointcloud": bev})
    return panels


def to_uint8(panels):
    import torch
    return {k: (v.detach().float().clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy() for k, v in panels.items()}


class RunLog:
    """Rank 0's outputs: the JSON-lines log, the image files and, where tensorboard imports, a SummaryWriter."""

    def __init__(self, log_dir):
        self.dir = Path(log_dir)
        (self.dir / "images").mkdir(parents=True, exist_ok=True)
        self.file = open(self.dir / "train_log.jsonl", "a")
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.writer = SummaryWriter(log_dir=str(self.dir / "tensorboard"))
        except ImportError:
            self.writer = None

    def line(self, row):
        text = json_line(row)
        self.file.write(text + "\n")
        self.file.flush()
        print(text, flush=True)
        if self.writer is not None:
            for k, v in row.items():
                if k not in ("iteration", "num_imgs") and isinstance(v, float) and math.isfinite(v):
                    self.writer.add_scalar(k, v, row["num_imgs"])

    def images(self, tag, num_imgs, panels):
        import numpy as np
        np.savez(self.dir / "images" / f"{tag}_{num_imgs:010d}.npz", **panels)
        if self.writer is not None:
            for k, v in panels.items():
                self.writer.add_images(f"{tag}/{k}", v, num_imgs, dataformats="NCHW")

    def close(self):
        self.file.close()
        if self.writer is not None:
            self.writer.close()


def seed_and_connect(rank, cfg, temp_dir):
    """Seed python, numpy and torch with cfg.random_seed + rank and, with several ranks, join the process group
    (reference: train_gan.py:79).  It runs before Trainer(cfg): the weights, z_fixed and the device's Philox stream
    (seeded from torch's seed of that moment) all follow this seed.  One rank needs no process group, only the seed."""
    from gans.utils import init_dist_process, init_random_seed
    if cfg.training.num_gpus > 1:
        init_dist_process(rank, Path(temp_dir), cfg.training.num_gpus, cfg.random_seed)
    else:
        init_random_seed(cfg.random_seed, rank)


def training_loop(rank, cfg, temp_dir, log_dir, total_iters):
    """One rank's loop (reference: train_gan.py:71-166)."""
    import torch
    from gans.config import to_config
    from gans.trainer import Trainer

    cfg = to_config(cfg)
    cfg.training.rank = rank
    seed_and_connect(rank, cfg, temp_dir)
    trainer = Trainer(cfg, sync_scalars=False)   # scalars stay on the device until a log line reads their mean
    first = rank == 0
    if first:
        info = torch.cuda.get_device_properties(trainer.device)
        print(f"rank 0: {info.name} {info.total_memory / 1024 ** 3:g} GB; batch {cfg.training.batch_size} = "
              f"{cfg.training.num_gpus} x {cfg.training.batch_size_per_gpu}; iterations {trainer.start_iteration + 1:,} .. "
              f"{total_iters:,}; log directory {log_dir}", flush=True)
        log = RunLog(log_dir)
        reals = trainer.fetch_reals(next(trainer.iter_train_loader))
        reals = {k: v.clone() for k, v in reals.items()}
        real_panels = to_uint8(image_panels(trainer.coord, image=reals["image"], raydrop_mask=reals["raydrop_mask"]))
    ck = cfg.training.checkpoint
    moving_avg = defaultdict(lambda: deque(maxlen=100))
    pointnet = None   # loaded at the first validation; False once the weights were found missing

    for i in range(trainer.start_iteration + 1, total_iters + 1):
        scalars = trainer.step(i)
        num_imgs = trainer.iters_to_imgs(i)
        for key, value in scalars.items():
            # (a captured body's scalars are static buffers that the next replay overwrites)
            moving_avg[key].append(value.detach().clone() if torch.is_tensor(value) else value)
        if not first:
            continue

        if i % int(ck.save_image) == 0:
            with torch.no_grad():
                aug = to_uint8(image_panels(trainer.coord, image_aug=trainer.A(trainer.warmup(reals["image"]))))
                log.images("real", num_imgs, {**real_panels, **aug})
                fakes = trainer.sample(ema=True)
                log.images("fake", num_imgs, to_uint8(image_panels(
                    trainer.coord, image=fakes.get("image"), image_orig=fakes.get("image_orig"),
                    raydrop_logit=fakes.get("raydrop_logit"), raydrop_mask=fakes.get("raydrop_mask"))))

        if i % int(ck.validation) == 0 and pointnet is not False:
            if pointnet is None:
                from gans.metrics.pointnet import pretrained_pointnet
                try:
                    pointnet = pretrained_pointnet()
                except FileNotFoundError as e:
                    pointnet = False
                    print(f"validation skipped for this run: {e}", flush=True)
            if pointnet is not False:
                scores = trainer.validation(pointnet=pointnet)
                log.line({"iteration": i, "num_imgs": num_imgs, **{"score/" + k: float(v) for k, v in scores.items()}})

        if i % int(ck.save_model) == 0:
            trainer.save_checkpoint(Path(log_dir) / f"models/checkpoint_{num_imgs:010d}.pth", num_imgs)

        if i % int(ck.save_stats) == 0:
            keys = sorted(moving_avg)
            host = {k: sum(moving_avg[k]) / len(moving_avg[k]) for k in keys if not torch.is_tensor(moving_avg[k][0])}
            dev = [k for k in keys if k not in host]
            if dev:   # one readback for every device scalar
                means = torch.stack([torch.stack([v.reshape(()).float() for v in moving_avg[k]]).mean() for k in dev]).cpu()
                host.update(zip(dev, means.tolist()))
            trainer.check_status()
            log.line({"iteration": i, "num_imgs": num_imgs, **{k: host[k] for k in keys}})

    if first:
        num_imgs = trainer.iters_to_imgs(total_iters)
        trainer.save_checkpoint(Path(log_dir) / f"models/checkpoint_{num_imgs:010d}.pth", num_imgs)
        log.close()
    if cfg.training.num_gpus > 1:
        torch.distributed.destroy_process_group()


def launch(cfg, log_dir, total_iters):
    """One rank runs here; several run as fresh child processes, started before this process has touched a GPU (a child
    of the spawn context begins as a new interpreter, nothing of this process's device state is carried over)."""
    num_gpus = int(cfg.training.num_gpus)
    with tempfile.TemporaryDirectory() as temp_dir:
        if num_gpus == 1:
            training_loop(0, plain(cfg), temp_dir, str(log_dir), total_iters)
            return 0
        import torch.multiprocessing as mp
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=training_loop, args=(rank, plain(cfg), temp_dir, str(log_dir), total_iters))
                 for rank in range(num_gpus)]
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
    import yaml
    args = parse(argv)
    cfg = derive_config(args)
    if args.dry_run:
        print(yaml.safe_dump(plain(cfg), sort_keys=False), flush=True)
        return 0
    log_dir = log_dir_for(args, cfg)
    log_dir.mkdir(parents=True, exist_ok=True)
    if args.resume is None:
        with open(log_dir / "training_config.yaml", "w") as f:
            yaml.safe_dump(plain(cfg), f, sort_keys=False)
    return launch(cfg, log_dir, total_iterations(args, cfg))


if __name__ == "__main__":
    sys.exit(main())
