"""Sim2real ray-drop rendering, headless: one keep-probability map per simulated scan, from a trained generator.

    python render_gan_noise.py --ckpt_path CKPT [--data_root data/kitti_raw_frontal] [--gan_dir GTAV_noise_v2] ...

Reads a checkpoint (gans.pretrained.autoload_ckpt) and the scans semseg.datasets.GTALiDAR lists
(<data_root>/GTAV/<seq>/<name>.npy, [H,W,5] with the depth in channel 3), fits the generator's latent code (and sensor
phase) to every scan (gans.sim2real.LatentFitter: stage 1 of demo_inversion.py, the generator frozen) on the simulator's
angle grid, and writes sigmoid(raydrop_logit) as float32 [H,W] to <data_root>/<gan_dir>/<seq>/<name>.npy: the files
semseg.datasets.GTALiDAR_GAN and configs/semseg/sim2real_w_gan_noise_dustyv*.yaml read.  Scans whose map exists are
skipped, so a killed run is resumed by running it again; --shard I/N takes the scans whose sorted index is I mod N (one
process per GPU).  Prints one progress line per batch and one final JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "dusty-gan-v2_amd")) if p not in sys.path]


def parse_shard(text):
    try:
        i, n = (int(v) for v in text.split("/"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"--shard wants I/N, got {text!r}")
    if not 0 <= i < n:
        raise argparse.ArgumentTypeError(f"--shard {text}: need 0 <= I < N")
    return i, n


def parse(argv=None):
    # the two defaults scripts/mb_sim2real.py decides live beside the fitter
    from gans.sim2real import DEFAULT_BATCH_SIZE
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--ckpt_path", type=str, required=True)
    parser.add_argument("--data_root", type=str, default="data/kitti_raw_frontal")
    parser.add_argument("--gan_dir", type=str, default="GTAV_noise_v2")
    parser.add_argument("--angle_file", type=str, default=None,
                        help="[H0,W0,2] (elevation, azimuth) .npy of the simulator's rays; default: "
                             "gans.coords.frontal_angle_grid at the generator's resolution")
    parser.add_argument("--batch_size", type=int, default=DEFAULT_BATCH_SIZE)
    parser.add_argument("--num_steps", type=int, default=500)
    parser.add_argument("--lr", type=float, default=5e-2)
    parser.add_argument("--latent_type", choices=["z", "w", "w+"], default="w+")
    parser.add_argument("--no_optimize_phase", action="store_true")
    parser.add_argument("--hypersphere_z", action="store_true")
    parser.add_argument("--no_graph", action="store_true", help="run every step eagerly (no hipGraph replay)")
    parser.add_argument("--shard", type=parse_shard, default=(0, 1), metavar="I/N")
    parser.add_argument("--limit", type=int, default=None)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--device", choices=["cuda"], default="cuda", help="the kernels have no CPU path")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    import numpy as np
    import torch

    from gans.coords import CoordBridge, frontal_angle_grid
    from gans.models.builder import build_generator
    from gans.pretrained import autoload_ckpt
    from gans.sim2real import DEFAULT_GRAPH, LatentFitter, gan_path, latent_prior, render_raydrop_maps, scan_list
    from gans.utils import init_random_seed

    ckpt = autoload_ckpt(args.ckpt_path)
    cfg = ckpt["cfg"]
    H, W = cfg.model.generator.synthesis_kwargs.resolution
    min_depth, max_depth = cfg.dataset.min_depth, cfg.dataset.max_depth
    angle = np.load(args.angle_file) if args.angle_file else frontal_angle_grid(H, W)
    coord = CoordBridge(num_ring=H, num_points=W, min_depth=min_depth, max_depth=max_depth, angle_array=angle)
    coord.to(args.device)

    G = build_generator(cfg.model.generator)
    G.load_state_dict(ckpt["G_ema"])
    G.eval().to(args.device)

    init_random_seed(random_seed=args.seed)
    generator = torch.Generator(device=args.device)
    generator.manual_seed(args.seed)
    fitter = LatentFitter(G, coord, args.batch_size, latent_type=args.latent_type, num_steps=args.num_steps, lr=args.lr,
                          optimize_phase=not args.no_optimize_phase, hypersphere=args.hypersphere_z,
                          prior=latent_prior(G, generator=generator), graph=DEFAULT_GRAPH and not args.no_graph,
                          generator=generator)

    scans = scan_list(args.data_root, args.shard, args.limit)
    outs = [gan_path(s, args.gan_dir) for s in scans]
    stats = render_raydrop_maps(fitter, scans, outs, shape=(H, W), min_depth=min_depth, max_depth=max_depth,
                                batch_size=args.batch_size,
                                manifest=os.path.join(args.data_root, args.gan_dir, "manifest.jsonl"),
                                log=lambda line: print(line, flush=True))
    stats.update(shard=f"{args.shard[0]}/{args.shard[1]}", graph=bool(fitter.captured))
    print(json.dumps(stats, allow_nan=False), flush=True)
    return stats


if __name__ == "__main__":
    main()
