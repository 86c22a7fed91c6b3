"""LiDAR beam upsampling benchmark, headless: hold out beams of dense scans, reconstruct them, score the held-out pixels.

    python eval_upsampling.py --ckpt_path CKPT [--data_root data/kitti_raw] [--factor 4] [--offset 0]
                              [--methods nearest,linear,gan] [--num_steps 500] [--batch_size 32] [--latent_type w+]
                              [--no_graph] [--limit N] [--out scores.json] [--random_seed 0]
    python eval_upsampling.py --synthetic 64 --methods nearest,linear       # no files, no checkpoint

Keeps the rows h % factor == offset of every scan (64 beams -> 16 at the default factor), reconstructs the others by
nearest / linear interpolation between the kept rows (one launch, native.beam_split) and, with `gan`, by fitting the
checkpoint's generator to the sparse scan (gans.sim2real.LatentFitter: stage 1 of demo_inversion.py, the generator
frozen, the step replayed as a hipGraph), and scores the held-out valid pixels with the four depth errors and three
threshold accuracies of gans/metrics/depth.py (one launch, native.depth_score).  The scans are the test split of KITTI
Raw (--data_root, default the checkpoint's cfg.dataset.root) or --synthetic N SyntheticRangeImages scans.  Without `gan`
in --methods no checkpoint is read and no generator is built; the scans then have the resolution and depth range of
configs/gans/dusty_v2.yaml unless a checkpoint is given.  Prints one line per batch, then one JSON line (also written to
--out) with gans.upsampling.UpsamplingBenchmark.summary(), the arguments, the scans per second and whether the fitter
replayed a captured graph.  Nothing is fetched from anywhere."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "dusty-gan-v2_amd")) if p not in sys.path]

# configs/gans/dusty_v2.yaml: what the scans look like when no checkpoint says otherwise
DEFAULT_SHAPE, DEFAULT_MIN_DEPTH, DEFAULT_MAX_DEPTH, DEFAULT_DATA_ROOT = (64, 512), 1.45, 80.0, "data/kitti_raw"
METHODS = ("nearest", "linear", "gan")   # gans.upsampling.METHODS (not imported: parsing must not need the library)


def parse(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--ckpt_path", type=str, default=None, help="needed for the method `gan` only")
    parser.add_argument("--data_root", type=str, default=None, help="KITTI Raw root (default: the checkpoint's cfg.dataset.root)")
    parser.add_argument("--synthetic", type=int, default=None, metavar="N",
                        help="N SyntheticRangeImages scans instead of the files")
    parser.add_argument("--factor", type=int, default=4, help="one row in `factor` is kept")
    parser.add_argument("--offset", type=int, default=0, help="the kept rows are h %% factor == offset")
    parser.add_argument("--methods", type=str, default="nearest,linear,gan")
    parser.add_argument("--num_steps", type=int, default=500)
    parser.add_argument("--batch_size", type=int, default=32)
    parser.add_argument("--latent_type", choices=["z", "w", "w+"], default="w+")
    parser.add_argument("--no_graph", action="store_true", help="run every fitting step eagerly (no hipGraph replay)")
    parser.add_argument("--limit", type=int, default=None, help="score the first LIMIT scans only")
    parser.add_argument("--out", type=str, default=None, metavar="FILE", help="also write the JSON line here")
    parser.add_argument("--random_seed", type=int, default=0)
    args = parser.parse_args(argv)
    args.methods = tuple(m.strip() for m in args.methods.split(",") if m.strip())
    if not args.methods or len(set(args.methods)) != len(args.methods) or any(m not in METHODS for m in args.methods):
        parser.error(f"--methods wants distinct names out of {','.join(METHODS)}, got {','.join(args.methods)!r}")
    if args.factor < 1 or not 0 <= args.offset < args.factor:
        parser.error(f"need --factor >= 1 and 0 <= --offset < --factor, got {args.factor}, {args.offset}")
    if args.batch_size < 1 or args.num_steps < 1 or (args.synthetic is not None and args.synthetic < 1) \
            or (args.limit is not None and args.limit < 1):
        parser.error("--batch_size, --num_steps, --synthetic and --limit must be positive")
    if "gan" in args.methods:   # first of all: a missing file must cost nothing
        if not args.ckpt_path:
            parser.error("the method `gan` needs --ckpt_path")
        if not os.path.isfile(args.ckpt_path):
            parser.error(f"--ckpt_path {args.ckpt_path}: no such file")
    elif args.ckpt_path and not os.path.isfile(args.ckpt_path):
        parser.error(f"--ckpt_path {args.ckpt_path}: no such file")
    return args


def _jsonable(v):
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, float) and not math.isfinite(v):
        return None
    return v


def _batches(args, shape, min_depth, max_depth, root, device):
    """(number of scans, iterator of {"depth", "mask"} batches on `device`)"""
    import torch
    if args.synthetic is not None:
        from gans.evaluation import synthetic_loader
        n = args.synthetic if args.limit is None else min(args.synthetic, args.limit)
        return n, synthetic_loader(num_scans=n, batch_size=args.batch_size, shape=shape, min_depth=min_depth,
                                   max_depth=max_depth, device=device, seed=args.random_seed)
    from gans.datasets.kitti import KITTIRaw
    data = KITTIRaw(root=root, split="test", shape=shape, min_depth=min_depth, max_depth=max_depth, device=device)
    if args.limit is not None and args.limit < len(data):
        data = torch.utils.data.Subset(data, range(args.limit))
    return len(data), torch.utils.data.DataLoader(data, batch_size=args.batch_size, num_workers=0, shuffle=False, drop_last=False)


def main(argv=None):
    args = parse(argv)
    import torch
    from gans.upsampling import UpsamplingBenchmark

    assert torch.cuda.is_available(), "no visible cuda devices"
    device = torch.device("cuda", 0)
    shape, min_depth, max_depth, root = DEFAULT_SHAPE, DEFAULT_MIN_DEPTH, DEFAULT_MAX_DEPTH, DEFAULT_DATA_ROOT
    ckpt = None
    if args.ckpt_path:
        from gans.pretrained import autoload_ckpt
        ckpt = autoload_ckpt(args.ckpt_path)
        cfg = ckpt["cfg"]
        shape = tuple(cfg.model.generator.synthesis_kwargs.resolution)
        min_depth, max_depth, root = cfg.dataset.min_depth, cfg.dataset.max_depth, cfg.dataset.root
    if args.factor > shape[0]:
        raise SystemExit(f"--factor {args.factor} exceeds the {shape[0]} beams of a scan")

    fitter = None
    if "gan" in args.methods:
        from gans.evaluation import build_coord
        from gans.models.builder import build_generator
        from gans.sim2real import DEFAULT_GRAPH, LatentFitter, latent_prior
        from gans.utils import init_random_seed
        G = build_generator(cfg.model.generator)
        G.load_state_dict(ckpt["G_ema"])
        G.eval().to(device)
        init_random_seed(random_seed=args.random_seed)
        generator = torch.Generator(device=device)
        generator.manual_seed(args.random_seed)
        fitter = LatentFitter(G, build_coord(cfg, device), args.batch_size, latent_type=args.latent_type,
                              num_steps=args.num_steps, prior=latent_prior(G, generator=generator),
                              graph=DEFAULT_GRAPH and not args.no_graph, generator=generator)

    total, loader = _batches(args, shape, min_depth, max_depth, args.data_root or root, device)
    bench = UpsamplingBenchmark(args.methods, args.factor, args.offset)
    done = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for item in loader:
        depth = item["depth"].to(device).float().contiguous()
        valid = item["mask"].to(device).float().contiguous()
        bench.update(depth, valid, fitter=fitter)
        torch.cuda.synchronize()   # progress lines tell finished work; the scores themselves are not read back here
        done += len(depth)
        print(f"[{done}/{total}] {done / max(time.perf_counter() - t0, 1e-9):.2f} scans/s", flush=True)
    seconds = time.perf_counter() - t0
    if not done:
        raise SystemExit("no scans to score")
    result = {"methods": bench.summary(), "args": dict(vars(args)), "scans": done, "seconds": seconds,
              "scans_per_second": done / seconds if seconds > 0 else 0.0,
              "captured": bool(fitter.captured) if fitter is not None else False}
    line = json.dumps(_jsonable(result), allow_nan=False)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    return result


if __name__ == "__main__":
    main()
