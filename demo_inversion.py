"""GAN inversion of a measured scan, headless (reference: demo_inversion.py; its options less the display switch).

    python demo_inversion.py --ckpt_path CKPT [--sample_id N | --synthetic] [--optimize_phase] ...

Reads a checkpoint (gans.pretrained.autoload_ckpt) and one KITTI Raw scan (or a synthetic range image), runs
gans.inversion.invert -- (1) latent / phase optimisation, (2) pivotal tuning -- and writes the results as .npy files
into --out_dir: latent, phase, inv_depth, inv_depth_orig, raydrop_prob, loss [steps, 1], target_inv_depth, target_mask.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "dusty-gan-v2_amd")) if p not in sys.path]


def parse(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--ckpt_path", type=str, required=True)
    parser.add_argument("--sample_id", type=int, default=-1)
    parser.add_argument("--latent_type", choices=["z", "w", "w+"], default="w")
    parser.add_argument("--num_steps_1st", type=int, default=500)
    parser.add_argument("--num_steps_2nd", type=int, default=500)
    parser.add_argument("--lr_1st", type=float, default=5e-2)
    parser.add_argument("--lr_1st_rampup_ratio", type=float, default=0.05)
    parser.add_argument("--lr_1st_rampdown_ratio", type=float, default=0.25)
    parser.add_argument("--lr_2nd", type=float, default=5e-4)
    parser.add_argument("--noise_ratio", type=float, default=0.75)
    parser.add_argument("--noise_coef", type=float, default=0.05 / 10)
    parser.add_argument("--optimize_phase", action="store_true")
    parser.add_argument("--perturb_z", action="store_true")
    parser.add_argument("--hypersphere_z", action="store_true")
    parser.add_argument("--device", choices=["cuda"], default="cuda", help="the kernels have no CPU path")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--synthetic", action="store_true",
                        help="a gans.datasets.synthetic.SyntheticRangeImages target instead of a KITTI Raw scan")
    parser.add_argument("--out_dir", type=str, default=".")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    import numpy as np
    import torch

    from gans.coords import CoordBridge, synthetic_angle_grid
    from gans.inversion import invert
    from gans.models.builder import build_generator
    from gans.pretrained import autoload_ckpt
    from gans.utils import init_random_seed

    ckpt = autoload_ckpt(args.ckpt_path)
    cfg = ckpt["cfg"]
    H, W = cfg.model.generator.synthesis_kwargs.resolution
    angle_file = f"data/coords/{cfg.dataset.name}.npy"
    if os.path.exists(angle_file):
        coord = CoordBridge(num_ring=H, num_points=W, min_depth=cfg.dataset.min_depth, max_depth=cfg.dataset.max_depth,
                            angle_file=angle_file)
    else:
        print(f"{angle_file} not found: using the synthetic angle grid", file=sys.stderr)
        coord = CoordBridge(num_ring=H, num_points=W, min_depth=cfg.dataset.min_depth, max_depth=cfg.dataset.max_depth,
                            angle_array=synthetic_angle_grid(H))
    coord.to(args.device)

    G = build_generator(cfg.model.generator)
    G.load_state_dict(ckpt["G_ema"])
    G.eval().to(args.device)

    if args.synthetic:
        from gans.datasets.synthetic import SyntheticRangeImages
        item = next(SyntheticRangeImages((H, W), cfg.dataset.min_depth, cfg.dataset.max_depth, 1, args.device,
                                         seed=args.seed))
        t_depth, t_mask = item["depth"], item["mask"]
        name = "synthetic"
    else:
        from gans.datasets.kitti import KITTIRaw
        dataset = KITTIRaw(root=cfg.dataset.root, split="test", shape=(H, W), min_depth=cfg.dataset.min_depth,
                           max_depth=cfg.dataset.max_depth, device=args.device)
        if args.sample_id == -1:
            args.sample_id = np.random.randint(len(dataset))
        print(f"sample id: {args.sample_id}")
        item = dataset[args.sample_id]
        t_depth, t_mask = item["depth"][None].float(), item["mask"][None].float()
        name = f"{args.sample_id:010d}"

    init_random_seed(random_seed=args.seed)
    generator = torch.Generator(device=args.device)
    generator.manual_seed(args.seed)
    out = invert(G, coord, t_depth, t_mask, latent_type=args.latent_type, num_steps_1st=args.num_steps_1st,
                 num_steps_2nd=args.num_steps_2nd, lr_1st=args.lr_1st, lr_2nd=args.lr_2nd,
                 lr_1st_rampup_ratio=args.lr_1st_rampup_ratio, lr_1st_rampdown_ratio=args.lr_1st_rampdown_ratio,
                 optimize_phase=args.optimize_phase, perturb_z=args.perturb_z, hypersphere_z=args.hypersphere_z,
                 noise_ratio=args.noise_ratio, noise_coef=args.noise_coef, generator=generator)
    t_inv = coord.convert(coord.convert(t_depth.to(args.device), "depth", "depth_norm"), "depth_norm",
                          "inv_depth_norm") * t_mask.to(args.device)
    out.update(target_inv_depth=t_inv, target_mask=t_mask)
    os.makedirs(args.out_dir, exist_ok=True)
    for k, v in out.items():
        path = os.path.join(args.out_dir, f"demo_inversion_{name}_{k}.npy")
        np.save(path, v.detach().cpu().numpy())
    loss = out["loss"]
    if len(loss):
        print(f"loss: first {loss[0].tolist()} last {loss[-1].tolist()}; results in {os.path.abspath(args.out_dir)}")


if __name__ == "__main__":
    main()
