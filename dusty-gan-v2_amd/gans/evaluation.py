"""Scoring a trained generator by the paper's protocol on one GPU (reference: test_gan.py:26-250).

    summary = collect_sets(ckpt, train_loader, test_loader, num_samples, batch_size, seed, device)
    scores = score_sets(summary, ("swd", "jsd", "1nna", "fpd", "kpd"))

collect_sets restates `preprocess` (test_gan.py:26-164) for one process that owns one GPU: no spawn, no queue, nothing
to sort by rank.  score_sets restates the metric blocks of `evaluate` (test_gan.py:215-249).  What differs from the
reference in plumbing:

  * the ray-drop noise -- one uniform map per run, shared by every generated sample -- reaches the generator through
    its `noise={"gumbel_u": ...}` argument, so the fused output stage runs; the reference's forward hook on the
    GumbelSigmoid module (test_gan.py:95-100) still works through the generator's modular fallback;
  * the latents are `torch.randn(num_samples, mapping_kwargs.in_ch)` -- 512 in every published configuration, which is
    what the reference hard-codes (test_gan.py:184);
  * furthest point sampling picks min(cfg.validation.num_points, H * W) points: a scan has no more;
  * the "emd" matrices of 1-NNA come from the match-free all-pairs kernel by default (`engine`).
"""
import os

import torch

from gans.utils import init_random_seed, sigmoid_to_tanh, tanh_to_sigmoid

METRICS = ("swd", "jsd", "1nna", "fpd", "kpd")
SET_NAMES = ("train", "test", "gen")


def parse_metrics(text):
    """"swd, jsd" -> ["swd", "jsd"] (test_gan.py:261); a name outside METRICS is an error here, not a silent no-op."""
    names = text.replace(" ", "").split(",")
    bad = [n for n in names if n not in METRICS]
    if bad:
        raise ValueError(f"unknown metric(s) {bad}: choose from {list(METRICS)}")
    return names


def needs_features(metrics):
    return "fpd" in metrics or "kpd" in metrics


def subsample(batch, n):
    """At most n rows at evenly spaced indices (test_gan.py:167-171)."""
    if len(batch) <= n:
        return batch
    return batch[torch.linspace(0, len(batch), n + 1)[:-1].long()]


def synthetic_loader(num_scans, batch_size, shape, min_depth, max_depth, device, seed):
    """`num_scans` scans of SyntheticRangeImages in batches of `batch_size` (the last one may be shorter); no files."""
    from gans.datasets.synthetic import SyntheticRangeImages
    source = SyntheticRangeImages(shape, min_depth, max_depth, batch_size, device, seed=seed)
    for lo in range(0, num_scans, batch_size):
        item = next(source)
        yield {k: v[:num_scans - lo] for k, v in item.items()}


def build_coord(cfg, device):
    """The depth <-> point cloud converter of the checkpoint's dataset (test_gan.py:80-88); the synthetic angle grid
    stands in where data/coords/<name>.npy is not on disk."""
    from gans.coords import CoordBridge, synthetic_angle_grid
    H, W = cfg.model.generator.synthesis_kwargs.resolution
    kw = dict(num_ring=H, num_points=W, min_depth=cfg.dataset.min_depth, max_depth=cfg.dataset.max_depth)
    angle_file = f"data/coords/{cfg.dataset.name}.npy"
    if os.path.exists(angle_file):
        coord = CoordBridge(angle_file=angle_file, **kw)
    else:
        coord = CoordBridge(angle_array=synthetic_angle_grid(H), **kw)
    return coord.to(device)


@torch.no_grad()
def collect_sets(ckpt_or_path, train_loader, test_loader, num_samples, batch_size, seed, device, pointnet=None,
                 features=True, record=None):
    """{"train-imgs", "train-points", "train-feats", "test-...", "gen-..."}: host tensors, one row per scan.

    imgs [N, 1, H, W] inverse depth in [0, 1] with dropped rays at the ray-drop constant; points [N, P, 3] / max_depth,
    furthest-point sampled; feats [N, 1808] PointNet features of the full cloud (absent with features=False: no PointNet
    is built then).  The loaders yield {"depth", "mask"} batches.  pointnet=None: pretrained_pointnet().
    record: a dict that receives "uniform" [1, H, W] (the run's ray-drop noise map) and the generator's
    "raydrop_logit" / "raydrop_mask" for every generated sample, where it returns them."""
    from gans.models.builder import build_generator
    from gans.pretrained import autoload_ckpt
    from gans.sampling.fps import downsample_point_clouds

    device = torch.device(device)
    if features and pointnet is None:   # before anything is built or generated: a missing file ends the run here
        from gans.metrics.pointnet import pretrained_pointnet
        pointnet = pretrained_pointnet()
    ckpt = autoload_ckpt(ckpt_or_path) if isinstance(ckpt_or_path, (str, os.PathLike)) else ckpt_or_path
    cfg = ckpt["cfg"]
    H, W = cfg.model.generator.synthesis_kwargs.resolution
    num_points = min(int(cfg.validation.num_points), H * W)
    raydrop_const = cfg.model.generator.measurement_kwargs.raydrop_const

    init_random_seed(seed)
    latents = torch.randn(num_samples, cfg.model.generator.mapping_kwargs.in_ch)   # on the host, as the reference draws them
    init_random_seed(seed)

    angle = ckpt["angle"].to(device)
    coord = build_coord(cfg, device)
    G = build_generator(cfg.model.generator)
    G.load_state_dict(ckpt["G_ema"])
    G.eval().to(device)
    if features:
        pointnet = pointnet.eval().to(device)

    # deterministic ray-drop: one clamped uniform map (clamp_probs) for every generated sample (test_gan.py:95-100)
    eps = torch.finfo(torch.float32).eps
    uniform = torch.rand(1, H, W, device=device).clamp_(eps, 1.0 - eps)

    def clouds(imgs):
        points = coord.convert(imgs, "inv_depth_norm", "point_set")
        points = points / coord.max_depth
        out = [imgs.cpu(), downsample_point_clouds(points, num_points).cpu()]
        if features:
            out.append(pointnet(points.transpose(1, 2)).cpu())
        return out

    def transform_reals(imgs, mask):
        imgs, mask = imgs.to(device).float(), mask.to(device).float()
        imgs = coord.convert(imgs.contiguous(), "depth", "inv_depth_norm")
        imgs = sigmoid_to_tanh(imgs)
        imgs = mask * imgs + (1 - mask) * raydrop_const
        return clouds(tanh_to_sigmoid(imgs).clamp(0, 1))

    def transform_fakes(imgs):
        return clouds(tanh_to_sigmoid(imgs).clamp(0, 1))

    summary = {}

    def add(name, parts):
        for key, value in zip(("imgs", "points", "feats"), parts):
            summary.setdefault(f"{name}-{key}", []).append(value)

    for name, loader in (("train", train_loader), ("test", test_loader)):
        for item in loader:
            add(name, transform_reals(item["depth"], item["mask"]))
    logits, masks = [], []
    for lo in range(0, num_samples, batch_size):
        z = latents[lo:lo + batch_size].to(device)
        out = G(z=z, angle=angle.repeat_interleave(len(z), dim=0),
                noise={"gumbel_u": uniform[None].expand(len(z), 1, H, W)})
        add("gen", transform_fakes(out["image"]))
        if "raydrop_logit" in out and "raydrop_mask" in out:
            logits.append(out["raydrop_logit"].cpu())
            masks.append(out["raydrop_mask"].cpu())
    if record is not None:
        record["uniform"] = uniform.cpu()
        if logits:
            record["raydrop_logit"], record["raydrop_mask"] = torch.cat(logits), torch.cat(masks)
    return {k: torch.cat(v, dim=0) for k, v in summary.items()}


@torch.no_grad()
def score_sets(summary, metrics, engine="pairwise", device="cuda"):
    """The metric blocks of test_gan.py:215-249 on what collect_sets returned; `engine`: how the EMD matrices of 1-NNA
    are computed (gans.metrics.cov_mmd_1nna.compute_cov_mmd_1nna)."""
    from gans.metrics.cov_mmd_1nna import compute_cov_mmd_1nna
    from gans.metrics.fpd_kpd import compute_frechet_distance, compute_squared_mmd
    from gans.metrics.jsd import compute_jsd
    from gans.metrics.swd import compute_swd

    for name in metrics:
        if name not in METRICS:
            raise ValueError(f"unknown metric {name!r}: choose from {list(METRICS)}")
    scores = {}
    if "swd" in metrics:     # as inverse depth images
        scores.update(compute_swd(img1=subsample(summary["gen-imgs"], 2048).to(device),
                                  img2=subsample(summary["test-imgs"], 2048).to(device)))
    if "jsd" in metrics:     # as point clouds
        scores["jsd"] = compute_jsd(pcs_gen=subsample(summary["gen-points"], 2048).to(device) / 2,
                                    pcs_ref=subsample(summary["test-points"], 2048).to(device) / 2)
    if "1nna" in metrics:    # as point clouds
        scores.update(compute_cov_mmd_1nna(pcs_gen=subsample(summary["gen-points"], 2048).to(device),
                                           pcs_ref=subsample(summary["test-points"], 2048).to(device),
                                           batch_size=256, metrics=("emd",), engine=engine))
    if "fpd" in metrics:     # as pointnet features
        scores["fpd"] = compute_frechet_distance(feats1=summary["gen-feats"].cpu().numpy(),
                                                 feats2=summary["train-feats"].cpu().numpy())
    if "kpd" in metrics:
        scores["kpd"] = compute_squared_mmd(feats1=summary["gen-feats"].cpu().numpy(),
                                            feats2=summary["train-feats"].cpu().numpy())
    return scores
